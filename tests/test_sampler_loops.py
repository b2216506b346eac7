"""`DiffusionSampler.sample` / `inpaint` on a ragged batch whose trajectory stays inside the cutoff (tests/_sampler_cases.py): the device
loops against float64 replays of the same noise, every network call teacher-forced on the replay's state, and the parts of sampler.py
that the golden fixtures never reach - `timesteps=`, the cosine schedule, `return_frames`, non-unit normalisation, the graphed loop on
ragged batches / with one step / with noise refills, `step_callback`, the three `on_nan` policies, `sample_sharded` on a device."""
import warnings

import pytest
import torch

import _sampler_cases as sc
from _cases import rel

pytestmark = pytest.mark.gpu
TOL = 1e-5            # one network call on identical inputs (the project's bar)
TRAJ = 5e-5           # a whole trajectory against its float64 replay (the bar of tests/test_sampler.py)
POS = sc.POS


def _dynamics(dev):
    from oareactdiff_amd import EGNNDynamics
    dyn = EGNNDynamics(model_config=dict(sc.CFG), fragment_names=["R", "TS", "P"], node_nfs=sc.NODE_NFS, edge_nf=0, condition_nf=1,
                       device=dev)
    dyn.load_state_dict(sc.weights(), strict=True)
    return dyn


def _sampler(dyn, schedule, T, pos_only, **kw):
    from oareactdiff_amd import DiffusionSampler
    return DiffusionSampler(dyn, schedule, T, sc.PRECISION, pos_only=pos_only, gaussian_prior_std=1.0, **kw)


def _flat(xs, sl):
    return torch.cat([torch.as_tensor(x)[:, sl].detach().cpu().double().reshape(-1) for x in xs])


def _inside_cutoff(r, b):
    assert r.min_active == b.inner, (f"trajectory left the cutoff: {r.min_active} of {b.inner} same-object edges active in the emptiest "
                                     f"of {len(r.calls)} network calls (max |pos| {r.max_pos:.1f})")


def _device_inside_cutoff(smp, b):
    """`_inside_cutoff` looks at the replay, which adds the prior term itself.  The device's own run is held to the same condition on
    what it leaves behind: every same-object pair of its final state inside the cutoff (measured: 4.9 ... 5.2 A against 10 A; a
    loop that dropped the prior term ends at |pos| ~ 470 A and fails here, and at the final-position gate)."""
    worst = 0.0
    for x, m in zip(smp.last_x, b.masks):
        p = x[:, :POS].detach().cpu().double()
        d = torch.cdist(p, p)
        assert bool(torch.isfinite(d).all())
        worst = max(worst, float(d[m[:, None] == m[None, :]].max()))
    assert worst < sc.CFG["cutoff"], f"device trajectory left the cutoff: same-object pair at {worst:.1f} A in its final state"
    return worst


def _compare(title, r, smp, dyn, pos_only, dev):
    """Final state against the replay, then every network call of the replay on the device (identical float32 inputs)."""
    b = sc.batch()
    far = _device_inside_cutoff(smp, b)
    print(f"{title}: largest same-object pair distance of the device's final state {far:.2f} A")
    ep = rel(_flat(smp.last_x, slice(0, POS)), _flat(r.x64, slice(0, POS)))
    eh = 0.0 if pos_only else rel(_flat(smp.last_x, slice(POS, None)), _flat(r.x64, slice(POS, None)))
    vel, feat = [], []
    ei, cond, nfs, cm = b.ei.to(dev), b.cond.to(dev), b.nfs.to(dev), b.cm.to(dev)
    for z32, t32, o, _ in r.calls:
        with torch.no_grad():
            out, _ = dyn([z.to(dev) for z in z32], ei, t32.to(dev), cond, nfs, cm)
        vel.append(rel(_flat(out, slice(0, POS)), _flat(o, slice(0, POS))))
        feat.append(rel(_flat(out, slice(POS, None)), _flat(o, slice(POS, None))))
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"{title}: final positions {ep:.2e} features {eh:.2e} after {len(r.calls)} network calls ({r.min_active} of {b.inner} same-object "
          f"edges active in every call, max |pos| {r.max_pos:.1f}); per call on identical inputs: velocity worst {max(vel):.2e} median "
          f"{med(vel):.2e}, features worst {max(feat):.2e} median {med(feat):.2e}")
    return ep, eh, max(vel), max(feat)


# Measured on an MI355X, suite launch shapes / OARD_TEST_SHAPES=auto; 3 160 of 3 160 same-object edges active in every call of every case:
#   case                         final pos  final h   per call velocity worst (median)             per call features worst (median)
#   polynomial_2_posonly  (17)   4.86e-07   -         1.45e-06 (7.33e-07) / 1.05e-06 (6.93e-07)    3.15e-07 (2.41e-07) / 3.01e-07 (2.44e-07)
#   cosine_full           (17)   3.64e-07   3.32e-07  1.32e-06 (5.89e-07) / 1.50e-06 (5.66e-07)    2.46e-07 (1.57e-07) / 2.21e-07 (1.54e-07)
#   polynomial_2_8_of_16  (9)    1.29e-06   -         1.11e-06 (7.56e-07) / 9.48e-07 (6.76e-07)    3.29e-07 (2.78e-07) / 3.25e-07 (2.53e-07)
#   inpaint               (22)   2.29e-07   -         1.02e-06 (6.81e-07) / 9.91e-07 (6.30e-07)    3.46e-07 (2.54e-07) / 3.78e-07 (2.67e-07)
# against the bars TRAJ = 5e-5 (final state) and TOL = 1e-5 (one call).
SAMPLE_CASES = {
    "polynomial_2_posonly": ("polynomial_2", 16, 16, True),
    "cosine_full": ("cosine", 16, 16, False),
    "polynomial_2_8_of_16_steps": ("polynomial_2", 16, 8, True),
}


@pytest.mark.parametrize("case", list(SAMPLE_CASES))
def test_sample_tracks_the_f64_replay_inside_the_cutoff(case):
    schedule, T, n_steps, pos_only = SAMPLE_CASES[case]
    dev = torch.device("cuda:0")
    b = sc.batch()
    r = sc.replay("sample", schedule, T, n_steps, pos_only)
    assert len(r.calls) == n_steps + 1
    _inside_cutoff(r, b)
    dyn = _dynamics(dev)
    smp = _sampler(dyn, schedule, T, pos_only)
    out, masks = smp.sample(b.B, b.frag, conditions=b.cond, h0=b.h0 if pos_only else None, noise_fn=b.noise,
                            timesteps=None if n_steps == T else n_steps)
    assert int(smp.last_status[0].item()) == 0
    ep, eh, wv, wh = _compare(f"sample {case}", r, smp, dyn, pos_only, dev)
    assert ep <= TRAJ and eh <= TRAJ
    assert wv <= TOL and wh <= TOL
    assert len(out) == 1 and [tuple(o.shape) for o in out[0]] == [(n, 9) for n in b.sizes]
    assert all(torch.equal(m.cpu(), mm) for m, mm in zip(masks, b.masks))


def test_inpaint_tracks_the_f64_replay_inside_the_cutoff():
    """T = 12, 2 resamplings, jump length 3, R and P fixed, with the Gaussian-prior term: without it the generated object leaves the
    cutoff (|pos| ~ 470 A) and the network would be gated on an empty radius graph for it.  The replay's condition
    ("trajectory left the cutoff") guards the REPLAY, whose callback adds the term; an `inpaint` that ignored
    `gaussian_prior_std` is caught on the device side: `_device_inside_cutoff` and the final-position gate (rel 151 when tried)."""
    dev = torch.device("cuda:0")
    b = sc.batch()
    r = sc.replay("inpaint", "polynomial_2", 12, 12, True)
    assert len(r.calls) == 22
    _inside_cutoff(r, b)
    dyn = _dynamics(dev)
    smp = _sampler(dyn, "polynomial_2", 12, True)
    out, _ = smp.inpaint(b.B, b.frag, conditions=b.cond, resamplings=2, jump_length=3, xh_fixed=[x.clone() for x in b.xh_fixed],
                         frag_fixed=[0, 2], noise_fn=b.noise)
    assert int(smp.last_status[0].item()) == 0
    ep, _, wv, wh = _compare("inpaint", r, smp, dyn, True, dev)
    assert ep <= TRAJ
    assert wv <= TOL and wh <= TOL
    for k in range(3):                                       # pos_only: the returned features are those of xh_fixed
        assert torch.equal(out[0][k][:, POS:].cpu().float(), b.h0[k])


def test_frames_and_normalisation():
    """`return_frames=4`, norm_values (1, 4, 10), norm_biases (0, 0.5, 0).  Frame i is the un-normalised state after the step to
    s = i T / 4 (en_diffusion.py:531-534), frame 0 the post-processed final sample (:554-557).  The normalisation touches what is
    returned only: the trajectory is that of the plain run, bit for bit.  (The reference's `unnormalize_z` writes into the running
    state when the constants are not the identity; the frames here are copies.)"""
    dev = torch.device("cuda:0")
    b = sc.batch()
    T, frames = 16, 4
    nv, nb = (1.0, 4.0, 10.0), (0.0, 0.5, 0.0)
    r = sc.replay("sample", "cosine", T, T, False)
    _inside_cutoff(r, b)
    assert len(r.trace) == T
    dyn = _dynamics(dev)
    plain = _sampler(dyn, "cosine", T, False)
    plain.sample(b.B, b.frag, conditions=b.cond, noise_fn=b.noise, graph=False)
    want_x = [x.clone() for x in plain.last_x]
    smp = _sampler(dyn, "cosine", T, False, norm_values=nv, norm_biases=nb)
    out, _ = smp.sample(b.B, b.frag, conditions=b.cond, noise_fn=b.noise, return_frames=frames)
    assert len(out) == frames
    for a, c in zip(smp.last_x, want_x):
        assert torch.equal(a, c)
    blocks = ((slice(0, POS), 0), (slice(POS, -1), 1), (slice(-1, None), 2))
    for i in range(1, frames):
        s = i * T // frames
        state = r.trace[T - 1 - s]                            # the trace holds the states after the steps to s = T - 1, ..., 0
        for sl, j in blocks:
            e = rel(_flat(out[i], sl), _flat([z[:, sl] * nv[j] + nb[j] for z in state], slice(None)))
            print(f"frame {i} (state at s = {s}), block {j}: {e:.2e}")
            assert e <= TRAJ                                 # measured (MI355X, both launch-shape settings): 1.40e-07 ... 6.30e-07
    e = rel(_flat(out[0], slice(0, POS)), _flat(r.x64, slice(0, POS)))
    print(f"frame 0 positions: {e:.2e}")
    assert e <= TRAJ                                         # measured: 3.64e-07
    for k in range(3):
        x = r.x64[k]
        cat = torch.nn.functional.one_hot(torch.argmax(x[:, POS:-1] * nv[1] + nb[1], dim=1), 5)
        charge = torch.round(x[:, -1:] * nv[2] + nb[2])
        assert torch.equal(out[0][k][:, POS:-1].cpu().long(), cat)
        assert torch.equal(out[0][k][:, -1:].cpu().double(), charge)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_graphed_loop_is_bitwise_the_eager_loop_on_ragged_batches():
    dev = torch.device("cuda:0")
    dyn = _dynamics(dev)
    b = sc.batch()
    for pos_only, schedule in ((True, "polynomial_2"), (False, "cosine")):
        smp = _sampler(dyn, schedule, 16, pos_only)
        h0 = b.h0 if pos_only else None

        def run(graph, seed=None, **kw):
            if seed is not None:
                torch.manual_seed(seed)
            out, _ = smp.sample(b.B, b.frag, conditions=b.cond, h0=h0, noise_fn=None if seed is not None else b.noise, graph=graph, **kw)
            assert bool(all(torch.isfinite(x).all() for x in smp.last_x))
            return [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]]
        eager = run(False)
        assert _same(eager, run(True))
        assert _same(eager, run(None))                              # B = 5: the automatic choice is the graphed loop
        eager_rng = run(False, seed=31)
        assert _same(eager_rng, run(True, seed=31))
        assert not _same(eager_rng[:3], eager[:3])
        # one step: the graph is never captured (the warm-up step is the whole loop)
        assert _same(run(False, timesteps=1), run(True, timesteps=1))
        assert _same(run(False, seed=32, timesteps=1), run(True, seed=32, timesteps=1))
        # room for 5 steps of noise per block: refills before replays 6, 11 and 16, in the eager loop's draw order
        old = smp.noise_block_bytes
        smp.noise_block_bytes = 5 * 4 * sum(n * 9 for n in b.sizes)
        try:
            assert _same(eager_rng, run(True, seed=31))
            assert _same(eager, run(True))
        finally:
            smp.noise_block_bytes = old
    # B = 12 (above the automatic threshold of 8): the graphed loop forced
    b12 = sc.batch(12)
    smp = _sampler(dyn, "polynomial_2", 16, True)
    got = {}
    for graph in (False, True, None):
        torch.manual_seed(33)
        out, _ = smp.sample(b12.B, b12.frag, conditions=b12.cond, h0=b12.h0, graph=graph)
        got[graph] = [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]]
        assert bool(all(torch.isfinite(x).all() for x in smp.last_x))
    assert _same(got[False], got[True]) and _same(got[False], got[None])


@pytest.mark.parametrize("graph", [False, True, None])
def test_step_callback_sees_every_call_in_order(graph):
    dev = torch.device("cuda:0")
    dyn = _dynamics(dev)
    b = sc.batch()
    smp = _sampler(dyn, "polynomial_2", 16, True)
    seen = []
    smp.sample(b.B, b.frag, conditions=b.cond, h0=b.h0, noise_fn=b.noise, graph=graph, step_callback=seen.append)
    assert seen == list(range(1, 17))
    seen.clear()
    smp.sample(b.B, b.frag, conditions=b.cond, h0=b.h0, noise_fn=b.noise, graph=graph, step_callback=seen.append, timesteps=4)
    assert seen == [1, 2, 3, 4]


def _group_means(x, mask, n):
    s = torch.zeros(n, x.shape[1], dtype=torch.float64).index_add_(0, mask, x.double())
    return s / torch.bincount(mask, minlength=n).clamp(min=1).unsqueeze(1)


@pytest.mark.parametrize("graph", [False, None])
def test_on_nan_policies(graph, capsys):
    """One NaN in h0 (object TS, first reaction): every network call of the run predicts NaN for that reaction.  Plain NaN arithmetic."""
    dev = torch.device("cuda:0")
    dyn = _dynamics(dev)
    b = sc.batch()
    bad = [h.clone() for h in b.h0]
    bad[1][4, 2] = float("nan")
    message = "Warning: detected nan in pos, resetting EGNN output to randn."
    assert dyn.nan_check == "sync"

    def run(smp, h0):
        torch.manual_seed(41)
        out, _ = smp.sample(b.B, b.frag, conditions=b.cond, h0=h0, graph=graph)
        return [o[:, :POS].cpu() for o in out[0]]

    def clean_run(smp):
        capsys.readouterr()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            pos = run(smp, b.h0)
        assert not [w for w in caught if "NaN" in str(w.message)]
        assert all(bool(torch.isfinite(p).all()) for p in pos)
        assert message not in capsys.readouterr().out
        assert dyn.nan_check == "sync"

    smp = _sampler(dyn, "polynomial_2", 16, True, on_nan="raise")
    with pytest.raises(FloatingPointError):
        run(smp, bad)
    assert dyn.nan_check == "sync"
    clean_run(smp)

    smp = _sampler(dyn, "polynomial_2", 16, True, on_nan="warn")
    with pytest.warns(UserWarning, match="predicted NaN positions"):
        pos = run(smp, bad)
    assert not all(bool(torch.isfinite(p).all()) for p in pos)
    assert dyn.nan_check == "sync"
    clean_run(smp)

    smp = _sampler(dyn, "polynomial_2", 16, True, on_nan="replace")
    capsys.readouterr()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        pos = run(smp, bad)
    assert not [w for w in caught if "NaN" in str(w.message)]
    assert message in capsys.readouterr().out
    assert dyn.nan_check == "sync"
    for p, m in zip(pos, b.masks):
        assert bool(torch.isfinite(p).all())
        assert float(_group_means(p, m, b.B).abs().max()) <= 1e-6 * float(p.abs().max())
    clean_run(smp)


def test_sample_sharded_without_a_process_group_is_sample():
    import torch.distributed as dist
    assert not (dist.is_available() and dist.is_initialized())
    dev = torch.device("cuda:0")
    dyn = _dynamics(dev)
    b = sc.batch()
    smp = _sampler(dyn, "polynomial_2", 16, True)
    out, masks, span = smp.sample_sharded(b.frag, conditions=b.cond, seed=7, h0=b.h0)
    assert span == (0, b.B)
    sharded = [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]]
    torch.manual_seed(7)
    out, masks2 = smp.sample(b.B, b.frag, conditions=b.cond, h0=b.h0)
    assert _same(sharded, [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]])
    assert _same(masks, masks2)
    assert bool(all(torch.isfinite(x).all() for x in sharded))
