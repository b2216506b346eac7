"""`DiffusionSampler.inpaint` on the fused RePaint step: the ragged batch, weights and float64 replay of tests/_sampler_cases.py
(T = 12, 2 resamplings, jump length 3, R and P fixed, Gaussian-prior term), the bars of tests/test_sampler_loops.py; the earlier launch
sequence (`fused=False`) beside it; the hipGraph replay of the loop, bit for bit the eager loop; `inpaint_sharded` on one device."""
import functools

import pytest
import torch

import _sampler_cases as sc
from _cases import rel

pytestmark = pytest.mark.gpu
TOL = 1e-5            # one network call on identical inputs (the project's bar)
TRAJ = 5e-5           # a whole trajectory against its float64 replay
POS = sc.POS
KW = dict(resamplings=2, jump_length=3)


@functools.lru_cache(maxsize=None)
def _dynamics():
    from oareactdiff_amd import EGNNDynamics
    dyn = EGNNDynamics(model_config=dict(sc.CFG), fragment_names=["R", "TS", "P"], node_nfs=sc.NODE_NFS, edge_nf=0, condition_nf=1,
                       device=torch.device("cuda:0"))
    dyn.load_state_dict(sc.weights(), strict=True)
    return dyn


def _sampler(T=12, **kw):
    from oareactdiff_amd import DiffusionSampler
    return DiffusionSampler(_dynamics(), "polynomial_2", T, sc.PRECISION, pos_only=True, gaussian_prior_std=1.0, **kw)


def _flat(xs, sl):
    return torch.cat([torch.as_tensor(x)[:, sl].detach().cpu().double().reshape(-1) for x in xs])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _run(smp, b, seed=None, frag_fixed=(0, 2), **kw):
    """One inpainting run -> final state and returned samples (clones); with `seed` on the device generator, else on `b.noise`."""
    if seed is not None:
        torch.manual_seed(seed)
    out, masks = smp.inpaint(b.B, b.frag, conditions=b.cond, xh_fixed=b.xh_fixed, frag_fixed=list(frag_fixed),
                             noise_fn=None if seed is not None else b.noise, **dict(KW, **kw))
    assert int(smp.last_status[0].item()) == 0
    assert len(out) == 1 and all(torch.equal(m.cpu(), mm) for m, mm in zip(masks, b.masks))
    return [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]]


def _group_means(p, mask, n):
    s = torch.zeros(n, p.shape[1], dtype=torch.float64).index_add_(0, mask, p.double())
    return s / torch.bincount(mask, minlength=n).clamp(min=1).unsqueeze(1)


def test_fused_loop_tracks_the_f64_replay_and_the_unfused_loop():
    """The bars of tests/test_sampler_loops.py's inpaint test on the fused loop, then `fused=False` on the same draws.  The float64
    replay (about 35 s of CPU, cached per process in tests/_sampler_cases.py) is the one that test uses: whichever runs first pays.
    Measured on an MI355X: fused against the replay 2.29e-07, fused=False against the fused loop 1.31e-07."""
    dev = torch.device("cuda:0")
    b = sc.batch()
    r = sc.replay("inpaint", "polynomial_2", 12, 12, True)
    assert len(r.calls) == 22
    assert r.min_active == b.inner, "the replay's trajectory left the cutoff"
    dyn = _dynamics()
    smp = _sampler()
    given = [x.clone() for x in b.xh_fixed]
    fused = _run(smp, b, graph=False)
    assert smp.last_inpaint_loop == "fused"
    assert _same(given, b.xh_fixed), "inpaint modified the caller's xh_fixed"
    # the device's own final state inside the cutoff (a loop that dropped the prior term ends at |pos| ~ 470 A)
    worst = 0.0
    for x, m in zip(fused[:3], b.masks):
        p = x[:, :POS].cpu().double()
        d = torch.cdist(p, p)
        assert bool(torch.isfinite(d).all())
        worst = max(worst, float(d[m[:, None] == m[None, :]].max()))
    assert worst < sc.CFG["cutoff"], f"device trajectory left the cutoff: same-object pair at {worst:.1f} A"
    ep = rel(_flat(fused[:3], slice(0, POS)), _flat(r.x64, slice(0, POS)))
    vel, feat = [], []
    ei, cond, nfs, cm = b.ei.to(dev), b.cond.to(dev), b.nfs.to(dev), b.cm.to(dev)
    for z32, t32, o, _ in r.calls:
        with torch.no_grad():
            out, _ = dyn([z.to(dev) for z in z32], ei, t32.to(dev), cond, nfs, cm)
        vel.append(rel(_flat(out, slice(0, POS)), _flat(o, slice(0, POS))))
        feat.append(rel(_flat(out, slice(POS, None)), _flat(o, slice(POS, None))))
    print(f"fused inpaint: final positions {ep:.2e} against the replay; per call velocity worst {max(vel):.2e}, features worst {max(feat):.2e}; "
          f"largest same-object pair distance {worst:.2f} A")
    assert ep <= TRAJ
    assert max(vel) <= TOL and max(feat) <= TOL
    for k in range(3):                                       # pos_only: the returned features are those of xh_fixed
        assert torch.equal(fused[3 + k][:, POS:].cpu().float(), b.h0[k])
    # the earlier launch sequence on the same draws
    unfused = _run(smp, b, fused=False)
    assert smp.last_inpaint_loop == "unfused"
    eu = rel(_flat(unfused[:3], slice(0, POS)), _flat(fused[:3], slice(0, POS)))
    print(f"fused=False against the fused loop, final positions: {eu:.2e}; against the replay: "
          f"{rel(_flat(unfused[:3], slice(0, POS)), _flat(r.x64, slice(0, POS))):.2e}")
    assert eu <= TRAJ
    for k in range(3):
        assert torch.equal(unfused[3 + k][:, POS:], fused[3 + k][:, POS:])
    with pytest.raises(AssertionError):
        _run(smp, b, fused=False, graph=True)


@pytest.mark.parametrize("frag_fixed", [(), (0, 1, 2)])
@pytest.mark.parametrize("graph", [False, True])
def test_nothing_fixed_and_everything_fixed(frag_fixed, graph):
    """Finite and CoM-free.  The final x | z0 step is not projected: it adds three CoM-free terms (state, prediction, noise), each
    freed of its mean by a float32 sum over n <= 30 rows, which leaves at most n 2^-24 max|term| each: 3 x 30 x 2^-24 = 5.4e-6 < 1e-5."""
    b = sc.batch()
    smp = _sampler()
    got = _run(smp, b, frag_fixed=frag_fixed, graph=graph)
    for x, m in zip(got[3:], b.masks):
        p = x[:, :POS].cpu()
        assert bool(torch.isfinite(x).all())
        gm, top = float(_group_means(p, m, b.B).abs().max()), float(p.abs().max())
        print(f"frag_fixed {frag_fixed} graph {graph}: largest group mean {gm:.2e}, max |pos| {top:.2e}")
        assert gm <= 1e-5 * top


def test_graphed_loop_is_bitwise_the_eager_loop():
    b = sc.batch()
    smp = _sampler()
    eager = _run(smp, b, graph=False)
    assert smp.last_inpaint_loop == "fused"
    assert _same(eager, _run(smp, b, graph=True)) and smp.last_inpaint_loop == "graphed"
    assert smp.last_inpaint_refills == 1
    eager_rng = _run(smp, b, seed=31, graph=False)
    assert _same(eager_rng, _run(smp, b, seed=31, graph=True))
    assert not _same(eager_rng[:3], eager[:3])
    # one step: the graph is never captured (the warm-up step is the whole loop)
    assert _same(_run(smp, b, graph=False, timesteps=1), _run(smp, b, graph=True, timesteps=1))
    assert _same(_run(smp, b, seed=32, graph=False, timesteps=1), _run(smp, b, seed=32, graph=True, timesteps=1))
    # room for 6 steps of noise per block: the 21 steps take 4 fills, and the jump steps (entries 5, 11, 17) are the last rows of
    # their blocks - the next draw after a jump row belongs to the next block
    from oareactdiff_amd.schedule import repaint_steps
    assert [i for i, (_, j) in enumerate(repaint_steps(2, 3, 12)) if j is not None] == [5, 11, 17]
    old = smp.noise_block_bytes
    smp.noise_block_bytes = 6 * 3 * 4 * sum(n * 9 for n in b.sizes)
    try:
        assert _same(eager_rng, _run(smp, b, seed=31, graph=True)) and smp.last_inpaint_refills == 4
        assert _same(eager, _run(smp, b, graph=True)) and smp.last_inpaint_refills == 4
    finally:
        smp.noise_block_bytes = old


def test_automatic_choice_of_the_loop():
    """graph=None is the fused eager loop, on the 5-reaction batch and on a 9-reaction one alike: the hipGraph replay of this loop
    measured slower than the eager loop at every batch size (profiles/inpaint_loop.txt), so - other than in `sample`, whose rule would
    have picked it for the 5 reactions - it runs only where it is asked for.  Seen through `last_inpaint_loop`, not through timing."""
    b = sc.batch()
    smp = _sampler()
    eager = _run(smp, b, graph=False)
    assert _same(eager, _run(smp, b)) and smp.last_inpaint_loop == "fused"
    assert _same(eager, _run(smp, b, graph=True)) and smp.last_inpaint_loop == "graphed"
    _run(smp, b, fused=False)
    assert smp.last_inpaint_loop == "unfused"
    b9 = sc.Batch(tuple(f[:9] for f in sc.FRAGS_12))
    assert b9.B == 9
    got = _run(smp, b9, seed=35)
    assert smp.last_inpaint_loop == "fused"
    assert _same(got, _run(smp, b9, seed=35, graph=True)) and smp.last_inpaint_loop == "graphed"
    assert bool(all(torch.isfinite(x).all() for x in got))


def test_inpaint_sharded_without_a_process_group_is_inpaint():
    import torch.distributed as dist
    assert not (dist.is_available() and dist.is_initialized())
    b = sc.batch()
    smp = _sampler()
    out, masks, span = smp.inpaint_sharded(b.frag, b.xh_fixed, conditions=b.cond, seed=7, frag_fixed=[0, 2], **KW)
    assert span == (0, b.B)
    sharded = [x.clone() for x in smp.last_x] + [o.clone() for o in out[0]]
    assert _same(sharded, _run(smp, b, seed=7))
    assert all(torch.equal(m.cpu(), mm) for m, mm in zip(masks, b.masks))
    assert bool(all(torch.isfinite(x).all() for x in sharded))
