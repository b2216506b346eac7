"""DDPMTrainer(ema_decay=...) on the fused step: the exponential moving average of the weights folded into the AdamW kernel
(oard_adamw_step_ema / oard_adamw_step_dev_ema) and the shadow module `ema_dynamics` whose parameters are views into the average.

The average is pinned as ModelEmaV2.update in float32 (trainer/ema.py:37-47):  ema = fl(fl(d32 ema) + fl(w32 p_new)); it never feeds
back into training.  Every gate here is therefore bit equality: weights, moments and clipping history to a twin trainer without the
average; the average to the recursion applied on the host to the twin's weights; the shadow module to a fresh module that loaded
`ema_state_dict()` (same kernels, same packed weights, same inputs).

The narrowest built width pair (32 x 8), one layer, two reactions of ragged small objects (one object is a single atom), time steps
and draws injected."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
NODE_NFS = [9, 9, 9]
FRAGS = [[1, 5], [3, 4], [2, 6]]              # atoms of R, TS, P in the two reactions
T = 1000
T_INT = [0.0, 500.0]
DECAY = 0.9
KW = dict(timesteps=T, precision=0.05, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0))


def _dev():
    return torch.device("cuda:0")


def _dynamics(state=None):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import state_spec, synthetic_state_dict
    dyn = EGNNDynamics(model_config=dict(CFG), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0, condition_nf=1, device=_dev())
    dyn.load_state_dict(synthetic_state_dict(state_spec(CFG, NODE_NFS, 1), CFG, seed=42) if state is None else state, strict=True)
    return dyn


def _trainer(fused=True, **kw):
    from oareactdiff_amd.trainer import DDPMTrainer
    return DDPMTrainer(_dynamics(), fused=fused, **dict(KW, **kw))


def _reps(poison=False):
    g = torch.Generator().manual_seed(5)
    reps = []
    for f in FRAGS:
        size = torch.tensor(f)
        mask = torch.repeat_interleave(torch.arange(len(f)), size)
        n = int(size.sum())
        one_hot = torch.zeros(n, 5)
        one_hot[torch.arange(n), torch.randint(0, 5, (n,), generator=g)] = 1.0
        reps.append({"size": size, "pos": 2.0 * torch.randn(n, 3, generator=g), "one_hot": one_hot,
                     "charge": torch.randint(1, 9, (n, 1), generator=g).float(), "mask": mask})
    if poison:
        reps[0]["pos"][0, 0] = float("inf")
    return reps


def _batch(poison=False, host_copies=True):
    from oareactdiff_amd.trainer import DDPMTrainer
    batch = (_reps(poison), torch.zeros(len(T_INT), 1))
    if host_copies:
        return DDPMTrainer.to_device(batch, _dev(), non_blocking=False)
    return [{k: v.to(_dev()) for k, v in r.items()} for r in batch[0]], batch[1].to(_dev())


def _step(tr, k, poison=False):
    """Step k of a run: the same time steps, its own recorded draws (clamped: keeps the t = 0 terms away from cdf differences of 0)."""
    g = torch.Generator().manual_seed(100 + k)
    t_int = torch.tensor(T_INT, device=_dev()).view(-1, 1)
    return tr.training_step(_batch(poison), t_int=t_int, draw=lambda shape: torch.randn(shape, generator=g).clamp(-2.0, 2.0).to(_dev()))


def _recursion(e, p, decay=DECAY):
    d32, w32 = np.float32(decay), np.float32(1.0 - decay)
    return d32 * e + w32 * p                    # float32 arrays: two rounded products, one rounded sum


def _run(steps=3, **kw):
    tr = _trainer(**kw)
    weights = []
    for k in range(steps):
        info = _step(tr, k)
        assert info["skipped"] == 0
        weights.append(tr.flat_param.cpu().numpy().copy())
    return tr, weights


@pytest.fixture(scope="module")
def runs():
    """Three fused steps: the twin without an average, and the average with the host-side and the device-side step decision."""
    w0 = _trainer().flat_param.cpu().numpy().copy()
    return {"w0": w0, "twin": _run(), "sync": _run(ema_decay=DECAY), "async": _run(ema_decay=DECAY, host_sync=False)}


def test_average_follows_the_recursion_and_never_feeds_back(runs):
    (twin, w_twin), (a, w_a), (b, w_b) = runs["twin"], runs["sync"], runs["async"]
    assert twin.flat_ema is None and a.flat_ema.shape == a.flat_param.shape and a.flat_ema.dtype == torch.float32
    sd_twin = twin.state_dict()
    for tr, w in ((a, w_a), (b, w_b)):
        for k in range(3):
            assert np.array_equal(w[k], w_twin[k]), k
        sd = tr.state_dict()
        assert sd["gradnorm_queue"] == sd_twin["gradnorm_queue"] and sd["opt_step"] == sd_twin["opt_step"] == 3
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(sd[key], sd_twin[key]), key
        assert set(sd) == set(sd_twin) | {"ema", "ema_decay"}
    want = runs["w0"]
    for k in range(3):
        want = _recursion(want, w_twin[k])
    assert want.dtype == np.float32 and not np.array_equal(want, w_twin[2])
    assert np.array_equal(a.flat_ema.cpu().numpy(), want)
    assert torch.equal(a.flat_ema, b.flat_ema) and torch.equal(a.flat_param, b.flat_param)


def _flat(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.params]).cpu().numpy()


def test_two_microbatches_and_the_generic_step_update_the_same_average():
    """`microbatches=2` takes the same `_ema` entry point (its weights differ from the one-batch step's in the order of one addition,
    so the recursion is applied to ITS weights).  The generic trainer (autograd + torch.optim.AdamW) on the device calls oard_ema_update
    per tensor on views of the flat average; where the weights are one flat buffer as well, it is one call."""
    for kw in (dict(microbatches=2, host_sync=False), dict(fused=False)):
        tr = _trainer(ema_decay=DECAY, **kw)
        want = _flat(tr).copy()
        assert np.array_equal(tr.flat_ema.cpu().numpy(), want)
        for k in range(2):
            g = torch.Generator().manual_seed(100 + k)
            t_int = torch.tensor(T_INT, device=_dev()).view(-1, 1)
            info = tr.training_step(_batch(host_copies=tr.fused), t_int=t_int,
                                    draw=lambda shape: torch.randn(shape, generator=g).clamp(-2.0, 2.0).to(_dev()))
            assert info["skipped"] == 0
            want = _recursion(want, _flat(tr))
            assert np.array_equal(tr.flat_ema.cpu().numpy(), want), (kw, k)
        assert (tr._mb is not None) == (kw.get("microbatches") == 2) and tr.fused == ("fused" not in kw)
    with torch.no_grad():
        tr = _trainer(ema_decay=DECAY)
        tr.flat_param.mul_(1.5)
        want = _recursion(tr.flat_ema.cpu().numpy(), tr.flat_param.cpu().numpy())
        tr._ema_step_generic()
        assert np.array_equal(tr.flat_ema.cpu().numpy(), want)


@pytest.mark.parametrize("host_sync", [True, False])
def test_skipped_step_leaves_the_average_untouched(host_sync):
    tr = _trainer(ema_decay=DECAY, host_sync=host_sync)
    assert _step(tr, 0)["skipped"] == 0
    before, w_before = tr.flat_ema.clone(), tr.flat_param.clone()
    assert not torch.equal(before, w_before)
    info = _step(tr, 1, poison=True)                 # inf in a position: non-finite loss, the step is skipped
    assert info["skipped"] == 1
    assert torch.equal(tr.flat_ema, before) and torch.equal(tr.flat_param, w_before)
    assert _step(tr, 2)["skipped"] == 0 and not torch.equal(tr.flat_ema, before)


def test_resume_continues_the_average_bit_for_bit():
    a, _ = _run(steps=2, ema_decay=DECAY)
    msd = {k: v.clone() for k, v in a.dynamics.state_dict().items()}
    tsd = a.state_dict()
    assert tsd["ema_decay"] == DECAY and torch.equal(tsd["ema"], a.flat_ema) and tsd["ema"].data_ptr() != a.flat_ema.data_ptr()
    _step(a, 2)                                      # the uninterrupted run
    b = _trainer(ema_decay=DECAY)
    b.dynamics.load_state_dict(msd, strict=True)
    b.load_state_dict(tsd)
    assert torch.equal(b.flat_ema, tsd["ema"]) and b.ema_decay == DECAY
    _step(b, 2)
    assert torch.equal(b.flat_ema, a.flat_ema) and torch.equal(b.flat_param, a.flat_param)
    assert not torch.equal(b.flat_ema, tsd["ema"])
    # a state without an average: one warning, and the average restarts from the weights
    c = _trainer(ema_decay=DECAY)
    c.dynamics.load_state_dict(msd, strict=True)
    with pytest.warns(UserWarning, match="EMA"):
        c.load_state_dict({k: v for k, v in tsd.items() if k not in ("ema", "ema_decay")})
    assert torch.equal(c.flat_ema, c.flat_param)
    # ... and a state with one into a trainer that keeps none is taken without it
    d = _trainer()
    d.dynamics.load_state_dict(msd, strict=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d.load_state_dict(tsd)
    assert d.flat_ema is None and "ema" not in d.state_dict()


def _forward_inputs(tr):
    """A fixed network input on the batch's layout."""
    reps = _reps()
    cm, ei, nfs = tr.loss._layout([r["mask"] for r in reps], [r["size"] for r in reps])
    g = torch.Generator().manual_seed(9)
    xh = [torch.randn(int(r["mask"].numel()), 9, generator=g).to(_dev()) for r in reps]
    t = torch.tensor([[0.3], [0.8]], device=_dev())
    return xh, ei.to(_dev()), t, torch.zeros(2, 1, device=_dev()), nfs.to(_dev()), cm.to(_dev())


def _forward(dyn, inputs):
    with torch.no_grad():
        out, _ = dyn(*inputs)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_shadow_module_is_the_average_without_a_copy():
    tr, _ = _run(steps=2, ema_decay=DECAY)
    inputs = _forward_inputs(tr)
    live_before = _forward(tr.dynamics, inputs)
    assert tr._ema_dynamics is None                  # built at the first look ...
    shadow = tr.ema_dynamics
    assert tr.ema_dynamics is shadow and shadow._ws is None and not shadow._packs        # ... and nothing allocated before its first call
    fresh = _dynamics(tr.ema_state_dict())           # strict=True inside
    got = _forward(shadow, inputs)
    assert _same(got, _forward(fresh, inputs)) and all(bool(torch.isfinite(o).all()) for o in got)
    assert not _same(got, live_before)
    assert _same(_forward(tr.dynamics, inputs), live_before), "calling the shadow moved the live module's output"
    # every trainable tensor of the shadow lies inside flat_ema; the others share the live module's storage; nothing wants a gradient
    lo, hi = tr.flat_ema.data_ptr(), tr.flat_ema.data_ptr() + 4 * tr.flat_ema.numel()
    named, live = dict(shadow.named_parameters()), dict(tr.dynamics.named_parameters())
    assert set(named) == set(live) and list(shadow.state_dict()) == list(tr.dynamics.state_dict())
    for name, p in named.items():
        assert not p.requires_grad
        if name in tr.names:
            assert lo <= p.data_ptr() and p.data_ptr() + 4 * p.numel() <= hi, name
        else:
            assert p.data_ptr() == live[name].data_ptr(), name
    assert all(b.data_ptr() == dict(tr.dynamics.named_buffers())[n].data_ptr() for n, b in shadow.named_buffers())
    assert shadow.nan_check == tr.dynamics.nan_check and shadow.edge_precision == tr.dynamics.edge_precision
    # one more step: the average moved behind the shadow's packed weights; its next call repacks
    _step(tr, 2)
    after = _forward(shadow, inputs)
    assert not _same(after, got)
    assert _same(after, _forward(_dynamics(tr.ema_state_dict()), inputs))
    # the loss under the averaged weights, without store / copy / restore
    from oareactdiff_amd.loss import DiffusionLoss
    fresh = _dynamics(tr.ema_state_dict())
    ref_loss = DiffusionLoss(fresh, "polynomial_2", T, KW["precision"], norm_values=KW["norm_values"], scales=KW["scales"])

    def draws():
        g = torch.Generator().manual_seed(31)
        return lambda shape: torch.randn(shape, generator=g).clamp(-2.0, 2.0).to(_dev())
    t_int = torch.tensor(T_INT, device=_dev()).view(-1, 1)
    batch = _batch(host_copies=False)
    with torch.no_grad():
        nll_ref, info_ref = ref_loss.compute_loss(batch[0], batch[1], training=False, t_int=t_int, draw=draws())
    w_live = tr.flat_param.clone()
    nll, info = tr.compute_loss(batch, training=False, weights="ema", t_int=t_int, draw=draws())
    assert torch.equal(nll, nll_ref) and info == info_ref and bool(torch.isfinite(nll).all())
    assert tr.loss.dynamics is tr.dynamics and torch.equal(tr.flat_param, w_live)
    nll_live, _ = tr.compute_loss(batch, training=False, t_int=t_int, draw=draws())
    assert not torch.equal(nll_live.detach(), nll)
    # on_train_end: the average becomes the model
    tr.copy_ema_to_model()
    assert torch.equal(tr.flat_param, tr.flat_ema)
    assert _same(_forward(tr.dynamics, inputs), _forward(shadow, inputs))
    with pytest.raises(RuntimeError):
        _trainer().ema_dynamics


def test_sampler_on_the_shadow_module_equals_a_fresh_load():
    from oareactdiff_amd import DiffusionSampler
    tr, _ = _run(steps=2, ema_decay=DECAY)
    steps = 4
    frag = [torch.tensor(f) for f in FRAGS]
    counts = [sum(f) for f in FRAGS]
    noise = {}

    def noise_fn(i):
        if i not in noise:
            g = torch.Generator().manual_seed(700 + i)
            noise[i] = [torch.randn(n, 9, generator=g) for n in counts]
        return noise[i]
    res = []
    for dyn in (tr.ema_dynamics, _dynamics(tr.ema_state_dict()), tr.dynamics):
        smp = DiffusionSampler(dyn, "polynomial_2", steps, 1e-5, norm_values=KW["norm_values"], gaussian_prior_std=1.0)
        out, _ = smp.sample(2, frag, conditions=torch.zeros(2, 1), noise_fn=noise_fn)
        torch.cuda.synchronize()
        res.append([o.clone() for o in out[0]])
    assert _same(res[0], res[1]) and all(bool(torch.isfinite(o).all()) for o in res[0])
    assert not _same(res[0], res[2])                 # (the live weights give another sample)
