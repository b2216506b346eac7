"""`DDPMTrainer.eval_inpaint_batch` (the reference's eval_inplaint_batch, trainer/pl_trainer.py:284-325): inpaint the transition state with
reactant and product fixed, then the mean / median RMSD to the true one - on live and on EMA weights, leaving all training state alone.

The narrowest built width pair (32 x 8), one layer, ragged reactions of 4 / 7 / 5 (/ 3) atoms per object, 4 timesteps, 2 resamplings, jump
length 2, a deterministic noise_fn.  The reference numbers are the float64 SVD RMSDs (tests/_kabsch_cases.py) of the samples a separate
`DiffusionSampler.inpaint` call with the same noise returns: the two runs are bitwise equal, so the gate is the kernel's parity gate."""
import numpy as np
import pytest
import torch

import _kabsch_cases as kc

pytestmark = pytest.mark.gpu

CFG = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
NODE_NFS = [9, 9, 9]
KW = dict(timesteps=4, precision=0.05)
RUN = dict(resamplings=2, jump_length=2)


def _dev():
    return torch.device("cuda:0")


def _dynamics():
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import state_spec, synthetic_state_dict
    dyn = EGNNDynamics(model_config=dict(CFG), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0, condition_nf=1, device=_dev())
    dyn.load_state_dict(synthetic_state_dict(state_spec(CFG, NODE_NFS, 1), CFG, seed=42), strict=True)
    return dyn


def _batch(sizes):
    from oareactdiff_amd.trainer import DDPMTrainer
    g = torch.Generator().manual_seed(5)
    reps = []
    for _ in range(3):                                           # R, TS, P: the same atoms per reaction
        size = torch.tensor(sizes)
        n = int(size.sum())
        one_hot = torch.zeros(n, 5)
        one_hot[torch.arange(n), torch.randint(0, 5, (n,), generator=g)] = 1.0
        reps.append({"size": size, "pos": 1.5 * torch.randn(n, 3, generator=g), "one_hot": one_hot,
                     "charge": torch.randint(1, 9, (n, 1), generator=g).float(), "mask": torch.repeat_interleave(torch.arange(len(sizes)), size)})
    return DDPMTrainer.to_device((reps, torch.zeros(len(sizes), 1)), _dev(), non_blocking=False)


def _noise(sizes):
    n = sum(sizes)

    def fn(i):
        g = torch.Generator().manual_seed(1000 + i)
        return [torch.randn(n, nf, generator=g).clamp(-2.0, 2.0) for nf in NODE_NFS]
    return fn


def _reference(dyn, batch, sizes, T=4):
    """float64 RMSDs (reflection allowed) of the TS that a separate sampler draws from the same noise -> (r, rho, the samples)."""
    from oareactdiff_amd import DiffusionSampler
    reps, cond = batch
    xh = [torch.cat([r["pos"], r["one_hot"], r["charge"]], dim=1) for r in reps]
    smp = DiffusionSampler(dyn, "polynomial_2", T, 0.05)
    out, _ = smp.inpaint(len(sizes), [r["size_host"] for r in reps], conditions=cond, xh_fixed=xh, frag_fixed=[0, 2],
                         noise_fn=_noise(sizes), **RUN)
    r, rho = kc.reference(xh[1].cpu().numpy(), out[0][1].cpu().numpy(), sizes, True)
    return r, rho, out[0]


def _state(tr):
    dyn = tr.dynamics
    return {"params": [p.detach().clone() for p in tr.params], "flat_param": tr.flat_param.clone(), "ema": tr.flat_ema.clone(),
            "m": tr.exp_avg.clone(), "v": tr.exp_avg_sq.clone(), "vmax": tr.max_exp_avg_sq.clone(), "opt_step": tr.opt_step,
            "queue": list(tr.gradnorm_queue.items), "skipped": tr.skipped_steps, "training": dyn.training, "nan_check": dyn.nan_check}


def _same_state(a, b):
    for k in ("flat_param", "ema", "m", "v", "vmax"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a["params"], b["params"]))
    for k in ("opt_step", "queue", "skipped", "training", "nan_check"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("sizes", [[4, 7, 5], [4, 7, 5, 3]], ids=["odd_count", "even_count"])
def test_mean_and_median_are_numpys_over_the_reference_rmsds(sizes):
    from oareactdiff_amd.trainer import DDPMTrainer
    tr = DDPMTrainer(_dynamics(), ema_decay=0.5, **KW)
    tr.dynamics.train()
    batch = _batch(sizes)
    before = _state(tr)
    mean, median = tr.eval_inpaint_batch(batch, cap=None, noise_fn=_noise(sizes), **RUN)
    _same_state(before, _state(tr))
    assert tr.dynamics.training
    r, rho, _ = _reference(tr.dynamics, batch, sizes)
    got = tr.last_rmsds
    assert got.shape == (len(sizes),) and got.is_cuda
    for g in range(len(sizes)):
        print(f"n={sizes[g]}: kernel {float(got[g]):.9g} reference {r[g]:.9g}")
        assert abs(float(got[g]) - r[g]) <= kc.gate(r[g], rho[g])
    lim = max(kc.gate(r[g], rho[g]) for g in range(len(sizes)))   # mean and median are averages of entries that each meet their gate
    print(f"mean {mean:.9g} / {np.mean(r):.9g}, median {median:.9g} / {np.median(r):.9g}")
    assert isinstance(mean, float) and isinstance(median, float)
    assert abs(mean - np.mean(r)) <= lim and abs(median - np.median(r)) <= lim
    if len(sizes) % 2 == 0:
        s = np.sort(r)
        assert s[1] != s[2] and abs(median - s[1]) > lim and abs(median - s[2]) > lim     # neither middle value alone (torch.median's answer)
    # the capped call: every entry <= 1, and the same sampler object serves it
    n_samplers = len(tr._eval_samplers)
    m1, _ = tr.eval_inpaint_batch(batch, noise_fn=_noise(sizes), **RUN)
    assert len(tr._eval_samplers) == n_samplers == 1
    assert bool((tr.last_rmsds <= 1.0).all()) and torch.equal(tr.last_rmsds, got.clamp(max=1.0)) and m1 <= 1.0
    _same_state(before, _state(tr))


def test_ema_weights_go_through_the_shadow_module():
    from oareactdiff_amd.trainer import DDPMTrainer
    sizes = [4, 7, 5]
    tr = DDPMTrainer(_dynamics(), ema_decay=0.5, timesteps=1000, precision=0.05, optimizer_config=dict(lr=1e-2))
    batch = _batch(sizes)
    g = torch.Generator().manual_seed(100)
    info = tr.training_step(batch, t_int=torch.tensor([0.0, 500.0, 900.0], device=_dev()).view(-1, 1),
                            draw=lambda shape: torch.randn(shape, generator=g).clamp(-2.0, 2.0).to(_dev()))
    assert info["skipped"] == 0 and not torch.equal(tr.flat_ema, tr.flat_param)
    before = _state(tr)
    live = tr.eval_inpaint_batch(batch, cap=None, timesteps=4, noise_fn=_noise(sizes), **RUN)
    r_live = tr.last_rmsds.clone()
    ema = tr.eval_inpaint_batch(batch, cap=None, timesteps=4, weights="ema", noise_fn=_noise(sizes), **RUN)
    r_ema = tr.last_rmsds.clone()
    _same_state(before, _state(tr))
    assert set(tr._eval_samplers) == {("polynomial_2", 4, "live"), ("polynomial_2", 4, "ema")}
    assert tr._eval_samplers[("polynomial_2", 4, "ema")].dynamics is tr.ema_dynamics
    assert tr.ema_dynamics.nan_check == tr.dynamics.nan_check
    # the run through trainer.ema_dynamics by hand
    r, rho, _ = _reference(tr.ema_dynamics, batch, sizes)
    for g_ in range(len(sizes)):
        assert abs(float(r_ema[g_]) - r[g_]) <= kc.gate(r[g_], rho[g_])
    lim = max(kc.gate(r[g_], rho[g_]) for g_ in range(len(sizes)))
    assert abs(ema[0] - np.mean(r)) <= lim and abs(ema[1] - np.median(r)) <= lim
    assert not torch.equal(r_ema, r_live) and ema != live
    with pytest.raises(ValueError):
        tr.eval_inpaint_batch(batch, weights="best")
