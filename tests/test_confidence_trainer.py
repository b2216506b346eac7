"""`ConfidenceTrainer` - the reference's `ConfModule` step (pl_trainer.py:421-669) - on cg_ragged_h32 (H = 32, B = 3 ragged, BCE)."""
import math

import numpy as np
import pytest
import torch

from _conf_grad_cases import ConfGradCase

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAME = "cg_ragged_h32"


def _trainer(g, state=None, **kw):
    from oareactdiff_amd import ConfidenceTrainer
    m = g.module(DEV, state=state)
    return m, ConfidenceTrainer(m, **kw)


def test_step_gradient_is_the_autograd_gradient_and_the_loss_is_compute_loss():
    """(a) The fused step (closed-form cotangent, sweep into the bucket) against `compute_loss(...)[0].backward()` on a second module."""
    g = ConfGradCase(NAME)
    batch = g.batch(DEV)
    m, tr = _trainer(g)
    info = tr.training_step(batch)
    m2, tr2 = _trainer(g)
    loss, logged = tr2.compute_loss(batch)
    assert loss.requires_grad
    tr2.flat_grad.zero_()
    loss.backward()                                                         # grad_inplace: lands in tr2's bucket
    top = float(tr2.flat_grad.abs().max())
    e = float((tr.flat_grad - tr2.flat_grad).abs().max()) / top
    print(f"bucket vs autograd path: {e:.2e} of the largest entry; loss {info['loss']:.8f} vs {float(loss.detach()):.8f}")
    assert top > 0 and e <= 1e-6, e
    assert abs(info["loss"] - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    assert abs(info["loss"] - g.loss64) <= 2e-5 * g.loss64
    assert info["skipped"] == 0 and set(logged) == {"acc", "precision", "F1", "mean"} <= set(info)
    assert all(abs(info[k] - logged[k]) <= 1e-6 for k in logged)
    # the parameter set: the reference's None tensors are outside the bucket
    assert not (set(tr.names) & g.none_names) and set(tr.names) == set(g.names)
    assert tr.n_params == sum(p.numel() for n, p in m.named_parameters() if n not in g.none_names) <= tr.flat_grad.numel()
    assert all(p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 for p in tr.params)


@pytest.mark.parametrize("amsgrad", [True, False])
def test_one_step_is_torch_adamw_on_that_gradient(amsgrad):
    """(b) float32 torch.optim.AdamW with the same configuration, applied to the step's gradient with the step's clip factor; the
    tensors outside the bucket keep their bits."""
    g = ConfGradCase(NAME)
    opt_cfg = dict(lr=5e-4, betas=(0.9, 0.999), weight_decay=0.01, amsgrad=amsgrad)
    m, tr = _trainer(g, optimizer_config=opt_cfg)
    tr.gradnorm_queue.items = [1e-3]                                        # forces clipping: max norm 2.5e-3
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    info = tr.training_step(g.batch(DEV))
    assert info["grad_norm"] > info["max_grad_norm"] == pytest.approx(2.5e-3)
    factor = info["max_grad_norm"] / (info["grad_norm"] + 1e-6)
    ref = [torch.nn.Parameter(before[n].clone()) for n in tr.names]
    for r, p in zip(ref, tr.params):
        r.grad = p.grad.detach().clone() * factor
    torch.optim.AdamW(ref, foreach=False, **opt_cfg).step()
    worst = max(float((p.detach() - r.detach()).abs().max()) for r, p in zip(ref, tr.params))
    print(f"amsgrad={amsgrad}: weights vs torch AdamW {worst:.2e}")
    assert worst <= 3e-6, worst
    moved = max(float((p.detach() - before[n]).abs().max()) for n, p in zip(tr.names, tr.params))
    assert moved > 1e-5
    for n, p in m.named_parameters():
        if n in g.none_names:
            assert torch.equal(p.detach(), before[n]) and p.grad is None, n


def test_clipping_history_follows_confmodule():
    """(c) max_grad_norm = 2.5 mean + 3 std of the history, which starts at [3000] (pl_trainer.py:465-468, 642-669)."""
    g = ConfGradCase(NAME)
    _, tr = _trainer(g)
    hist = [3000.0]
    for _ in range(3):
        info = tr.training_step(g.batch(DEV))
        want = 2.5 * float(np.mean(hist)) + 3 * float(np.std(hist))
        assert info["max_grad_norm"] == pytest.approx(want, rel=1e-12)
        hist.insert(0, min(info["grad_norm"], want))
        assert tr.gradnorm_queue.items == pytest.approx(hist, rel=1e-12)
    assert tr.opt_step == 3 and tr.skipped_steps == 0


def test_nan_input_skips_the_step():
    """(d) weights, moments, step count and clipping history bit-unchanged; the skip is counted."""
    g = ConfGradCase(NAME)
    m, tr = _trainer(g)
    tr.training_step(g.batch(DEV))
    snap = [t.clone() for t in (tr.flat_param, tr.exp_avg, tr.exp_avg_sq, tr.max_exp_avg_sq)]
    hist = list(tr.gradnorm_queue.items)
    reps, res = g.batch(DEV)
    reps[1]["pos"] = reps[1]["pos"].clone()
    reps[1]["pos"][0, 0] = float("nan")
    info = tr.training_step((reps, res))
    assert info["skipped"] == 1 and tr.skipped_steps == 1 and tr.opt_step == 1
    assert all(torch.equal(a, b) for a, b in zip(snap, (tr.flat_param, tr.exp_avg, tr.exp_avg_sq, tr.max_exp_avg_sq)))
    assert tr.gradnorm_queue.items == hist and math.isnan(info["max_grad_norm"])
    info = tr.training_step(g.batch(DEV))                                   # and training goes on
    assert info["skipped"] == 0 and tr.opt_step == 2 and math.isfinite(info["loss"])


def test_eight_steps_lower_the_loss():
    """(e) one fixed batch, BCE."""
    g = ConfGradCase(NAME)
    _, tr = _trainer(g)
    losses = [tr.training_step(g.batch(DEV))["loss"] for _ in range(8)]
    print("losses:", " ".join(f"{x:.5f}" for x in losses))
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]


@pytest.mark.parametrize("ema", [None, 0.9])
def test_state_dict_round_trip_reproduces_the_next_step(ema):
    """(f) module state + trainer state -> a new module and trainer: the next step gives the same bits."""
    g = ConfGradCase(NAME)
    batch = g.batch(DEV)
    m, tr = _trainer(g, ema_decay=ema)
    for _ in range(2):
        tr.training_step(batch)
    weights = {k: v.detach().clone() for k, v in m.state_dict().items()}
    state = tr.state_dict()
    m2, tr2 = _trainer(g, state=weights, ema_decay=ema)
    tr2.load_state_dict(state)
    a, b = tr.training_step(batch), tr2.training_step(batch)
    assert a == b
    for x, y in ((tr.flat_param, tr2.flat_param), (tr.exp_avg, tr2.exp_avg), (tr.exp_avg_sq, tr2.exp_avg_sq),
                 (tr.max_exp_avg_sq, tr2.max_exp_avg_sq)):
        assert torch.equal(x, y)
    if ema is not None:
        assert torch.equal(tr.flat_ema, tr2.flat_ema) and not torch.equal(tr.flat_ema, tr.flat_param)
    assert tr.gradnorm_queue.items == tr2.gradnorm_queue.items and tr2.opt_step == 3
