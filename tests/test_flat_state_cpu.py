"""`oareactdiff_amd.flat_state`: the layout both trainers give their flat buffers, the host side of the adaptive clipping rule, and the
key sets of the trainers' `state_dict()` (generic trainer on the CPU; fused trainer and confidence trainer on the device)."""
import numpy as np
import pytest
import torch

from oareactdiff_amd.flat_state import FlatLayout, Queue, clip_decision

SHAPES = [(), (3,), (2, 2), (5,), (2, 4)]
# the two packing rules in use: back to back (DDPMTrainer), and every start on a multiple of four floats with the total padded too
# (ConfidenceTrainer: n = (n + numel + 3) // 4 * 4 after every tensor)
EXPECTED = {1: ([0, 1, 4, 8, 13], 21), 4: ([0, 4, 8, 12, 20], 28)}
SHARED = {"names", "skipped_steps", "gradnorm_queue"}
FLAT = {"opt_step", "param_groups", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
EMA = {"ema_decay", "ema"}


@pytest.mark.parametrize("align", [1, 4])
def test_layout_offsets_and_views(align):
    tensors = [torch.randn(s) for s in SHAPES]
    lay = FlatLayout(tensors, align)
    starts, size = EXPECTED[align]
    assert lay.starts == starts and lay.size == size
    assert lay.offsets() == {id(t): o for t, o in zip(tensors, starts)}
    flat = torch.zeros(size)
    views = lay.views(flat)
    dests = lay.dests(flat)
    assert list(dests) == [id(t) for t in tensors]
    for t, v, o in zip(tensors, views, starts):
        assert v.shape == t.shape and v.data_ptr() == flat.data_ptr() + 4 * o == dests[id(t)].data_ptr()
        assert dests[id(t)].shape == t.shape
        v.fill_(1.0)
    covered = torch.zeros(size, dtype=torch.bool)
    for t, o in zip(tensors, starts):
        covered[o: o + t.numel()] = True
    assert int(covered.sum()) == sum(t.numel() for t in tensors) == 21
    assert torch.equal(flat, covered.float())                          # every element of every tensor, and the gaps still zero


@pytest.mark.parametrize("a,b", [(1.5, 3.0), (2.5, 3.0)])
def test_clip_decision(a, b, capsys):
    q = Queue()
    q.add(3000)
    gscale, allowed = clip_decision(q, 10.0, a, b)
    assert gscale == 1 and allowed == a * 3000.0 and q.items == [10.0, 3000]
    assert capsys.readouterr().out == ""
    hist = [10.0, 3000.0]
    want = a * float(np.mean(hist)) + b * float(np.std(hist))
    norm = 2.0 * want
    gscale, allowed = clip_decision(q, norm, a, b)
    assert allowed == want and gscale == want / (norm + 1e-6) and q.items == [want, 10.0, 3000]
    assert capsys.readouterr().out == f"Clipped gradient with value {norm:.1f} while allowed {want:.1f}\n"
    # a non-finite norm is neither clipped nor remembered
    for bad in (float("nan"), float("inf")):
        gscale, _ = clip_decision(q, bad, a, b)
        assert gscale == 1 and q.items == [want, 10.0, 3000]


@pytest.mark.parametrize("ema", [None, 0.9])
def test_state_keys_of_the_generic_trainer(ema):
    from test_trainer_ema_cpu import _trainer
    tr = _trainer(ema_decay=ema)
    assert not tr.fused and not hasattr(tr, "flat_param") and tr.flat_grad.numel() == sum(p.numel() for p in tr.params)
    assert set(tr.state_dict()) == SHARED | {"fused", "optimizer"} | (EMA if ema else set())


@pytest.mark.gpu
@pytest.mark.parametrize("ema", [None, 0.9])
def test_state_keys_of_the_fused_trainer(ema):
    from _grad_cases import GradCase
    from test_trainer_fused import _trainer
    tr = _trainer(GradCase("g9_grad_h32"), torch.device("cuda:0"), True, True, ema_decay=ema)
    assert tr.fused and tr.flat_param.numel() == tr.flat_grad.numel() == tr.layout.size == sum(p.numel() for p in tr.params)
    assert set(tr.state_dict()) == SHARED | FLAT | {"fused"} | (EMA if ema else set())


@pytest.mark.gpu
@pytest.mark.parametrize("ema", [None, 0.9])
def test_state_keys_of_the_confidence_trainer(ema):
    from _conf_grad_cases import ConfGradCase
    from test_confidence_trainer import NAME, _trainer
    _, tr = _trainer(ConfGradCase(NAME), ema_decay=ema)
    assert tr.flat_param.numel() == tr.flat_grad.numel() == tr.layout.size >= tr.n_params
    assert set(tr.state_dict()) == SHARED | FLAT | (EMA if ema else set())
