"""k_ema_update (behind oard_ema_update) and the EMA instantiations of k_adamw (oard_adamw_step_ema, oard_adamw_step_dev_ema) on their own.

The average's semantics are pinned as `ModelEmaV2.update` in float32 (trainer/ema.py:37-47):
    ema = fl(fl(d32 * ema) + fl(w32 * p)),   d32 = float32(decay), w32 = float32(1.0 - decay)
two rounded products and one add.  The gate is therefore BIT EQUALITY - to torch's evaluation of `d32 * e + w32 * p` on the device
and to numpy's in float32 on the host - not a tolerance.  The two fused kernels must leave parameters and moments bit-identical to
the plain entry points on the same inputs (the average never feeds back) and the average equal to the expression applied to the plain
entry point's parameters.  Every array carries a guard element behind it (the pattern of tests/test_optimizer_kernels.py)."""
import numpy as np
import pytest
import torch

from test_optimizer_kernels import HYPER, Bucket, _lib, dev_step, history, host_rule, host_step, make_state

pytestmark = pytest.mark.gpu

NS = [1, 255, 256, 257, 513]                   # around the 256-thread block
DECAYS = [0.0, 0.5, 0.999, 1.0]
GUARD = 11.0


def scalars(decay):
    return np.float32(decay), np.float32(1.0 - decay)


def special_values(n, seed):
    """n values ~ N(0, 1) with exact zeros, denormals and +-large values among them, plus the guard element."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    specials = torch.tensor([0.0, -0.0, 1e-40, -3e-42, 3e38, -2.5e38, 1.1754944e-38, 7e-46])
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))[:min(n, specials.numel())]
    x[idx] = specials[:idx.numel()]
    return torch.cat([x, torch.tensor([GUARD])])


def host_ema(e, p, decay):
    """The expression in numpy float32 (every intermediate is a float32 array: two rounded products, one rounded sum)."""
    d32, w32 = scalars(decay)
    with np.errstate(all="ignore"):
        return torch.from_numpy(d32 * e.cpu().numpy() + w32 * p.cpu().numpy())


def dev_ema(e, p, decay):
    """... and by torch on the device: two tensor-by-scalar products, one sum."""
    d32, w32 = scalars(decay)
    return e * float(d32) + p * float(w32)


def ema_update(e, p, n, decay):
    capi, L = _lib()
    stream = torch.cuda.current_stream(e.device).cuda_stream
    with torch.cuda.device(e.device):
        rc = L.oard_ema_update(None if e is None else e.data_ptr(), p.data_ptr(), n, decay, stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", NS)
def test_ema_update_is_the_float32_expression_bit_for_bit(n, decay):
    capi, L = _lib()
    dev = torch.device("cuda:0")
    e0, p0 = special_values(n, 10 * n).to(dev), special_values(n, 10 * n + 5).to(dev)
    e, p = e0.clone(), p0.clone()
    assert ema_update(e, p, n, decay) == capi.OARD_OK
    want_dev, want_host = dev_ema(e0[:n], p0[:n], decay), host_ema(e0[:n], p0[:n], decay)
    # bit patterns: torch.equal would call -0.0 and 0.0 equal and NaN unequal to itself
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)         # noqa: E731
    assert torch.equal(bits(want_dev), bits(want_host)), "torch on the device and numpy on the host disagree about the reference"
    assert torch.equal(e[:n], want_dev) and torch.equal(bits(e[:n]), bits(want_host)), (n, decay)
    assert e[n].item() == GUARD and torch.equal(p, p0), "a guard element or the parameters were written"
    if decay == 1.0:
        assert torch.equal(e[:n], e0[:n])                        # (torch.equal: 1 * (-0.0) + 0 * p is +0.0 by the expression itself)
    if decay == 0.0:
        assert torch.equal(e[:n], p0[:n])


@pytest.mark.parametrize("gscale", [1.0, 0.37])
@pytest.mark.parametrize("amsgrad", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_adamw_step_ema_equals_the_plain_step_plus_the_expression(n, amsgrad, gscale):
    capi, L = _lib()
    dev = torch.device("cuda:0")
    decay = 0.9
    plain, fused = Bucket(n, 300 + n, dev), Bucket(n, 300 + n, dev)
    ema = torch.cat([plain.p[:n].clone(), torch.tensor([GUARD], device=dev)])
    want = ema[:n].clone()
    if not amsgrad:
        plain.vm = fused.vm = None                               # a null max_exp_avg_sq
    stream = torch.cuda.current_stream(dev).cuda_stream
    for step in range(1, 4):
        grad = torch.cat([torch.randn(n, generator=torch.Generator().manual_seed(step)) * 10.0 ** (step - 2), torch.tensor([9.0])]).to(dev)
        plain.g.copy_(grad); fused.g.copy_(grad)
        assert host_step(plain, step, gscale, amsgrad) == capi.OARD_OK
        with torch.cuda.device(dev):
            rc = L.oard_adamw_step_ema(fused.p.data_ptr(), fused.g.data_ptr(), fused.m.data_ptr(), fused.v.data_ptr(),
                                       fused.vm.data_ptr() if fused.vm is not None else None, n, HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
                                       HYPER["eps"], HYPER["wd"], step, amsgrad, gscale, ema.data_ptr(), decay, stream)
        assert rc == capi.OARD_OK
        torch.cuda.synchronize()
        names = ("p", "g", "m", "v") + (("vm",) if amsgrad else ())
        for k in names:
            assert torch.equal(getattr(fused, k), getattr(plain, k)), (k, step)          # guards included
        want_host = host_ema(want, plain.p[:n], decay)
        want = dev_ema(want, plain.p[:n], decay)                  # the recursion on the PLAIN entry point's parameters
        assert torch.equal(ema[:n], want) and torch.equal(ema[:n].cpu(), want_host), step
        assert ema[n].item() == GUARD
    assert not torch.equal(ema[:n], plain.p[:n])


def _dev_step_ema(b, state, cap, norm, flag, clip, ema, decay):
    capi, L = _lib()
    dev = b.dev
    nf = torch.tensor([norm, flag], dtype=torch.float32, device=dev)
    out4 = torch.full((4,), -1.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = L.oard_adamw_step_dev_ema(b.p.data_ptr(), b.g.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), b.vm.data_ptr(), b.n, HYPER["lr"],
                                       HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], 1, clip, state.data_ptr(), cap, nf.data_ptr(),
                                       nf.data_ptr() + 4, out4.data_ptr(), None if ema is None else ema.data_ptr(), decay, stream)
    torch.cuda.synchronize()
    return rc, out4.cpu()


@pytest.mark.parametrize("n", [257, 513])
def test_adamw_step_dev_ema_accepted_and_skipped(n):
    capi, L = _lib()
    dev = torch.device("cuda:0")
    cap, decay = 50, 0.999
    hist = history(9, 4)
    b0 = Bucket(n, 500 + n, dev)
    ema0 = torch.cat([torch.randn(n, generator=torch.Generator().manual_seed(n)), torch.tensor([GUARD])]).to(dev)
    h = np.array(hist)
    g32 = float(np.float32(2.0 * (1.5 * float(np.mean(h)) + 3 * float(np.std(h)))))          # a clipped step
    # accepted: oard_adamw_step_dev on a clone, then the expression
    plain, st_plain = b0.clone(), make_state(hist, cap, 3, 1, dev)
    rc, out_plain = dev_step(plain, st_plain, cap, g32, 0.0, 1)
    assert rc == capi.OARD_OK and out_plain[3].item() == 0.0 and out_plain[2].item() < 1.0
    got, st_got, ema = b0.clone(), make_state(hist, cap, 3, 1, dev), ema0.clone()
    rc, out_got = _dev_step_ema(got, st_got, cap, g32, 0.0, 1, ema, decay)
    assert rc == capi.OARD_OK and torch.equal(out_got, out_plain)
    assert got.same_bits(plain) and torch.equal(st_got[:4 + cap], st_plain[:4 + cap])
    assert not torch.equal(got.p[:n], b0.p[:n])
    assert torch.equal(ema[:n], dev_ema(ema0[:n], plain.p[:n], decay)) and torch.equal(ema[:n].cpu(), host_ema(ema0[:n], plain.p[:n], decay))
    assert ema[n].item() == GUARD
    # skipped (raised flag; non-finite norm): parameters, moments and the average keep their bits, the skip is counted
    for norm, flag in ((0.25, 1.0), (float("nan"), 0.0)):
        got, state, ema = b0.clone(), make_state(hist, cap, 3, 1, dev), ema0.clone()
        before = state.cpu().clone()
        rc, out4 = _dev_step_ema(got, state, cap, norm, flag, 1, ema, decay)
        assert rc == capi.OARD_OK and out4[3].item() == 1.0
        st = state.cpu()
        assert st[2].item() == 2.0 and torch.equal(st[:2], before[:2]) and torch.equal(st[3: 4 + cap], before[3: 4 + cap])
        assert got.same_bits(b0) and torch.equal(ema, ema0), "a skipped step moved a parameter, a moment or the average"


@pytest.mark.parametrize("ema_null,decay", [(True, 0.5), (False, -0.1), (False, 1.5)])
def test_bad_arguments_are_refused_and_write_nothing(ema_null, decay):
    capi, L = _lib()
    dev = torch.device("cuda:0")
    n, cap = 300, 50
    hist = history(9, 4)
    b0 = Bucket(n, 77, dev)
    ema0 = torch.full((n + 1,), 2.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # oard_ema_update
    ema, p = ema0.clone(), b0.p.clone()
    with torch.cuda.device(dev):
        rc = L.oard_ema_update(None if ema_null else ema.data_ptr(), p.data_ptr(), n, decay, stream)
    torch.cuda.synchronize()
    assert rc == capi.OARD_EINVAL and torch.equal(ema, ema0) and torch.equal(p, b0.p)
    # oard_adamw_step_ema
    got, ema = b0.clone(), ema0.clone()
    with torch.cuda.device(dev):
        rc = L.oard_adamw_step_ema(got.p.data_ptr(), got.g.data_ptr(), got.m.data_ptr(), got.v.data_ptr(), got.vm.data_ptr(), n, HYPER["lr"],
                                   HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], 1, 1, 1.0, None if ema_null else ema.data_ptr(),
                                   decay, stream)
    torch.cuda.synchronize()
    assert rc == capi.OARD_EINVAL and got.same_bits(b0) and torch.equal(ema, ema0)
    # oard_adamw_step_dev_ema: not even the decision is taken
    got, ema, state = b0.clone(), ema0.clone(), make_state(hist, cap, 3, 1, dev)
    before = state.cpu().clone()
    rc, out4 = _dev_step_ema(got, state, cap, 0.5, 0.0, 1, None if ema_null else ema, decay)
    assert rc == capi.OARD_EINVAL and got.same_bits(b0) and torch.equal(ema, ema0)
    assert torch.equal(state.cpu(), before) and out4.tolist() == [-1.0] * 4
    assert host_rule(hist, 0.5, cap, 1)[0] != hist                      # (an accepted step would have pushed to the history)
