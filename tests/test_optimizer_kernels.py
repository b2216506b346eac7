"""k_clip_decide / k_adamw<DEV> (behind oard_adamw_step_dev) and k_adamw (behind oard_adamw_step) on their own.

The device-side clipping decision against the host rule of DDPMTrainer (pl_trainer.py:391-418, utils/training_tools.py:6-23) restated
here in Python floats and numpy: max_norm = 1.5 np.mean(h) + 3 np.std(h), clip if g > max_norm with the factor max_norm / (g + 1e-6),
push min(g, max_norm) at the front, drop what falls beyond the capacity - at history lengths on both sides of every branch of the
kernel's pairwise sum (n < 8, n % 8 != 0, n = 8 k), with the queue full (the history shifts and drops its oldest entry), at capacities
1, 50 and 64, with clip = 0, with a raised flag and with non-finite norms.  History, counters and the passed-through norm must be the
reference's bits; max_norm and the factor (float32 outputs) agree to 1e-6; parameters and moments are those of oard_adamw_step called
with the host-derived step and factor (test_trainer_fused.test_adamw_kernel_matches_torch pins that one to torch.optim.AdamW).

MEASURED on an MI355X: in all 26 parametrised cases and the further ones the history, the counters and out4[0] are the reference's
bits, max_norm and the factor agree with the reference's doubles to the 7 digits printed (bound 1e-6), and the parameters are
bit-identical to oard_adamw_step's.  test_adamw_extents: max |p - torch| 7.15e-07 after three steps (n = 255, 256), bound 3e-6."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HYPER = dict(lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
N_PARAM = 5000
SENTINEL = -7.0                    # history slots beyond the entries in use: must stay as they are


def host_rule(hist, g, cap, clip):
    """-> (history, max_norm, factor) of one accepted step, as DDPMTrainer._fused_step decides on the host."""
    if not clip:
        return list(hist), float("nan"), 1.0
    h = np.array(hist, dtype=np.float64)
    max_norm = 1.5 * float(np.mean(h)) + 3 * float(np.std(h))
    factor, push = 1.0, g
    if g > max_norm:
        factor, push = max_norm / (g + 1e-6), float(max_norm)
    return ([push] + list(hist))[:cap], max_norm, factor


def history(n, seed):
    """n positive entries over two decades."""
    r = np.random.RandomState(seed)
    return [float(x) for x in 0.3 * 10.0 ** r.uniform(-1.0, 1.0, n)]


class Bucket:
    """Parameters, gradient and AdamW moments of n elements, each with a guard element behind it."""

    def __init__(self, n, seed, dev):
        g = torch.Generator().manual_seed(seed)
        self.n, self.dev = n, dev
        self.p = torch.randn(n + 1, generator=g).to(dev)
        self.g = (0.1 * torch.randn(n + 1, generator=g)).to(dev)
        self.m = (0.05 * torch.randn(n + 1, generator=g)).to(dev)
        self.v = (0.01 * torch.rand(n + 1, generator=g)).to(dev)
        self.vm = (0.02 * torch.rand(n + 1, generator=g)).to(dev)

    def clone(self):
        other = Bucket.__new__(Bucket)
        other.n, other.dev = self.n, self.dev
        for k in ("p", "g", "m", "v", "vm"):
            setattr(other, k, getattr(self, k).clone())
        return other

    def tensors(self):
        return self.p, self.g, self.m, self.v, self.vm

    def same_bits(self, other):
        return all(torch.equal(a, b) for a, b in zip(self.tensors(), other.tensors()))

    def guards_of(self, other):
        return all(torch.equal(a[self.n:], b[self.n:]) for a, b in zip(self.tensors(), other.tensors()))


def _lib():
    from oareactdiff_amd import _capi
    return _capi, _capi.lib()


def host_step(b, step, factor, amsgrad=1):
    capi, L = _lib()
    stream = torch.cuda.current_stream(b.dev).cuda_stream
    with torch.cuda.device(b.dev):
        return L.oard_adamw_step(b.p.data_ptr(), b.g.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), b.vm.data_ptr() if b.vm is not None else None,
                                 b.n, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], step, amsgrad, factor, stream)


def make_state(hist, cap, steps, skipped, dev):
    st = torch.full((4 + cap + 8,), SENTINEL, dtype=torch.float64)
    st[0], st[1], st[2], st[3] = len(hist), steps, skipped, 0.0
    if hist:
        st[4: 4 + len(hist)] = torch.tensor(hist, dtype=torch.float64)
    return st.to(dev)


def dev_step(b, state, cap, norm, flag, clip, n=None):
    """oard_adamw_step_dev -> (rc, out4 on the host)."""
    capi, L = _lib()
    dev = b.dev
    nf = torch.tensor([norm, flag], dtype=torch.float32, device=dev)
    out4 = torch.full((4,), -1.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        rc = L.oard_adamw_step_dev(b.p.data_ptr(), b.g.data_ptr(), b.m.data_ptr(), b.v.data_ptr(), b.vm.data_ptr(), b.n if n is None else n,
                                   HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], 1, clip, state.data_ptr(), cap,
                                   nf.data_ptr(), nf.data_ptr() + 4, out4.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, out4.cpu()


def check_accepted(b0, hist, cap, steps, skipped, g32, clip, what, n=None):
    """One accepted step from (b0, hist): device decision against the host rule, parameters against oard_adamw_step.
    -> (the bucket after the step, the new history)."""
    capi, L = _lib()
    dev = b0.dev
    want_hist, max_norm, factor = host_rule(hist, g32, cap, clip)
    got, state = b0.clone(), make_state(hist, cap, steps, skipped, dev)
    rc, out4 = dev_step(got, state, cap, g32, 0.0, clip, n=n)
    assert rc == capi.OARD_OK, what
    st = state.cpu()
    # bit-equal: the history (and nothing beyond it), the three counters, the norm passed through
    assert st[0].item() == len(want_hist) and st[1].item() == steps + 1 and st[2].item() == skipped, (what, st[:4].tolist())
    assert st[4: 4 + len(want_hist)].tolist() == want_hist, (what, st[4: 4 + len(want_hist)].tolist()[:3], want_hist[:3])
    assert st[4 + len(want_hist): 4 + cap].tolist() == [SENTINEL] * (cap - len(want_hist)), what
    assert out4[0].item() == g32 and out4[3].item() == 0.0, (what, out4.tolist())
    if clip:
        e_max = abs(out4[1].item() - max_norm) / abs(max_norm)
        assert e_max <= 1e-6, (what, out4[1].item(), max_norm)
    else:
        assert math.isnan(out4[1].item()), what
    e_fac = abs(out4[2].item() - factor) / abs(factor)
    assert e_fac <= 1e-6, (what, out4[2].item(), factor)
    ref = b0.clone()
    if (b0.n if n is None else n) > 0:
        assert host_step(ref, steps + 1, factor) == capi.OARD_OK
        torch.cuda.synchronize()
    for name, x, y in zip(("param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), got.tensors(), ref.tensors()):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-9), (what, name, float((x - y).abs().max()))
    assert got.guards_of(b0) and torch.equal(got.g, b0.g), what
    print(f"{what}: max_norm {max_norm:.6e} factor {factor:.6e}; out4 {out4.tolist()}; parameters identical to oard_adamw_step: "
          f"{torch.equal(got.p, ref.p)}, max |dp| {float((got.p - ref.p).abs().max()):.2e}")
    return got, want_hist


CAP_N = [(50, n) for n in (1, 2, 7, 8, 9, 15, 16, 17, 49, 50)] + [(64, 63), (64, 64), (1, 1)]


@pytest.mark.parametrize("clipping", [True, False], ids=["norm_clips", "norm_passes"])
@pytest.mark.parametrize("cap,n", CAP_N)
def test_device_decision_matches_the_host_rule(cap, n, clipping):
    dev = torch.device("cuda:0")
    hist = history(n, 1000 * cap + n)
    assert min(hist) > 0 and (n < 8 or max(hist) / min(hist) > 10)
    h = np.array(hist)
    max_norm = 1.5 * float(np.mean(h)) + 3 * float(np.std(h))
    g32 = float(np.float32((2.5 if clipping else 0.9) * max_norm))
    assert (g32 > max_norm) == clipping
    b0 = Bucket(N_PARAM, 7, dev)
    _, new = check_accepted(b0, hist, cap, 7, 2, g32, 1, f"capacity {cap} history {n} clipping {clipping}")
    assert len(new) == min(n + 1, cap) and new[1:] == hist[:len(new) - 1]
    if n == cap and cap > 1:
        assert hist[-1] not in new                  # the oldest entry is dropped


def test_three_steps_read_the_step_count_from_device_memory():
    """Three consecutive steps on ONE state buffer (clipped, not clipped, clipped), no host write in between."""
    capi, L = _lib()
    dev = torch.device("cuda:0")
    cap, steps0 = 50, 3
    hist = history(49, 5)
    state = make_state(hist, cap, steps0, 0, dev)
    got, ref = Bucket(N_PARAM, 9, dev), Bucket(N_PARAM, 9, dev)
    for i, mult in enumerate((3.0, 0.5, 1.7)):
        h = np.array(hist)
        g32 = float(np.float32(mult * (1.5 * float(np.mean(h)) + 3 * float(np.std(h)))))
        hist, max_norm, factor = host_rule(hist, g32, cap, 1)
        assert (factor != 1.0) == (mult > 1)
        grad = (0.1 * torch.randn(N_PARAM + 1, generator=torch.Generator().manual_seed(40 + i))).to(dev)
        got.g.copy_(grad); ref.g.copy_(grad)
        rc, out4 = dev_step(got, state, cap, g32, 0.0, 1)
        assert rc == capi.OARD_OK and out4[3].item() == 0.0
        assert host_step(ref, steps0 + 1 + i, factor) == capi.OARD_OK
        torch.cuda.synchronize()
        st = state.cpu()
        assert st[:3].tolist() == [float(len(hist)), float(steps0 + 1 + i), 0.0]
        assert st[4: 4 + len(hist)].tolist() == hist, i
        for x, y in zip(got.tensors(), ref.tensors()):
            assert torch.allclose(x, y, rtol=1e-6, atol=1e-9), i
    assert len(hist) == cap


def test_clip_off_takes_the_step_and_leaves_the_history():
    dev = torch.device("cuda:0")
    hist = history(9, 3)
    check_accepted(Bucket(N_PARAM, 11, dev), hist, 50, 4, 1, float(np.float32(1e3 * max(hist))), 0, "clip = 0")


@pytest.mark.parametrize("norm,flag", [(0.25, 1.0), (0.25, -3.0), (float("inf"), 0.0), (float("nan"), 0.0), (float("-inf"), 0.0)])
def test_skipped_step_touches_nothing_but_the_skip_count(norm, flag):
    capi, L = _lib()
    dev = torch.device("cuda:0")
    cap = 50
    for clip in (1, 0):
        hist = history(17, 8)
        b0 = Bucket(N_PARAM, 13, dev)
        got, state = b0.clone(), make_state(hist, cap, 6, 2, dev)
        before = state.cpu().clone()
        rc, out4 = dev_step(got, state, cap, norm, flag, clip)
        assert rc == capi.OARD_OK
        st = state.cpu()
        assert st[2].item() == 3.0
        assert torch.equal(st[:2], before[:2]) and torch.equal(st[3: 4 + cap], before[3: 4 + cap]), "history / counters of a skipped step"
        assert got.same_bits(b0), "a skipped step moved a parameter or a moment"
        g32 = float(np.float32(norm))
        assert (math.isnan(out4[0].item()) and math.isnan(g32)) or out4[0].item() == g32
        assert math.isnan(out4[1].item()) and out4[2].item() == 1.0 and out4[3].item() == 1.0, out4.tolist()
        # ... and the next accepted step on the same state carries on from the untouched counters
        rc, out4 = dev_step(got, state, cap, 0.25, 0.0, clip)
        assert rc == capi.OARD_OK and out4[3].item() == 0.0
        st = state.cpu()
        assert st[1].item() == 7.0 and st[2].item() == 3.0
        ref = b0.clone()
        _, _, factor = host_rule(hist, 0.25, cap, clip)
        assert host_step(ref, 7, factor) == capi.OARD_OK
        torch.cuda.synchronize()
        assert all(torch.allclose(x, y, rtol=1e-6, atol=1e-9) for x, y in zip(got.tensors(), ref.tensors()))


def test_no_parameters_and_bad_capacities():
    capi, L = _lib()
    dev = torch.device("cuda:0")
    hist = history(8, 21)
    b0 = Bucket(4, 17, dev)
    # n = 0: the decision is taken (history, step count), no parameter is touched
    got, _ = check_accepted(b0, hist, 50, 1, 0, float(np.float32(10 * max(hist))), 1, "n = 0", n=0)
    assert got.same_bits(b0)
    for cap in (0, 65, -1):
        got, state = b0.clone(), make_state(hist, 64, 1, 0, dev)
        before = state.cpu().clone()
        rc, out4 = dev_step(got, state, cap, 0.5, 0.0, 1)
        assert rc == capi.OARD_EINVAL, cap
        assert torch.equal(state.cpu(), before) and got.same_bits(b0) and out4.tolist() == [-1.0] * 4, f"capacity {cap}: something was launched"


@pytest.mark.parametrize("amsgrad", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_adamw_extents(n, amsgrad):
    """oard_adamw_step around its 256-thread block: against torch.optim.AdamW(foreach=False) over three steps with the 3e-6 bound of
    test_adamw_kernel_matches_torch; a guard element behind every buffer stays; amsgrad = 0 takes a null max_exp_avg_sq; step = 0 is
    refused."""
    capi, L = _lib()
    dev = torch.device("cuda:0")
    b = Bucket(n, 100 + n, dev)
    b.m.zero_(); b.v.zero_(); b.vm.zero_()                   # torch.optim.AdamW starts from zero moments
    b.m[n], b.v[n], b.vm[n] = 3.0, 4.0, 5.0                  # the guards
    b0 = b.clone()
    if not amsgrad:
        b.vm = None
    # step = 0: refused, nothing launched
    assert host_step(b, 0, 1.0, amsgrad) == capi.OARD_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(b.tensors()[:4], b0.tensors()[:4]))
    ref = torch.nn.Parameter(b0.p[:n].clone())
    opt = torch.optim.AdamW([ref], lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=HYPER["wd"],
                            amsgrad=bool(amsgrad), foreach=False)
    gen = torch.Generator().manual_seed(n)
    gscale = 0.37
    for step in range(1, 4):
        grad = torch.cat([torch.randn(n, generator=gen) * 10.0 ** (step - 2), torch.tensor([9.0])]).to(dev)
        b.g.copy_(grad)
        if n > 0:
            ref.grad = grad[:n] * gscale
            opt.step()
        assert host_step(b, step, gscale, amsgrad) == capi.OARD_OK
        torch.cuda.synchronize()
        if n > 0:
            e = float((b.p[:n] - ref.detach()).abs().max())
            print(f"n {n} amsgrad {amsgrad} step {step}: max |p - torch| {e:.2e}")
            assert e <= 3e-6, (step, e)
            # the moments: the same formulas up to the order of one product (w2 (g g) here, (w2 g) g in addcmul_): a few float32
            # roundings per step over three steps stay under 1e-6 relative; 1e-5 leaves a decade
            st = opt.state[ref]
            assert torch.allclose(b.m[:n], st["exp_avg"], rtol=1e-5, atol=1e-9) and torch.allclose(b.v[:n], st["exp_avg_sq"], rtol=1e-5, atol=1e-12)
            if amsgrad:
                assert torch.allclose(b.vm[:n], st["max_exp_avg_sq"], rtol=1e-5, atol=1e-12)
        assert b.p[n].item() == b0.p[n].item() and b.m[n].item() == 3.0 and b.v[n].item() == 4.0 and b.g[n].item() == 9.0, "a guard element was written"
        if amsgrad:
            assert b.vm[n].item() == 5.0
    if n > 0:
        assert not torch.equal(b.p[:n], b0.p[:n])
