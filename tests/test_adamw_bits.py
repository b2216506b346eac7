"""The four AdamW entry points against the bits recorded before their kernels shared one body (tests/golden/adamw_bits.npz, written by
oracle/make_goldens_adamw.py on an MI355X from the four hand-copied kernels k_adamw, k_adamw_dev, k_adamw_ema and k_adamw_dev_ema).

The kernels are now instantiations of one `adamw_elem` whose products are rounded or fused as those four bodies were compiled, so the
gate is BIT EQUALITY of parameters, moments and the average - uint32 patterns, so that -0.0 and 0.0 differ.  Inputs are rebuilt here
from CPU-generator seeds; the fixture holds results only.  n = 257 is one full 256-thread block plus one thread; exact zeros, -0.0 and
float32 denormals sit among the parameters, moments and gradients, every value is finite and below 1e18 in magnitude (the squared
gradient stays finite, the denominator is at least eps), so no case produces inf or NaN.  Every buffer carries a guard element.

Part 1: oard_adamw_step_ema after three steps (gradients scaled 0.1, 1, 10) and oard_adamw_step_dev_ema after one accepted step from
a fixed history (with its out4) reproduce the fixture.  Part 2: oard_adamw_step and oard_adamw_step_dev give the same parameters and
moments and leave an average they were never given untouched.

MEASURED on an MI355X: both parts passed on the four hand-copied kernels (the commit before the shared body) and pass unchanged on it."""
import os

import numpy as np
import pytest
import torch

from test_optimizer_kernels import HYPER, SENTINEL, _lib, history, make_state

pytestmark = pytest.mark.gpu

N = 257
DECAY = 0.9
CAP = 50
CASES = [(amsgrad, gscale) for amsgrad in (0, 1) for gscale in (1.0, 0.37)]
GUARD = 11.0
NAMES = ("p", "m", "v", "vmax", "ema")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_bits.npz")
HIST = history(9, 4)
SPECIALS = [0.0, -0.0, 1e-40, -3e-42, 1.1754944e-38, 7e-46, -1.4e-45]


def case_key(amsgrad, gscale):
    return f"a{amsgrad}_g{gscale:g}"


def _plant(x, values, gen):
    idx = torch.randperm(N, generator=gen)[:len(values)]
    x[idx] = torch.tensor(values)
    return x


def make_inputs():
    """-> ({p, m, v, vmax, ema}: [N + 1] CPU tensors, the last element a guard; [three gradients, each [N + 1]])."""
    gen = torch.Generator().manual_seed(2570)
    t = {"p": _plant(torch.randn(N, generator=gen), SPECIALS + [1e17, -4e16], gen),
         "m": _plant(0.05 * torch.randn(N, generator=gen), SPECIALS, gen),
         "v": _plant(0.01 * torch.rand(N, generator=gen), [0.0, 1e-40, 3e-42, 1.1754944e-38, 2e15], gen),       # a second moment is >= 0
         "vmax": _plant(0.02 * torch.rand(N, generator=gen), [0.0, 2e-41, 5e16], gen),
         "ema": _plant(torch.randn(N, generator=gen), SPECIALS + [-2e17], gen)}
    grads = [_plant(torch.randn(N, generator=gen) * 10.0 ** (step - 2), SPECIALS + [3e15, -1e16], gen) for step in (1, 2, 3)]
    for x in list(t.values()) + grads:
        assert torch.isfinite(x).all() and float(x.abs().max()) < 1e18
    tail = torch.tensor([GUARD])
    return {k: torch.cat([x, tail]) for k, x in t.items()}, [torch.cat([g, tail]) for g in grads]


def bits(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint32)


def _pointers(t, grad, with_ema):
    head = (t["p"].data_ptr(), grad.data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["vmax"].data_ptr())
    return head, ((t["ema"].data_ptr(), DECAY) if with_ema else ())


def run_host(amsgrad, gscale, with_ema, dev):
    """Three steps of oard_adamw_step_ema (or oard_adamw_step) -> the five buffers on the device, guards included."""
    capi, L = _lib()
    t0, grads = make_inputs()
    t = {k: x.to(dev) for k, x in t0.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = L.oard_adamw_step_ema if with_ema else L.oard_adamw_step
    for step, grad in enumerate(grads, 1):
        grad = grad.to(dev)
        head, ema = _pointers(t, grad, with_ema)
        with torch.cuda.device(dev):
            rc = fn(*head, N, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], step, amsgrad, gscale, *ema, stream)
        assert rc == capi.OARD_OK
        torch.cuda.synchronize()
        assert grad[N].item() == GUARD
    return t


def dev_norm(gscale):
    """A gradient norm that passes the clipping rule for gscale = 1 and is clipped to about `gscale` of itself otherwise."""
    h = np.array(HIST)
    max_norm = 1.5 * float(np.mean(h)) + 3 * float(np.std(h))
    return float(np.float32(0.9 * max_norm if gscale == 1.0 else max_norm / gscale))


def run_dev(amsgrad, gscale, with_ema, dev):
    """One accepted step of oard_adamw_step_dev_ema (or oard_adamw_step_dev) from HIST with 3 steps taken, on the second gradient
    -> (the five buffers, out4)."""
    capi, L = _lib()
    t0, grads = make_inputs()
    t = {k: x.to(dev) for k, x in t0.items()}
    grad = grads[1].to(dev)
    state = make_state(HIST, CAP, 3, 1, dev)
    nf = torch.tensor([dev_norm(gscale), 0.0], dtype=torch.float32, device=dev)
    out4 = torch.full((4,), -1.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = L.oard_adamw_step_dev_ema if with_ema else L.oard_adamw_step_dev
    head, ema = _pointers(t, grad, with_ema)
    with torch.cuda.device(dev):
        rc = fn(*head, N, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["wd"], amsgrad, 1, state.data_ptr(), CAP,
                nf.data_ptr(), nf.data_ptr() + 4, out4.data_ptr(), *ema, stream)
    assert rc == capi.OARD_OK
    torch.cuda.synchronize()
    st = state.cpu()
    assert st[:3].tolist() == [len(HIST) + 1.0, 4.0, 1.0] and st[4 + len(HIST) + 1].item() == SENTINEL
    assert grad[N].item() == GUARD and torch.equal(grad.cpu(), grads[1])
    return t, out4


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same(got, golden, prefix, names, what):
    for k in names:
        want = golden[f"{prefix}_{k}"]
        assert want.dtype == np.uint32 and want.shape == (N + 1,)
        b = bits(got[k])
        differ = np.flatnonzero(b != want)
        print(f"{what} {prefix} {k}: {differ.size} of {N + 1} bit patterns differ")
        assert differ.size == 0, (what, prefix, k, differ[:8].tolist())


@pytest.mark.parametrize("amsgrad,gscale", CASES)
def test_ema_entry_points_reproduce_the_recorded_bits(golden, amsgrad, gscale):
    dev = torch.device("cuda:0")
    key = case_key(amsgrad, gscale)
    t0, _ = make_inputs()
    got = run_host(amsgrad, gscale, True, dev)
    _same(got, golden, f"host_{key}", NAMES, "oard_adamw_step_ema")
    assert all(got[k][N].item() == GUARD for k in NAMES)
    assert not torch.equal(got["p"].cpu(), t0["p"]) and not torch.equal(got["ema"].cpu(), t0["ema"])
    assert torch.equal(got["vmax"].cpu(), t0["vmax"]) != bool(amsgrad)
    got, out4 = run_dev(amsgrad, gscale, True, dev)
    _same(got, golden, f"dev_{key}", NAMES, "oard_adamw_step_dev_ema")
    assert np.array_equal(bits(out4), golden[f"dev_{key}_out4"]), out4.tolist()
    assert out4[3].item() == 0.0 and (out4[2].item() == 1.0) == (gscale == 1.0) and abs(out4[2].item() - gscale) < 1e-5
    assert all(got[k][N].item() == GUARD for k in NAMES)
    for k in NAMES:
        assert np.isfinite(got[k].cpu().numpy()).all(), k


@pytest.mark.parametrize("amsgrad,gscale", CASES)
def test_plain_entry_points_give_the_same_bits_and_leave_the_average(golden, amsgrad, gscale):
    dev = torch.device("cuda:0")
    key = case_key(amsgrad, gscale)
    t0, _ = make_inputs()
    got = run_host(amsgrad, gscale, False, dev)
    _same(got, golden, f"host_{key}", NAMES[:4], "oard_adamw_step")
    assert np.array_equal(bits(got["ema"]), bits(t0["ema"])), "oard_adamw_step wrote an average it was not given"
    got, out4 = run_dev(amsgrad, gscale, False, dev)
    _same(got, golden, f"dev_{key}", NAMES[:4], "oard_adamw_step_dev")
    assert np.array_equal(bits(out4), golden[f"dev_{key}_out4"]), out4.tolist()
    assert np.array_equal(bits(got["ema"]), bits(t0["ema"])), "oard_adamw_step_dev wrote an average it was not given"
    assert all(got[k][N].item() == GUARD for k in NAMES)
