"""oareactdiff_amd.metrics: `batch_rmsd` with the reference's signature and defaults (analyze/rmsd.py:78-100) and `kabsch_rmsd` under it,
against the float64 SVD reference of tests/_kabsch_cases.py (same-order Kabsch fit, minimum over the structure and its z-mirror) with the
gate of tests/test_kabsch_kernel.py."""
import numpy as np
import pytest
import torch

import _kabsch_cases as kc

SIZES = [4, 7, 1, 5]
WIDTH = 9


def _lists(seed=0):
    """Per-object sample lists as `inpaint` returns them ([n, 9]: positions, one-hot, charge) and the true structures, three objects with
    the same ragged sizes; the generated object is the true one moved rigidly plus noise of a size that puts the RMSDs on both sides of 1."""
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    xh, out = [], []
    for k in range(3):
        x = rng.standard_normal((n, WIDTH)).astype(np.float32)
        x[:, :3] *= 1.5
        y = x.copy()
        p = kc.seg_ptr(SIZES)
        for g in range(len(SIZES)):
            s = slice(p[g], p[g + 1])
            y[s, :3] = x[s, :3] @ kc.random_rotation(rng).T.astype(np.float32) + rng.standard_normal(3).astype(np.float32) \
                + (0.2 + 0.6 * g) * rng.standard_normal((SIZES[g], 3)).astype(np.float32)
        xh.append(x)
        out.append(y)
    return xh, out


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_batch_rmsd_reproduces_the_reference(idx):
    from oareactdiff_amd.metrics import batch_rmsd, kabsch_rmsd
    dev = torch.device("cuda:0")
    xh, out = _lists()
    frag = [torch.tensor(SIZES, device=dev) for _ in range(3)]
    xh_d, out_d = [torch.from_numpy(x).to(dev) for x in xh], [torch.from_numpy(x).to(dev) for x in out]
    r, rho = kc.reference(xh[idx], out[idx], SIZES, True)
    assert (r > 1.0).any() and (r < 1.0).any()
    kw = {} if idx == 1 else {"idx": idx}                        # idx = 1 is the default
    capped = batch_rmsd(frag, out_d, xh_d, **kw)
    assert capped.shape == (len(SIZES),) and capped.is_cuda and capped.dtype == torch.float32
    assert len(capped.tolist()) == len(SIZES)
    free = batch_rmsd(frag, out_d, xh_d, cap=None, **kw)
    for g in range(len(SIZES)):
        print(f"idx={idx} n={SIZES[g]}: kernel {float(free[g]):.9g} reference {r[g]:.9g}")
        assert abs(float(free[g]) - r[g]) <= kc.gate(r[g], rho[g])
        assert abs(float(capped[g]) - min(r[g], 1.0)) <= kc.gate(min(r[g], 1.0), rho[g])
    assert float(capped.max()) == 1.0
    # without the reflection: the proper-rotation reference, never below the other
    r0, rho0 = kc.reference(xh[idx], out[idx], SIZES, False)
    proper = batch_rmsd(frag, out_d, xh_d, ignore_chirality=False, cap=None, **kw)
    for g in range(len(SIZES)):
        assert abs(float(proper[g]) - r0[g]) <= kc.gate(r0[g], rho0[g])
    assert bool((proper >= free).all())
    # the sample tensors are read where they lie: a [n, 3] view of the [n, 9] tensor, host sizes, the optional outputs
    rm, rot, al = kabsch_rmsd(xh_d[idx][:, :3], out_d[idx], SIZES, cap=None, return_rotation=True, return_aligned=True)
    assert torch.equal(rm, free) and rot.shape == (len(SIZES), 3, 3) and al.shape == (sum(SIZES), 3)
    back = torch.sqrt(((al.double() - xh_d[idx][:, :3].double()) ** 2).sum(1))
    p = kc.seg_ptr(SIZES)
    for g in range(len(SIZES)):
        got = float(torch.sqrt((back[p[g]: p[g + 1]] ** 2).mean()))
        assert abs(got - r[g]) <= 1e-6 * (np.abs(xh[idx][:, :3]).max() + np.abs(out[idx][:, :3]).max())


@pytest.mark.gpu
def test_wrong_sizes_cannot_leave_the_tensors():
    from oareactdiff_amd.metrics import kabsch_rmsd
    dev = torch.device("cuda:0")
    xh, out = _lists()
    a, b = torch.from_numpy(xh[1]).to(dev), torch.from_numpy(out[1]).to(dev)
    with pytest.raises(ValueError):
        kabsch_rmsd(a, b, [4, 7, 1, 6])
    with pytest.raises(ValueError):
        kabsch_rmsd(a, b[:-1], SIZES)
    # device sizes are not read back: the boundaries are clamped to the rows that exist
    r = kabsch_rmsd(a, b, torch.tensor([4, 7, 1, 600, 3], device=dev), cap=None)
    want = kabsch_rmsd(a, b, SIZES + [0], cap=None)
    assert torch.equal(r[:3], want[:3]) and torch.equal(r[3:4], want[3:4]) and bool(torch.isnan(r[4])) and bool(torch.isnan(want[4]))


def test_cpu_tensors_raise():
    from oareactdiff_amd._capi import OardError
    from oareactdiff_amd.metrics import batch_rmsd, kabsch_rmsd
    xh, out = _lists()
    a, b = torch.from_numpy(xh[1]), torch.from_numpy(out[1])
    with pytest.raises(OardError):
        kabsch_rmsd(a, b, SIZES)
    with pytest.raises(OardError):
        batch_rmsd([torch.tensor(SIZES)] * 3, [torch.from_numpy(x) for x in out], [torch.from_numpy(x) for x in xh])
