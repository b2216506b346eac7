"""k_kabsch_rmsd through the C ABI alone (`oard_kabsch_rmsd`, include/oard.h): the optimal-superposition RMSD per segment against a
float64 reference computed on the host by a different algorithm (SVD of the covariance, determinant corrected, residual RMSD; the minimum
over b and its z-mirror for the reflection flag) - tests/_kabsch_cases.py.

Gate per segment: |k - r| <= 2^-23 r + 1e-10 rho, rho = sqrt((G_a + G_b) / (2 n)) - one rounding of the float32 output, and float64
arithmetic with five orders of margin for another summation order at n = 1024 and an offset of 60.
Measured on an MI355X (worst over all kinds, sizes and both flags): |k - r| = 0.455 of the gate; the kernel returns fl32(r) itself in every
segment except where r is rounding noise (identical structures, the mirror image with the flag), and there |k - fl32(r)| <= 7.8e-16 rho."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _kabsch_cases as kc

pytestmark = pytest.mark.gpu
GUARD = 8


def _dev():
    return torch.device("cuda:0")


def _lib():
    from oareactdiff_amd import _capi
    return _capi, _capi.lib()


@functools.lru_cache(maxsize=None)
def _case(kind):
    a, b = kc.make_kind(kind)
    ref = {f: kc.reference(a, b, kc.SIZES, bool(f)) for f in (0, 1)}
    return a, b, ref


def _launch(a, b, sizes, flags=0, cap=0.0, lda=3, ldb=3, rot=True, aligned=True):
    """a, b: float32 numpy [n, 3], laid out on the device with row strides lda / ldb (the other columns NaN).  Outputs carry GUARD NaN
    rows behind them.  -> (rmsd [G], rot [G, 3, 3] | None, aligned [n, 3] | None) as numpy."""
    _capi, L = _lib()
    dev = _dev()
    n, G = len(a), len(sizes)
    wide = []
    for x, ld in ((a, lda), (b, ldb)):
        w = torch.full((max(n, 1), ld), float("nan"), device=dev)
        w[:n, :3] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        wide.append(w)
    ptr = torch.from_numpy(kc.seg_ptr(sizes).astype(np.int32)).to(dev)
    nan = float("nan")
    o_r = torch.full((G + GUARD,), nan, device=dev)
    o_m = torch.full((G + GUARD, 9), nan, device=dev) if rot else None
    o_a = torch.full((n + GUARD, 3), nan, device=dev) if aligned else None
    with torch.cuda.device(dev):
        rc = L.oard_kabsch_rmsd(wide[0].data_ptr(), lda, wide[1].data_ptr(), ldb, ptr.data_ptr(), G, flags, cap, o_r.data_ptr(),
                                None if o_m is None else o_m.data_ptr(), None if o_a is None else o_a.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    for w, ld in zip(wide, (lda, ldb)):                          # inputs untouched, the padding columns still NaN
        assert ld == 3 or bool(torch.isnan(w[:, 3:]).all())
    guards = [o_r[G:]] + ([o_m[G:]] if rot else []) + ([o_a[n:]] if aligned else [])
    assert all(bool(torch.isnan(g).all()) for g in guards), "a guard row behind an output was written"
    return (o_r[:G].cpu().numpy(), o_m[:G].cpu().numpy().reshape(G, 3, 3) if rot else None, o_a[:n].cpu().numpy() if aligned else None)


def _check_parity(k, ref, sizes, what):
    r, rho = ref
    frac = beyond = 0.0
    for g, n in enumerate(sizes):
        if n == 0:
            assert np.isnan(k[g]), (what, g)
            continue
        err, lim = abs(float(k[g]) - r[g]), kc.gate(r[g], rho[g])
        print(f"  {what} n={n}: kernel {float(k[g]):.9g} reference {r[g]:.9g} |diff| {err:.2e} gate {lim:.2e}")
        assert err <= lim, (what, n, float(k[g]), r[g], err, lim)
        frac = max(frac, err / lim if lim > 0 else 0.0)
        if rho[g] > 0:                               # the float64 part alone: what is left beside the output's own rounding
            beyond = max(beyond, abs(float(k[g]) - float(np.float32(r[g]))) / rho[g])
    return frac, beyond


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind", kc.KINDS)
def test_parity(kind, flags):
    a, b, ref = _case(kind)
    k, _, _ = _launch(a, b, kc.SIZES, flags)
    frac, beyond = _check_parity(k, ref[flags], kc.SIZES, f"{kind} flags={flags}")
    print(f"{kind} flags={flags}: worst |k - r| / gate = {frac:.3f}; worst |k - fl32(r)| / rho = {beyond:.2e}")


def test_strides_and_bounds():
    """lda = 9, ldb = 6 with NaN in every column that is not a coordinate: the same bits as the dense launch; nothing behind an output is
    written (`_launch` checks the guard rows of every launch of this file)."""
    a, b, ref = _case("rigid_noise")
    dense = _launch(a, b, kc.SIZES, 1)
    wide = _launch(a, b, kc.SIZES, 1, lda=9, ldb=6)
    for d, w in zip(dense, wide):
        assert np.array_equal(d, w, equal_nan=True)
    _check_parity(wide[0], ref[1], kc.SIZES, "strided")
    only = _launch(a, b, kc.SIZES, 1, lda=9, ldb=6, rot=False, aligned=False)
    assert only[1] is None and only[2] is None and np.array_equal(only[0], dense[0], equal_nan=True)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind", kc.KINDS)
def test_rot_and_aligned(kind, flags):
    a, b, ref = _case(kind)
    k, rot, al = _launch(a, b, kc.SIZES, flags)
    p = kc.seg_ptr(kc.SIZES)
    for g, n in enumerate(kc.SIZES):
        if n == 0:
            assert np.isnan(rot[g]).all()
            continue
        R = rot[g].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6, (kind, n)
        if kind in kc.DEGENERATE:
            continue                                             # R is not unique there: orthogonality and the RMSD (test_parity) only
        det = np.linalg.det(R)
        if flags == 0:
            assert abs(det - 1.0) <= 1e-5, (kind, n, det)
        elif kind == "mirror" and n >= 4:
            assert abs(det + 1.0) <= 1e-5, (kind, n, det)
        sa, sb = a[p[g]: p[g + 1]].astype(np.float64), b[p[g]: p[g + 1]].astype(np.float64)
        want = (sb - sb.mean(0)) @ R.T + sa.mean(0)
        assert np.abs(al[p[g]: p[g + 1]] - want).max() <= 2.0 ** -22 * np.abs(sa).max(), (kind, n)
        # and it IS the superposition: its distance from a is the RMSD
        # (aligned differs from the exact superposition by its own float32 rounding, 2^-24 |aligned|, and by rot's, 3 x 2^-25 |b - c_b|, per
        # coordinate: under sqrt(3) x 2^-22 x scale as an RMS over the rows; 1e-6 x scale bounds that)
        back = np.sqrt(np.sum((al[p[g]: p[g + 1]].astype(np.float64) - sa) ** 2) / n)
        scale = np.abs(sa).max() + np.abs(sb - sb.mean(0)).max()
        assert abs(back - ref[flags][0][g]) <= 1e-6 * scale, (kind, n)


def test_special_segments():
    a, b, ref = _case("independent")
    p = kc.seg_ptr(kc.SIZES)
    empty = kc.SIZES.index(0)
    clean = {cap: _launch(a, b, kc.SIZES, 1, cap=cap)[0] for cap in (0.0, 0.5)}
    assert np.isnan(clean[0.0][empty]) and np.isnan(clean[0.5][empty])
    r = ref[1][0]
    live = [g for g, n in enumerate(kc.SIZES) if n]
    assert np.array_equal(clean[0.5][live], np.minimum(clean[0.0][live], np.float32(0.5)))
    assert (clean[0.0][live] > 0.5).any() and (clean[0.0][live] < 0.5).any()      # the cap both bites and does not
    g_nan, g_inf = kc.SIZES.index(23), kc.SIZES.index(129)
    pa, pb = a.copy(), b.copy()
    pa[p[g_nan] + 5, 1] = np.nan
    pb[p[g_inf] + 100, 2] = np.inf
    for cap in (0.0, 0.5):
        k, rot, al = _launch(pa, pb, kc.SIZES, 1, cap=cap)
        for g in (g_nan, g_inf):
            assert (np.isnan(k[g]) if cap == 0.0 else k[g] == np.float32(cap)), (cap, g, k[g])
            assert np.isnan(rot[g]).all() and np.isnan(al[p[g]: p[g + 1]]).all()
        others = [g for g in range(len(kc.SIZES)) if g not in (g_nan, g_inf)]
        assert np.array_equal(k[others].view(np.uint32), clean[cap][others].view(np.uint32)), "a poisoned segment changed another one"
    assert np.isfinite(r[live]).all()


def test_repeatable_and_independent_of_the_launch():
    a, b, _ = _case("offset")
    one = _launch(a, b, kc.SIZES, 1)
    two = _launch(a, b, kc.SIZES, 1)
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)
    p = kc.seg_ptr(kc.SIZES)
    g = kc.SIZES.index(23)
    alone = _launch(a[p[g]: p[g + 1]], b[p[g]: p[g + 1]], [23], 1)
    assert alone[0][0].view(np.uint32) == one[0][g].view(np.uint32)
    assert np.array_equal(alone[1][0], one[1][g]) and np.array_equal(alone[2], one[2][p[g]: p[g + 1]])


def test_argument_checks():
    _capi, L = _lib()
    dev = _dev()
    a = torch.zeros(4, 3, device=dev)
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    out = torch.full((4,), float("nan"), device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    A, P, O = a.data_ptr(), ptr.data_ptr(), out.data_ptr()
    f = C.c_float(0.0)
    with torch.cuda.device(dev):
        for args in ((None, 3, A, 3, P, 1), (A, 3, None, 3, P, 1), (A, 3, A, 3, None, 1), (A, 3, A, 3, P, -1), (A, 2, A, 3, P, 1),
                     (A, 3, A, 2, P, 1)):
            assert L.oard_kabsch_rmsd(*args, 0, f, O, None, None, st) == _capi.OARD_EINVAL, args
        assert L.oard_kabsch_rmsd(A, 3, A, 3, P, 1, 0, f, None, None, None, st) == _capi.OARD_EINVAL
        assert L.oard_kabsch_rmsd(A, 3, A, 3, P, 0, 0, f, O, None, None, st) == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out).all()), "n_segments = 0 wrote something"
