"""The formulas of k_kabsch_rmsd (csrc/oard_kabsch.h) pinned on the host: a numpy emulation of its algorithm - Horn's quaternion matrix of
the cross-covariance, cyclic Jacobi, the residual pass, the mirror image through the sign of S's last row - against the SVD reference
the GPU tests use, on every size and kind of tests/test_kabsch_kernel.py and both flag settings.  Never loads the library."""
import numpy as np
import pytest

import _kabsch_cases as kc


@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("kind", kc.KINDS)
def test_horn_jacobi_residual_matches_the_svd_reference(kind, reflect):
    a, b = kc.make_kind(kind)
    p = kc.seg_ptr(kc.SIZES)
    worst = 0.0
    for g, n in enumerate(kc.SIZES):
        if n == 0:
            continue
        sa, sb = a[p[g]: p[g + 1]], b[p[g]: p[g + 1]]
        r, rho = kc.svd_rmsd(sa, sb, reflect)
        k, M = kc.emulate(sa, sb, reflect)
        worst = max(worst, abs(k - r) / rho if rho > 0 else abs(k - r))       # n = 1: rho = 0 and both are exactly 0
        assert abs(k - r) <= 1e-10 * rho, (kind, n, k, r)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-12
        if not reflect:
            assert abs(np.linalg.det(M) - 1.0) <= 1e-12
    print(f"{kind}, reflect={reflect}: worst |emulation - reference| / rho = {worst:.1e}")


def test_the_mirror_image_is_found_with_an_improper_map():
    a, b = kc.make_kind("mirror")
    p = kc.seg_ptr(kc.SIZES)
    for g, n in enumerate(kc.SIZES):
        if n < 4:
            continue
        sa, sb = a[p[g]: p[g + 1]], b[p[g]: p[g + 1]]
        k0, M0 = kc.emulate(sa, sb, False)
        k1, M1 = kc.emulate(sa, sb, True)
        assert np.linalg.det(M0) > 0 and np.linalg.det(M1) < 0
        assert k1 <= 1e-6 < k0                     # float32 inputs: the mirror image fits to rounding, the rotation alone does not
        # the map takes centred b onto centred a
        y, x = sb.astype(np.float64) - sb.astype(np.float64).mean(0), sa.astype(np.float64) - sa.astype(np.float64).mean(0)
        assert np.abs(y @ M1.T - x).max() <= 1e-5


def test_reference_agrees_with_a_brute_force_search_on_a_small_case():
    """The SVD reference itself: no rotation from a dense random sample beats it, and it beats most of them."""
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((7, 3)), rng.standard_normal((7, 3))
    r, _ = kc.svd_rmsd(a, b, False)
    x, y = a - a.mean(0), b - b.mean(0)
    tried = [np.sqrt(np.sum((y @ kc.random_rotation(rng).T - x) ** 2) / 7) for _ in range(2000)]
    assert r <= min(tried) + 1e-12
