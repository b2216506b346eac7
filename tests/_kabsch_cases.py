"""Shared by the Kabsch-RMSD tests: the float64 reference (a DIFFERENT algorithm from the kernel's: SVD of the covariance with the
determinant correction, then the residual), the input kinds, the per-segment gate and - for the host-side test - a numpy emulation of
the kernel's own algorithm (Horn's quaternion matrix, cyclic Jacobi, residual pass)."""
import numpy as np

SIZES = [1, 2, 3, 4, 23, 0, 63, 64, 65, 129, 1024]          # one launch: an empty segment in the middle
KINDS = ["independent", "identical", "rigid", "rigid_noise", "mirror", "collinear", "coplanar", "offset"]
DEGENERATE = {"identical", "collinear", "coplanar"}


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_kind(kind, sizes=SIZES, seed=0):
    """-> (a, b) float32 [sum(sizes), 3], segment after segment."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    A, B = [], []
    for n in sizes:
        a = 1.5 * rng.standard_normal((n, 3))
        if kind == "independent":
            b = 1.5 * rng.standard_normal((n, 3))
        elif kind == "identical":
            b = a.copy()
        elif kind in ("rigid", "rigid_noise"):
            b = a @ random_rotation(rng).T + rng.standard_normal(3) * 3.0
            if kind == "rigid_noise":
                b = b + 0.05 * rng.standard_normal((n, 3))
        elif kind == "mirror":
            b = (a * np.array([1.0, 1.0, -1.0])) @ random_rotation(rng).T
        elif kind == "collinear":
            a = np.outer(1.5 * rng.standard_normal(n), random_rotation(rng)[0]) + rng.standard_normal(3)
            b = np.outer(1.5 * rng.standard_normal(n), random_rotation(rng)[0]) + rng.standard_normal(3)
        elif kind == "coplanar":
            a[:, 2] = 0.0
            a = a @ random_rotation(rng).T
            b = 1.5 * rng.standard_normal((n, 3))
            b[:, 2] = 0.0
            b = b @ random_rotation(rng).T + rng.standard_normal(3)
        elif kind == "offset":
            b = 1.5 * rng.standard_normal((n, 3)) - 40.0
            a = a + 60.0
        else:
            raise KeyError(kind)
        A.append(a)
        B.append(b)
    return np.concatenate(A).astype(np.float32), np.concatenate(B).astype(np.float32)


def seg_ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _svd_fit(x, y):
    """Centred float64 x (target), y: the proper rotation R minimising |R y - x| (Kabsch, determinant corrected) and the residual RMSD."""
    u, _, vt = np.linalg.svd(y.T @ x)                       # H = sum y x^T = U S V^T;  R = V diag(1, 1, d) U^T
    d = np.sign(np.linalg.det(vt.T @ u.T))
    d = 1.0 if d == 0 else d
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    return r, float(np.sqrt(np.sum((y @ r.T - x) ** 2) / len(x)))


def svd_rmsd(a, b, reflect):
    """float64 reference of one segment -> (rmsd, rho); rho = sqrt((G_a + G_b) / (2 n)), the scale of the gate's second term."""
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    if len(a) == 0:
        return float("nan"), float("nan")
    x, y = a - a.mean(0), b - b.mean(0)
    r = _svd_fit(x, y)[1]
    if reflect:
        r = min(r, _svd_fit(x, y * np.array([1.0, 1.0, -1.0]))[1])
    return r, float(np.sqrt((np.sum(x * x) + np.sum(y * y)) / (2 * len(a))))


def reference(a, b, sizes, reflect):
    p = seg_ptr(sizes)
    out = [svd_rmsd(a[p[g]: p[g + 1]], b[p[g]: p[g + 1]], reflect) for g in range(len(sizes))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def gate(r, rho):
    """|k - r| <= 2^-23 r + 1e-10 rho: one rounding of the float32 output, then the float64 arithmetic (a different summation order at
    n = 1024 and an offset of 60 stays five orders below it)."""
    return 2.0 ** -23 * r + 1e-10 * rho


# ---- the kernel's algorithm in numpy (host-side test of the formulas; never loads the library) ---------------------------------------
def _jacobi_max_eigvec(N, sweeps=10):
    A, V = N.copy(), np.eye(4)
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            apq = A[p, q]
            if apq == 0.0:
                continue
            with np.errstate(over="ignore", divide="ignore"):
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = np.copysign(1.0, theta) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            J = np.eye(4)
            J[p, p] = J[q, q] = c
            J[p, q], J[q, p] = s, -s
            A = J.T @ A @ J
            V = V @ J
    return V[:, int(np.argmax(np.diag(A)))]


def horn_rotation(S):
    """S[i][j] = sum y_i x_j (centred y = b, x = a) -> R with R y ~ x."""
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    q = _jacobi_max_eigvec(N)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def emulate(a, b, reflect):
    """One segment as the kernel computes it -> (rmsd, map on centred b)."""
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    x, y = a - a.mean(0), b - b.mean(0)
    S = y.T @ x
    best, M = None, None
    for sz in ((1.0, -1.0) if reflect else (1.0,)):
        Sm = S.copy()
        Sm[2] *= sz
        R = horn_rotation(Sm)
        R[:, 2] *= sz
        e = float(np.sqrt(np.sum((y @ R.T - x) ** 2) / len(a)))
        if best is None or e < best:
            best, M = e, R
    return best, M
