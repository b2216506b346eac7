"""Shared by the order-matched-RMSD tests: the two float64 yardsticks and the case builders.

`brute` is the yardstick of the kernel's exact branch: every species-preserving permutation, each fitted by the SVD Kabsch of
tests/_kabsch_cases.py (a different algorithm from the kernel's quaternion / Jacobi ranking).  `search` is the yardstick of its search
branch: the same alternation of assignment and superposition from the same five starts per chirality, with scipy's
`linear_sum_assignment` and the SVD fit in place of the kernel's shortest-augmenting-path solver and Horn's matrix."""
import itertools

import numpy as np

from _kabsch_cases import _svd_fit, random_rotation

ROUNDS = 32
MIRROR = np.array([1.0, 1.0, -1.0])
KINDS = ["independent", "rigid", "rigid_noise", "mirror"]              # generic random clouds: parity is asked
DEGENERATE = ["identical", "collinear", "coplanar"]                    # axes / assignments not unique: properties only
PLANTED = {"rigid", "rigid_noise", "mirror"}                           # b is a (noisy, mirrored) copy of a under a known permutation
LABELS = (6, 1, 7, 8, 9, 16)                                           # species labels, in the order the counts are given

# name -> species counts; one launch holds them all, in this order
EXACT = [("n1", (1,)), ("n2", (2,)), ("distinct6", (1, 1, 1, 1, 1, 1)), ("c332", (3, 3, 2)), ("c431", (4, 3, 1)), ("c52", (5, 2)),
         ("c7", (7,)), ("empty", ()), ("mismatch", (3, 2))]
SEARCH = [("c8", (8,)), ("c12", (12,)), ("mol23", (7, 12, 2, 2)), ("n63", (20, 30, 8, 5)), ("n64", (64,)), ("n65", (65,)),
          ("n256", (100, 120, 20, 16)), ("n257", (257,))]
SEGMENTS = EXACT + SEARCH
NAMES = [s[0] for s in SEGMENTS]
SIZES = [int(sum(s[1])) for s in SEGMENTS]
STATUS = {"mismatch": 2, "n257": 3, **{n: 0 for n, _ in EXACT if n != "mismatch"}, **{n: 1 for n, _ in SEARCH if n != "n257"}}
NO_REFERENCE = {"empty", "mismatch", "n257"}


def blocks(sp):
    return [np.where(sp == s)[0] for s in np.unique(sp)]


def assign(x, yr, sp):
    """perm with perm[i] the row of yr matched to row i of x: the minimum of sum |x_i - yr_perm[i]|^2 per species block."""
    from scipy.optimize import linear_sum_assignment
    perm = np.arange(len(x))
    for idx in blocks(sp):
        cost = ((x[idx][:, None, :] - yr[idx][None, :, :]) ** 2).sum(-1)
        r, c = linear_sum_assignment(cost)
        perm[idx[r]] = idx[c]
    return perm


def axes(x):
    """Principal axes of a centred cloud: eigenvectors by ascending eigenvalue, made proper."""
    _, v = np.linalg.eigh(x.T @ x)
    if np.linalg.det(v) < 0:
        v[:, 2] = -v[:, 2]
    return v


def _centred(a, b):
    a, b = np.asarray(a, np.float64)[:, :3], np.asarray(b, np.float64)[:, :3]
    return a - a.mean(0), b - b.mean(0)


def search(a, b, sp, reflect=True, rounds=ROUNDS):
    """-> (rmsd, perm, most rounds any run used).  Rows of a and b carry the same species `sp` row by row."""
    x, y0 = _centred(a, b)
    best, bestp, most = np.inf, None, 0
    for sz in ((1.0, -1.0) if reflect else (1.0,)):
        y = y0 * np.array([1.0, 1.0, sz])
        va, vb = axes(x), axes(y)
        starts = [_svd_fit(x, y)[0]] + [va @ np.diag(s) @ vb.T for s in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
        for rot in starts:
            prev = None
            for it in range(rounds):
                p = assign(x, y @ rot.T, sp)
                if prev is not None and (p == prev).all():
                    break
                prev = p
                rot, e = _svd_fit(x, y[p])
                most = max(most, it + 1)
            if e < best:
                best, bestp = e, prev
    return best, bestp, most


def brute(a, b, sp, reflect=True):
    """-> (rmsd, perm): the minimum over every species-preserving permutation (and the mirror image), each by the SVD fit; batched."""
    x, y0 = _centred(a, b)
    groups = blocks(sp)
    perms = []
    for combo in itertools.product(*[itertools.permutations(g) for g in groups]):
        p = np.arange(len(x))
        for g, c in zip(groups, combo):
            p[g] = c
        perms.append(p)
    perms = np.array(perms)
    best, bestp = np.inf, None
    for sz in ((1.0, -1.0) if reflect else (1.0,)):
        y = (y0 * np.array([1.0, 1.0, sz]))[perms]                     # [N, n, 3]
        u, _, vt = np.linalg.svd(np.einsum("pki,kj->pij", y, x))        # H = sum y x^T = U S V^T;  R = V diag(1, 1, d) U^T
        v, ut = np.swapaxes(vt, 1, 2), np.swapaxes(u, 1, 2)
        d = np.sign(np.linalg.det(v @ ut))
        d[d == 0] = 1.0
        v[:, :, 2] *= d[:, None]
        rot = v @ ut
        e = np.sqrt(((np.einsum("pij,pkj->pki", rot, y) - x) ** 2).sum((1, 2)) / len(x))
        k = int(np.argmin(e))
        if e[k] < best:
            best, bestp = float(e[k]), perms[k]
    return best, bestp


def same_order(a, b, reflect=True):
    x, y = _centred(a, b)
    r = _svd_fit(x, y)[1]
    return min(r, _svd_fit(x, y * MIRROR)[1]) if reflect else r


def rho(a, b):
    x, y = _centred(a, b)
    return float(np.sqrt((np.sum(x * x) + np.sum(y * y)) / (2 * len(x))))


def make_segment(kind, counts, rng):
    """-> a, b float32 [n, 3], sp int32 [n] (species of row k of a AND of b), planted int64 [n] (b[planted[k]] belongs to a[k])."""
    n = int(sum(counts))
    sp = np.repeat(np.array(LABELS[:len(counts)]), counts)
    sp = sp[rng.permutation(n)]                                        # species interleaved over the rows
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
        b = (a * MIRROR) @ random_rotation(rng).T + rng.standard_normal(3)
    elif kind == "collinear":
        a = np.outer(1.5 * rng.standard_normal(n), random_rotation(rng)[0]) + rng.standard_normal(3)
        b = np.outer(1.5 * rng.standard_normal(n), random_rotation(rng)[0]) + rng.standard_normal(3)
    elif kind == "coplanar":
        a[:, 2] = 0.0
        a = a @ random_rotation(rng).T
        b = 1.5 * rng.standard_normal((n, 3))
        b[:, 2] = 0.0
        b = b @ random_rotation(rng).T + rng.standard_normal(3)
    else:
        raise KeyError(kind)
    planted = np.arange(n)
    for idx in blocks(sp):
        planted[idx] = idx[rng.permutation(len(idx))]
    shuffled = np.empty_like(b)
    shuffled[planted] = b
    return a.astype(np.float32), shuffled.astype(np.float32), sp.astype(np.int32), planted


def make_kind(kind, segments=SEGMENTS, seed=0):
    """One launch: -> dict(a, b [N, 3] float32; sp_a, sp_b [N] int32; sizes; planted: per segment).  The species of b differ from a's
    in the segment called `mismatch` only (one row of b gets another segment-internal label: equal counts no more)."""
    rng = np.random.default_rng([seed, (KINDS + DEGENERATE).index(kind)])
    A, B, SA, SB, P = [], [], [], [], []
    for name, counts in segments:
        a, b, sp, planted = make_segment(kind, counts, rng)
        sb = sp.copy()
        if name == "mismatch":
            k = int(np.where(sp == LABELS[0])[0][0])
            sb[k] = LABELS[1]
        A.append(a), B.append(b), SA.append(sp), SB.append(sb), P.append(planted)
    return dict(a=np.concatenate(A), b=np.concatenate(B), sp_a=np.concatenate(SA), sp_b=np.concatenate(SB),
                sizes=[int(sum(c)) for _, c in segments], planted=P)


def segment(case, g):
    p = np.concatenate([[0], np.cumsum(case["sizes"])])
    s = slice(int(p[g]), int(p[g + 1]))
    return case["a"][s], case["b"][s], case["sp_a"][s], case["planted"][g]


def planted_rmsd(a, b, planted, reflect):
    """The RMSD of the planted permutation: what a matcher that finds it (or better) returns at most."""
    return same_order(a, b[planted], reflect)
