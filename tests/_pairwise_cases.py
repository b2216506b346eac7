"""Shared by the pairwise-RMSD and leader-clustering tests: numpy emulations of the integer parts of csrc/oard_pairwise.h (the pair
decode and the group search, integer for integer; the leader walk) and the planted-cluster inputs of the end-to-end test.  Never loads
the library."""
import math

import numpy as np

from _kabsch_cases import random_rotation

# ---- the pair decode (pair_row_start, pair_decode, pair_find_group of csrc/oard_pairwise.h) ------------------------------------------------


def row_start(i, K):
    """Pairs before row i of a K x K upper triangle."""
    return i * (2 * K - i - 1) // 2


def decode(q, K):
    """q in [0, K (K - 1) / 2) -> (i, j), i < j: the square root proposes, the two integer loops decide."""
    b = float(2 * K - 1)
    disc = max(b * b - 8.0 * float(q), 0.0)
    i = int((b - math.sqrt(disc)) * 0.5)
    i = min(max(i, 0), K - 2)
    while i > 0 and row_start(i, K) > q:
        i -= 1
    while i < K - 2 and row_start(i + 1, K) <= q:
        i += 1
    return i, i + 1 + (q - row_start(i, K))


def find_group(ptr, v):
    """The largest g in [0, G) with ptr[g] <= v (ptr ascending, G + 1 entries, G >= 1): the kernel's binary search."""
    lo, hi = 0, len(ptr) - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if ptr[mid] <= v:
            lo = mid
        else:
            hi = mid
    return lo


def tables(sizes):
    """Group sizes K_g -> (group_ptr, pair_ptr, mat_ptr) as int64 arrays of G + 1 entries."""
    k = np.asarray(sizes, np.int64)
    z = np.zeros(1, np.int64)
    return (np.concatenate([z, np.cumsum(k)]), np.concatenate([z, np.cumsum(k * (k - 1) // 2)]), np.concatenate([z, np.cumsum(k * k)]))


def pair_of(p, group_ptr, pair_ptr):
    """Pair index p of a launch -> (g, i, j), or None where the kernel writes nothing."""
    g = find_group(pair_ptr, p)
    K = int(group_ptr[g + 1] - group_ptr[g])
    q = int(p - pair_ptr[g])
    if K < 2 or q < 0 or q >= K * (K - 1) // 2:
        return None
    return (g,) + decode(q, K)


# ---- the leader walk (k_leader_cluster) -------------------------------------------------------------------------------------------------
LEADER_MAX = 1024


def leader_walk(D, threshold, order=None):
    """D [K, K] float32, threshold -> (label [K] int32, n_clusters): the kernel's rule with its float32 compares.  More than LEADER_MAX
    members: -1 throughout."""
    D = np.asarray(D, np.float32)
    K = len(D)
    thr = np.float32(threshold)
    label = np.full(K, -1, np.int32)
    if K > LEADER_MAX:
        return label, -1
    leaders = []
    for t in range(K):
        m = t if order is None else int(order[t])
        if m < 0 or m >= K:
            continue
        best, bl = None, None
        for l, lead in enumerate(leaders):
            d = D[m, lead]
            if d <= thr and (bl is None or d < best):
                best, bl = d, l
        if bl is None:
            leaders.append(m)
            label[m] = m
        else:
            label[m] = leaders[bl]
    return label, len(leaders)


# ---- planted clusters (tests/test_distinct_candidates.py) ---------------------------------------------------------------------------------
PLANT_COUNTS = (2, 1, 1, 5)           # 2! 1! 1! 5! = 240 species-preserving permutations: the exact branch
PLANT_LABELS = (6, 7, 8, 1)
PLANT_BASES = [0, 1, 2, 0, 1, 0, 2, 0]
PLANT_SIGMA = 0.005


def planted(seed=20, bases=PLANT_BASES, m=3):
    """K = len(bases) candidates of one reaction: m base conformers of 9 atoms drawn N(0, 1.5^2); candidate k is base bases[k] with like
    atoms shuffled, every second candidate z-mirrored, a random rotation and translation, jitter of sigma 0.005, rounded to float32.
    -> (pos [K, 9, 3] float32, species [K, 9] int32)."""
    rng = np.random.default_rng(seed)
    n = int(sum(PLANT_COUNTS))
    sp0 = np.repeat(np.array(PLANT_LABELS), PLANT_COUNTS)
    conf = 1.5 * rng.standard_normal((m, n, 3))
    pos, species = [], []
    for k, b in enumerate(bases):
        perm = np.arange(n)
        for s in np.unique(sp0):
            idx = np.where(sp0 == s)[0]
            perm[idx] = idx[rng.permutation(len(idx))]
        c = conf[b][perm]
        if k % 2:
            c = c * np.array([1.0, 1.0, -1.0])
        c = c @ random_rotation(rng).T + 3.0 * rng.standard_normal(3) + PLANT_SIGMA * rng.standard_normal((n, 3))
        pos.append(c.astype(np.float32))
        species.append(sp0[perm].astype(np.int32))
    return np.stack(pos), np.stack(species)
