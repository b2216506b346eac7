"""The integer parts of csrc/oard_pairwise.h as tests/_pairwise_cases.py restates them, without a device: the pair decode against
itertools, the group search over ragged tables, and the leader walk against the reference's de-duplication rule written out plainly."""
import itertools

import numpy as np

import _pairwise_cases as pc


def test_decode_is_the_upper_triangle_row_by_row():
    for K in range(0, 71):
        want = list(itertools.combinations(range(K), 2))
        assert len(want) == K * (K - 1) // 2
        got = [pc.decode(q, K) for q in range(len(want))]
        assert got == want, K


def test_decode_at_large_group_sizes():
    for K in (4096, 46341):
        total = K * (K - 1) // 2
        assert total < 2 ** 31                                  # 46341 is the largest K whose pairs fit the launch
        for q in (0, total - 1, total // 3, total // 2, total - K):
            i, j = pc.decode(q, K)
            assert 0 <= i < j < K
            assert pc.row_start(i, K) + (j - i - 1) == q
            assert pc.row_start(i, K) <= q < pc.row_start(i + 1, K)
        assert pc.decode(0, K) == (0, 1) and pc.decode(total - 1, K) == (K - 2, K - 1)
        # the first and last pair of rows deep in the triangle, where the square root cancels most
        for i in (1, K // 2, K - 3, K - 2):
            assert pc.decode(pc.row_start(i, K), K) == (i, i + 1)
            assert pc.decode(pc.row_start(i + 1, K) - 1, K) == (i, K - 1)


def test_group_search_over_ragged_tables_with_empty_groups():
    sizes = [3, 0, 1, 5, 0, 0, 2, 1, 8, 1, 0]
    group_ptr, pair_ptr, mat_ptr = pc.tables(sizes)
    want = [(g, i, j) for g, K in enumerate(sizes) for i, j in itertools.combinations(range(K), 2)]
    assert int(pair_ptr[-1]) == len(want) and int(mat_ptr[-1]) == sum(K * K for K in sizes)
    got = [pc.pair_of(p, group_ptr, pair_ptr) for p in range(len(want))]
    assert got == want
    # groups of 0 and 1 members first and last
    sizes = [0, 1, 4, 1, 0]
    group_ptr, pair_ptr, _ = pc.tables(sizes)
    assert [pc.pair_of(p, group_ptr, pair_ptr) for p in range(6)] == [(2, i, j) for i, j in itertools.combinations(range(4), 2)]


def _plain_rule(D, threshold, order):
    """demo.py:548-555 restated: a structure is new when its smallest RMSD to the structures kept so far exceeds the threshold.  The
    loop there only keeps or drops; which kept structure a dropped one belongs to is the one at that smallest RMSD (the first of equals)."""
    kept, label = [], {}
    for m in order:
        min_rmsd, at = 100, None
        for u in kept:
            rmsd = D[m, u]
            if rmsd < min_rmsd:                                 # min(min_rmsd, rmsd): a NaN never lowers it
                min_rmsd, at = rmsd, u
        if min_rmsd > threshold or at is None:
            kept.append(m)
            label[m] = m
        else:
            label[m] = at
    return np.array([label[m] for m in range(len(D))], np.int32), len(kept)


def _random_matrix(rng, K, threshold, nan_rows):
    centres = rng.integers(0, max(K // 3, 1), K)
    D = np.where(centres[:, None] == centres[None, :], 0.6 * threshold, 3.0 * threshold) * rng.uniform(0.5, 1.5, (K, K))
    D = np.float32(0.5) * (D + D.T).astype(np.float32)
    at = rng.random((K, K)) < 0.2                               # entries exactly at the threshold
    at = at | at.T
    D[at] = np.float32(threshold)
    for r in nan_rows:
        D[r, :] = np.nan
        D[:, r] = np.nan
    np.fill_diagonal(D, 0.0)
    return D


def test_leader_walk_is_the_reference_rule():
    rng = np.random.default_rng(3)
    thr = np.float32(0.1)
    for K in (0, 1, 2, 3, 7, 20, 64, 65):
        for trial in range(4):
            nan_rows = list(rng.choice(K, size=min(K, trial), replace=False)) if K else []
            D = _random_matrix(rng, K, thr, nan_rows)
            for order in (None, rng.permutation(K)):
                label, n = pc.leader_walk(D, thr, order)
                want, want_n = _plain_rule(D, thr, range(K) if order is None else order)
                assert n == want_n and (label == want).all(), (K, trial)
                for r in nan_rows:                              # a poisoned member ends up alone
                    assert label[r] == r and (np.delete(label, r) != r).all()


def test_leader_walk_ties_and_limit():
    thr = np.float32(0.1)
    D = np.array([[0, 1, thr, thr], [1, 0, thr, 0.05], [thr, thr, 0, 1], [thr, 0.05, 1, 0]], np.float32)
    label, n = pc.leader_walk(D, thr)
    assert n == 2 and label.tolist() == [0, 1, 0, 1]          # member 2: a tie at the threshold goes to leader 0; member 3: the nearer one
    label, n = pc.leader_walk(D, np.nextafter(thr, np.float32(0)))
    assert n == 3 and label.tolist() == [0, 1, 2, 1]          # just below: "close" is d <= threshold in float32
    big = np.zeros((pc.LEADER_MAX + 1, pc.LEADER_MAX + 1), np.float32)
    label, n = pc.leader_walk(big, thr)
    assert n == -1 and (label == -1).all()
