"""k_leader_cluster through the C ABI alone (`oard_leader_cluster`, include/oard.h) on matrices uploaded from the host: labels and counts
equal the host emulation of tests/_pairwise_cases.py exactly - the kernel does integer work and float compares only, so there is no
tolerance.  One launch holds every case; the group over the stated limit gets -1 throughout; the canaries stay."""
import functools

import numpy as np
import pytest
import torch

import _pairwise_cases as pc

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = -7
THRESHOLD = np.float32(0.1)


def _lib():
    from oareactdiff_amd import _capi
    return _capi, _capi.lib()


def _random(rng, K, nan_rows=0, at_threshold=0.2):
    """Blobs of members within 0.6 .. 0.9 of the threshold of each other, 3 x apart otherwise; a fifth of the entries EXACTLY at the
    threshold; `nan_rows` members whose row and column are NaN (their diagonal too, as a poisoned member's is)."""
    centres = rng.integers(0, max(K // 4, 1), K)
    D = np.where(centres[:, None] == centres[None, :], 0.75, 3.0) * THRESHOLD * rng.uniform(0.8, 1.2, (K, K))
    D = (0.5 * (D + D.T)).astype(np.float32)
    at = np.triu(rng.random((K, K)) < at_threshold)
    D[at | at.T] = THRESHOLD
    np.fill_diagonal(D, 0.0)
    for r in rng.choice(K, size=min(nan_rows, K), replace=False) if K else []:
        D[r, :] = np.nan
        D[:, r] = np.nan
    return D


@functools.lru_cache(maxsize=None)
def _cases():
    rng = np.random.default_rng(5)
    cases = []                                                  # (name, D, order or None)
    for K in (0, 1, 2, 64, 65, 130):
        D = _random(rng, K, nan_rows=min(K // 8, 5))
        cases.append((f"K{K}", D, None))
        cases.append((f"K{K}-order", D, rng.permutation(K).astype(np.int32)))
    cases.append(("identical", np.zeros((40, 40), np.float32), None))
    far = np.full((70, 70), 5.0, np.float32)
    np.fill_diagonal(far, 0.0)
    cases.append(("far", far, None))
    cases.append(("all-at-threshold", np.full((9, 9), THRESHOLD, np.float32), None))
    cases.append(("just-above", np.full((9, 9), np.nextafter(THRESHOLD, np.float32(1)), np.float32), None))
    cases.append(("all-nan", np.full((6, 6), np.nan, np.float32), None))
    cases.append(("over-limit", np.zeros((pc.LEADER_MAX + 1, pc.LEADER_MAX + 1), np.float32), None))
    cases.append(("at-limit", _random(rng, pc.LEADER_MAX, nan_rows=3, at_threshold=0.01), None))
    return cases


def _launch(cases, with_order):
    """One `oard_leader_cluster` call over `cases` -> (label per case, n_clusters per case).  with_order: the order array is passed (index
    order written out for the cases that have none)."""
    _capi, L = _lib()
    dev = torch.device("cuda:0")
    sizes = [len(D) for _, D, _ in cases]
    group_ptr, _, mat_ptr = pc.tables(sizes)
    G, M, T = len(cases), int(group_ptr[-1]), int(mat_ptr[-1])
    dist = torch.from_numpy(np.concatenate([D.reshape(-1) for _, D, _ in cases] + [np.zeros(1, np.float32)])).to(dev)
    order = np.concatenate([np.arange(len(D), dtype=np.int32) if o is None else o for _, D, o in cases] + [np.zeros(1, np.int32)])
    d_order = torch.from_numpy(order).to(dev)
    d_gp, d_mp = torch.from_numpy(group_ptr.astype(np.int32)).to(dev), torch.from_numpy(mat_ptr).to(dev)
    label = torch.full((GUARD + M + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    count = torch.full((GUARD + G + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.oard_leader_cluster(dist.data_ptr(), d_mp.data_ptr(), d_gp.data_ptr(), d_order.data_ptr() if with_order else None, G,
                                   float(THRESHOLD), label[GUARD:].data_ptr(), count[GUARD:].data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    for t, n in ((label, M), (count, G)):
        assert bool((t[:GUARD] == SENTINEL).all()) and bool((t[GUARD + n:] == SENTINEL).all()), "a canary was written"
    lab, cnt = label[GUARD: GUARD + M].cpu().numpy(), count[GUARD: GUARD + G].cpu().numpy()
    return [lab[group_ptr[g]: group_ptr[g + 1]] for g in range(G)], cnt


@functools.lru_cache(maxsize=None)
def _expected():
    return [pc.leader_walk(D, THRESHOLD, o) for _, D, o in _cases()]


def test_labels_and_counts_equal_the_host_emulation():
    cases = _cases()
    lab, cnt = _launch(cases, with_order=True)
    for (name, D, o), got, n, (want, want_n) in zip(cases, lab, cnt, _expected()):
        assert n == want_n and (got == want).all(), name
    by = {c[0]: g for g, c in enumerate(cases)}
    assert cnt[by["identical"]] == 1 and (lab[by["identical"]] == 0).all()
    assert cnt[by["far"]] == 70 and (lab[by["far"]] == np.arange(70)).all()
    assert cnt[by["all-at-threshold"]] == 1 and cnt[by["just-above"]] == 9 and cnt[by["all-nan"]] == 6
    assert cnt[by["over-limit"]] == -1 and (lab[by["over-limit"]] == -1).all()
    assert cnt[by["at-limit"]] > 0 and (lab[by["at-limit"]] >= 0).all()
    assert cnt[by["K0"]] == 0 and cnt[by["K1"]] == 1


def test_null_order_is_index_order_and_groups_are_independent():
    cases = [c for c in _cases() if c[2] is None and len(c[1]) <= 130]
    want = [pc.leader_walk(D, THRESHOLD) for _, D, _ in cases]
    lab, cnt = _launch(cases, with_order=False)
    for (name, _, _), got, n, (w, wn) in zip(cases, lab, cnt, want):
        assert n == wn and (got == w).all(), name
    for g in (3, len(cases) - 1):                               # a group launched alone: the same labels
        one, c1 = _launch([cases[g]], with_order=False)
        assert c1[0] == cnt[g] and (one[0] == lab[g]).all()
