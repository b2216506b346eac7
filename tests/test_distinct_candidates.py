"""The Python layer end to end on planted clusters (tests/_pairwise_cases.planted): `metrics.pairwise_rmsd`, `metrics.leader_clusters`
and `confidence.distinct_candidates`.  K = 8 candidates of a reaction are noisy, shuffled, rotated, partly mirrored copies of 3 base
conformers; the float64 references of the repository place every matched RMSD inside a cluster below threshold / 4 and every one
across clusters (and every same-order one) above 4 x threshold, so no rounding in a kernel can move an entry across the threshold: the
clustering is then fixed exactly - 3 clusters partitioned by base, each led by its best-scored member -, and without the matching
there are 8.  Two reactions run candidate-major in one call; each equals that reaction alone."""
import functools

import numpy as np
import pytest
import torch

import _match_cases as mc
import _pairwise_cases as pc

THRESHOLD = 0.1
SEEDS = (20, 21)                                              # reaction r is planted(SEEDS[r])
K = len(pc.PLANT_BASES)
# distinct scores; reaction 0: the best of base 0 is candidate 5, of base 1 candidate 4, of base 2 candidate 6
SCORES = np.array([[0.10, 0.30, 0.20, 0.50, 0.90, 0.95, 0.40, 0.05],
                   [0.70, 0.15, 0.25, 0.35, 0.05, 0.45, 0.85, 0.55]], np.float32)


@functools.lru_cache(maxsize=None)
def _reaction(r):
    return pc.planted(SEEDS[r])


def _inputs(reactions, dev):
    """Candidate-major: segment k * R + r is candidate k of reaction reactions[r] -> (scores [K R], x [n, 5] with the species as the last
    column, sizes [K R])."""
    R = len(reactions)
    rows, scores = [], []
    for k in range(K):
        for r in reactions:
            pos, sp = _reaction(r)
            rows.append(np.concatenate([pos[k], np.full((len(pos[k]), 1), 7.5, np.float32), sp[k][:, None].astype(np.float32) + 0.25], 1))
            scores.append(SCORES[r, k])
    x = torch.from_numpy(np.concatenate(rows)).to(dev)
    return torch.tensor(scores, device=dev), x, torch.full((K * R,), rows[0].shape[0], dtype=torch.int64, device=dev)


def test_preconditions_on_the_planted_inputs():
    """No GPU: the margins that make the clustering exact, from the float64 references alone."""
    for r in range(len(SEEDS)):
        pos, sp = _reaction(r)
        intra, inter, same_intra = 0.0, np.inf, np.inf
        for i in range(K):
            for j in range(i + 1, K):
                assert (sp[i] == sp[j]).all()
                m = mc.brute(pos[i], pos[j], sp[i], True)[0]
                if pc.PLANT_BASES[i] == pc.PLANT_BASES[j]:
                    intra, same_intra = max(intra, m), min(same_intra, mc.same_order(pos[i], pos[j], True))
                else:
                    inter = min(inter, m)
        print(f"reaction {r}: intra {intra:.4f} inter {inter:.3f} same-order intra {same_intra:.3f}")
        assert intra <= THRESHOLD / 4 and inter >= 4 * THRESHOLD and same_intra >= 4 * THRESHOLD


def _check_reaction(res, row, r):
    bases = np.array(pc.PLANT_BASES)
    label, leader, order = res.label[row].cpu().numpy(), res.is_leader[row].cpu().numpy(), res.order[row].cpu().numpy()
    assert int(res.n_clusters[row]) == 3
    for b in range(3):
        members = np.where(bases == b)[0]
        best = members[np.argmax(SCORES[r, members])]
        assert (label[members] == best).all(), (r, b, label)   # one label per base, and it is the base's best-scored member
    assert leader.sum() == 3 and (leader == (label == np.arange(K))).all()
    assert (order == np.argsort(-SCORES[r], kind="stable")).all()
    distinct = order[leader[order]]                             # "the distinct structures, best first"
    assert len(distinct) == 3 and sorted(bases[distinct]) == [0, 1, 2] and (np.diff(SCORES[r, distinct]) < 0).all()


@pytest.mark.gpu
def test_planted_clusters_two_reactions_and_each_alone():
    from oareactdiff_amd.confidence import distinct_candidates
    dev = torch.device("cuda:0")
    scores, x, sizes = _inputs((0, 1), dev)
    both = distinct_candidates(scores, x, sizes, 2, threshold=THRESHOLD)
    assert both.label.shape == (2, K) and both.is_leader.dtype == torch.bool and both.n_clusters.shape == (2,)
    assert bool((both.is_leader.sum(1) == both.n_clusters).all())
    for r in (0, 1):
        _check_reaction(both, r, r)
        alone = distinct_candidates(*_inputs((r,), dev), 1, threshold=THRESHOLD)
        _check_reaction(alone, 0, r)
        for f in ("label", "is_leader", "n_clusters", "order"):
            assert torch.equal(getattr(alone, f)[0], getattr(both, f)[r]), (r, f)
    # without the matching every candidate stands alone: the matching is what does the work
    plain = distinct_candidates(scores, x, sizes, 2, threshold=THRESHOLD, match_order=False)
    assert plain.n_clusters.tolist() == [K, K] and bool(plain.is_leader.all())
    assert torch.equal(plain.label, torch.arange(K, device=dev).expand(2, K))


@pytest.mark.gpu
def test_pairwise_rmsd_result_object_and_leader_clusters():
    from oareactdiff_amd import metrics
    dev = torch.device("cuda:0")
    _, x, sizes = _inputs((0, 1), dev)
    groups = metrics.candidate_groups(2, K)
    assert groups[1] == [1, 3, 5, 7, 9, 11, 13, 15]
    res = metrics.pairwise_rmsd(x, sizes, groups, species=x[:, -1], match_order=True, return_status=True)
    assert res.flat.shape == (2 * K * K,) and res.group_ptr == (0, K, 2 * K) and res.mat_ptr == (0, K * K, 2 * K * K)
    stacked = res.stacked()
    assert stacked.shape == (2, K, K) and stacked.data_ptr() == res.flat.data_ptr() and res.matrix(1).data_ptr() == stacked[1].data_ptr()
    assert torch.equal(stacked, stacked.transpose(1, 2)) and bool((stacked.diagonal(dim1=1, dim2=2) == 0).all())
    assert bool((res.status == metrics.MATCH_EXACT).all())
    # entry [i, j] is matched_rmsd of member i against member j, bit for bit (explicit copies)
    n = int(sizes[0])
    seg = lambda s: x[s * n: (s + 1) * n]
    for g, i, j in ((0, 0, 3), (1, 2, 6), (1, 7, 1)):
        a, b = seg(groups[g][i]), seg(groups[g][j])
        one = metrics.matched_rmsd(a, b, [n], a[:, -1], b[:, -1]) if i < j else metrics.matched_rmsd(b, a, [n], b[:, -1], a[:, -1])
        assert torch.equal(one.view(torch.int32), stacked[g, i, j].reshape(1).view(torch.int32))
    bases = np.array(pc.PLANT_BASES)
    same = torch.from_numpy(bases[:, None] == bases[None, :]).to(dev)
    assert bool((stacked[:, same] <= THRESHOLD / 4 * 1.01).all()) and bool((stacked[:, ~same] >= 4 * THRESHOLD * 0.99).all())
    # index order: the first member of every base leads it
    label, n_clusters = metrics.leader_clusters(res, THRESHOLD)
    assert label.shape == (2 * K,) and n_clusters.tolist() == [3, 3]
    first = np.array([pc.PLANT_BASES.index(b) for b in pc.PLANT_BASES])
    assert label.cpu().numpy().reshape(2, K).tolist() == [first.tolist(), first.tolist()]
    label2, n2 = metrics.leader_clusters(stacked, THRESHOLD)   # a plain [G, K, K] tensor
    assert torch.equal(label2, label) and torch.equal(n2, n_clusters)
    # ragged groups, an empty one among them
    ragged = metrics.pairwise_rmsd(x, sizes, [[0, 2, 4], [], [1], [3, 5]], return_status=True)
    assert ragged.group_ptr == (0, 3, 3, 4, 6) and ragged.mat_ptr == (0, 9, 9, 10, 14) and ragged.matrix(1).shape == (0, 0)
    assert float(ragged.matrix(2)) == 0.0 and ragged.matrix(3).shape == (2, 2)
    with pytest.raises(ValueError):
        ragged.stacked()
    assert metrics.leader_clusters(ragged, THRESHOLD)[1].tolist() == [3, 0, 1, 2]


@pytest.mark.gpu
def test_argument_errors_on_the_device():
    from oareactdiff_amd import metrics
    from oareactdiff_amd.confidence import distinct_candidates
    dev = torch.device("cuda:0")
    scores, x, sizes = _inputs((0, 1), dev)
    with pytest.raises(ValueError):
        metrics.pairwise_rmsd(x, sizes, torch.tensor(metrics.candidate_groups(2, K), device=dev))
    with pytest.raises(ValueError):
        distinct_candidates(scores[:-1], x, sizes, 2)
    with pytest.raises(ValueError):
        metrics.pairwise_rmsd(x, sizes, [[0, 2 * K]])


def test_argument_errors_without_a_device():
    from oareactdiff_amd import _capi, metrics
    from oareactdiff_amd.confidence import distinct_candidates
    scores, x, sizes = _inputs((0, 1), torch.device("cpu"))
    with pytest.raises(_capi.OardError):
        distinct_candidates(scores, x, sizes, 2)
    with pytest.raises(_capi.OardError):
        metrics.pairwise_rmsd(x, sizes, metrics.candidate_groups(2, K))
    with pytest.raises(_capi.OardError):
        metrics.leader_clusters(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError):
        distinct_candidates(scores[:-1], x, sizes, 2)
    with pytest.raises(ValueError):
        metrics.leader_clusters(torch.zeros(1, 4, 4), threshold=float("nan"))
    assert metrics.candidate_groups(3, 2) == [[0, 3], [1, 4], [2, 5]]
