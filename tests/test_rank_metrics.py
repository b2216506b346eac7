"""The Python layer over `oard_rank_metrics`: `metrics.rank_metrics`, `midrank`, the three selectors, and `confidence.ranking_report`,
against the float64 references of tests/_rank_cases.py."""
import numpy as np
import pytest
import torch

import _rank_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [5, 0, 70, 1, 130]
KIND = "quantised-real"


def _case():
    s, t = rc.make_kind(KIND)
    n = sum(SIZES) + 3                                   # three rows in no segment
    return s[:n].copy(), t[:n].copy()


def _check(m, ref, what):
    got = np.stack([x.cpu().numpy() for x in m], axis=1)
    assert all(x.dtype == torch.float64 and x.device.type == "cuda" for x in m)
    e = rc.check_table(got, ref, what)
    print(f"{what}: worst |auroc - pairs| {e[0]:.2e}; worst float64 column gap {e[1]:.2e}")


@pytest.mark.parametrize("sizes_on", ["host", "device"])
def test_rank_metrics_midrank_and_selectors(sizes_on):
    from oareactdiff_amd import binary_auroc, midrank, pearson_corrcoef, rank_metrics, spearman_corrcoef
    s, t = _case()
    ref_rs, ref_rt, ref = rc.reference(s, t, SIZES)
    ds, dt = torch.from_numpy(s).to(DEV), torch.from_numpy(t).to(DEV)
    sizes = SIZES if sizes_on == "host" else torch.tensor(SIZES, device=DEV)
    m = rank_metrics(ds, dt, sizes)
    assert m._fields == ("n", "n_pos", "auroc", "pearson", "spearman", "mae", "mean_score", "mean_target")
    _check(m, ref, f"sizes on the {sizes_on}")
    r = midrank(ds, sizes)
    assert r.dtype == torch.float64 and np.array_equal(r.cpu().numpy(), ref_rs, equal_nan=True) and bool(torch.isnan(r[-3:]).all())
    assert np.array_equal(midrank(dt, sizes).cpu().numpy(), ref_rt, equal_nan=True)
    for sel, col in ((binary_auroc, m.auroc), (pearson_corrcoef, m.pearson), (spearman_corrcoef, m.spearman)):
        got = sel(ds, dt, sizes)
        assert np.array_equal(got.cpu().numpy().view(np.int64), col.cpu().numpy().view(np.int64))      # NaN bits included


def test_converted_inputs_and_one_segment_of_everything():
    from oareactdiff_amd import midrank, rank_metrics
    s, t = _case()
    n = len(s)
    ref = rc.reference(s, t, [n])
    wide = torch.full((n, 3), float("nan"), device=DEV)
    wide[:, 1] = torch.from_numpy(s).to(DEV)
    view = wide[:, 1]
    assert not view.is_contiguous()
    t64 = torch.from_numpy(t).to(DEV).double()
    _check(rank_metrics(view, t64), ref[2], "a strided view and a float64 tensor, sizes=None")
    assert np.array_equal(midrank(view).cpu().numpy(), ref[0])
    assert bool(torch.isnan(wide[:, [0, 2]]).all())
    # an empty list of sizes: no segment, every rank NaN; no rows at all: one empty segment
    assert bool(torch.isnan(midrank(view, [])).all()) and rank_metrics(view, t64, []).n.numel() == 0
    empty = rank_metrics(torch.zeros(0, device=DEV), torch.zeros(0, device=DEV))
    assert empty.n.tolist() == [0.0] and bool(torch.isnan(empty.auroc).all())


def test_errors():
    from oareactdiff_amd import midrank, rank_metrics
    from oareactdiff_amd._capi import OardError
    a = torch.zeros(4, device=DEV)
    with pytest.raises(OardError):
        rank_metrics(torch.zeros(4), torch.zeros(4))
    with pytest.raises(OardError):
        rank_metrics(a, torch.zeros(4))
    with pytest.raises(OardError):
        midrank(torch.zeros(4))
    with pytest.raises(ValueError):
        rank_metrics(a, torch.zeros(5, device=DEV))
    with pytest.raises(ValueError):
        rank_metrics(a, a, [3, 2])                      # host sizes are checked: more rows than there are


def test_ranking_report_against_a_numpy_loop():
    import scipy.stats
    from oareactdiff_amd import Confidence, rank_candidates, ranking_report
    R, K, threshold = 5, 7, 0.3
    rng = np.random.default_rng(11)
    scores = (np.round(rng.random((K, R)) * 4) / 4).astype(np.float32)          # quarters: ties inside most reactions
    scores[:, 3] = 0.5                                                           # a reaction whose scores are all equal
    rmsd = rng.random((K, R)).astype(np.float32)
    d_s, d_r = torch.from_numpy(scores.reshape(-1)).to(DEV), torch.from_numpy(rmsd.reshape(-1)).to(DEV)
    rep = ranking_report(d_s, d_r, R, threshold=threshold)
    assert Confidence.ranking_report is ranking_report
    best_index = rank_candidates(d_s, R)[0].cpu().numpy()
    assert all(x.shape == (R,) and x.device.type == "cuda" for x in rep)
    for r in range(R):
        pick = int(np.flatnonzero(scores[:, r] == scores[:, r].max())[0])        # highest score, ties by the lower candidate index
        assert best_index[r] == pick
        assert float(rep.top1_rmsd[r]) == rmsd[pick, r] == float(d_r.reshape(K, R)[best_index[r], r])
        assert float(rep.best_rmsd[r]) == rmsd[:, r].min()
        assert bool(rep.hit_at_1[r]) == bool(rmsd[pick, r] < np.float32(threshold))
        assert float(rep.regret[r]) == float(rmsd[pick, r] - rmsd[:, r].min())
        want = rc._corr(scipy.stats.spearmanr, scores[:, r].astype(np.float64), -rmsd[:, r].astype(np.float64))
        got = float(rep.spearman[r])
        assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= rc.TOL_F64, (r, got, want)
    assert np.isnan(float(rep.spearman[3]))
