"""The algorithm of csrc/oard_rank.h, restated in numpy (`_rank_cases.emulate`: integer compare-and-count, int64 twice-rank sum, two-pass
Pearson), against scipy's `rankdata` / `pearsonr` / `spearmanr` and AUROC by pair counting, on every segment size and kind of the GPU
tests.  Gates: ranks exactly equal; AUROC within 1e-15 (exact integers and one division); the float64 columns within 1e-10."""
import numpy as np
import pytest

import _rank_cases as rc


@pytest.mark.parametrize("kind", rc.KINDS)
def test_emulation_matches_the_references(kind):
    s, t = rc.make_kind(kind)
    ref_rs, ref_rt, ref = rc.reference_of_kind(kind)
    rs, rt, out = rc.emulate(s, t, rc.SIZES)
    assert np.array_equal(rs, ref_rs, equal_nan=True) and np.array_equal(rt, ref_rt, equal_nan=True)
    assert np.isnan(rs[-rc.TRAIL:]).all() and np.isnan(rt[-rc.TRAIL:]).all()
    e_auc, e_f64 = rc.check_table(out, ref, kind)
    print(f"{kind}: worst |auroc - pairs| {e_auc:.2e}; worst float64 column gap {e_f64:.2e}")


def test_pair_count_auroc_is_sklearns():
    sklearn = pytest.importorskip("sklearn.metrics")
    del sklearn
    worst, seen = 0.0, 0
    for kind in rc.KINDS:
        s, t = rc.make_kind(kind)
        ptr = rc.seg_ptr(rc.SIZES)
        for g in range(len(rc.SIZES)):
            a, b = s[ptr[g]:ptr[g + 1]].astype(np.float64), t[ptr[g]:ptr[g + 1]] >= 0.5
            if len(a) == 0 or np.isnan(a).any():
                continue
            want = rc.auroc_sklearn(a, b)
            if want is not None:
                worst, seen = max(worst, abs(rc.auroc_pairs(a, b) - want)), seen + 1
    print(f"pair counting vs sklearn on {seen} segments: worst {worst:.2e}")
    assert seen > 0 and worst <= 1e-12                      # sklearn integrates a curve in float64: its own rounding, not ours


def test_special_cases_give_exactly_the_stated_values():
    nan = float("nan")
    # empty segment: col 0 = 0, the rest NaN
    _, _, out = rc.emulate(np.zeros(3, np.float32), np.zeros(3, np.float32), [0, 3])
    assert out[0, 0] == 0 and np.isnan(out[0, 1:]).all()
    # one class only: AUROC 0
    s = np.array([0.1, 0.7, 0.3], np.float32)
    for label in (0.0, 1.0):
        _, _, out = rc.emulate(s, np.full(3, label, np.float32), [3])
        assert out[0, rc.AUROC] == 0.0 and out[0, rc.NPOS] == 3 * label
    # zero variance in either argument: Pearson and Spearman NaN
    _, _, out = rc.emulate(np.full(4, 0.5, np.float32), np.array([0, 1, 0, 1], np.float32), [4])
    assert np.isnan(out[0, rc.PEARSON]) and np.isnan(out[0, rc.SPEARMAN]) and out[0, rc.AUROC] == 0.5
    _, _, out = rc.emulate(np.array([1, 2, 3, 4], np.float32), np.ones(4, np.float32), [4])
    assert np.isnan(out[0, rc.PEARSON]) and np.isnan(out[0, rc.SPEARMAN])
    # a NaN: cols 2-7 and the ranks NaN in that segment only
    s = np.array([0.2, nan, 0.9, 0.1, 0.8], np.float32)
    t = np.array([0, 1, 1, 0, 1], np.float32)
    rs, rt, out = rc.emulate(s, t, [3, 2])
    assert out[0, 0] == 3 and out[0, 1] == 2 and np.isnan(out[0, 2:]).all() and np.isnan(rs[:3]).all() and np.isnan(rt[:3]).all()
    assert rs[3:].tolist() == [1.0, 2.0] and out[1, rc.AUROC] == 1.0 and abs(out[1, rc.SPEARMAN] - 1.0) <= rc.TOL_F64
    # +-inf is ordered like any value; the moment columns follow IEEE
    s = np.array([np.inf, -np.inf, 0.5, np.inf], np.float32)
    t = np.array([1, 0, 0, 1], np.float32)
    rs, _, out = rc.emulate(s, t, [4])
    assert rs.tolist() == [3.5, 1.0, 2.0, 3.5] and out[0, rc.AUROC] == 1.0 and np.isfinite(out[0, rc.SPEARMAN])
    assert np.isnan(out[0, rc.PEARSON]) and out[0, rc.MAE] == np.inf and np.isnan(out[0, rc.MEAN_S]) and out[0, rc.MEAN_T] == 0.5
    # ties: midranks are exact halves, and count half in AUROC
    s = np.array([0.5, 0.5, 0.5, 0.25], np.float32)
    rs, _, out = rc.emulate(s, np.array([1, 0, 0, 0], np.float32), [4])
    assert rs.tolist() == [3.0, 3.0, 3.0, 1.0] and out[0, rc.AUROC] == (1 + 0.5 * 2) / 3
    # segment boundaries beyond the rows are clamped: the shorter segment's numbers
    a = rc.emulate(s, s, [3, 9])[2]
    b = rc.emulate(s, s, [3, 1])[2]
    assert np.array_equal(a, b, equal_nan=True)
