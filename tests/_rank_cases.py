"""Shared cases of the ranking-metric tests (csrc/oard_rank.h, `oard_rank_metrics`): segment sizes, kinds of scores and targets, the
float64 references - scipy's `rankdata(method="average")`, `pearsonr`, `spearmanr`, and AUROC by explicit O(n^2) pair counting with half
credit for ties (cross-checked against sklearn's `roc_auc_score` where sklearn imports) - and `emulate`, a numpy restatement of the
kernel's own algorithm: integer compare-and-count, an int64 sum of twice-ranks, two-pass Pearson.  No GPU here."""
import functools
import warnings

import numpy as np
import scipy.stats

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000]      # around the wave (64), the counting workgroup's 64 rows and 256 threads
TRAIL = 7                                                  # rows behind the last segment, in no segment
NAN_SEGMENT = 5                                            # `nan_one`: the segment (64 rows) that holds the one NaN
COLS = 8
N, NPOS, AUROC, PEARSON, SPEARMAN, MAE, MEAN_S, MEAN_T = range(COLS)

VALUES = ["continuous", "quantised", "constant", "saturated"]
TARGETS = ["mixed", "all_pos", "all_neg", "real"]
KINDS = [f"{v}-{t}" for v in VALUES for t in TARGETS] + ["nan_one", "inf"]

TOL_AUROC = 1e-15     # exact integers and one division, the value in [0, 1]
TOL_F64 = 1e-10       # this project's bar for its float64 kernels (tests/test_kabsch_emulation_cpu.py)


def seg_ptr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int32)


def _seed(kind):
    return 1000 + KINDS.index(kind)


def make_values(value_kind, n, rng):
    if value_kind == "continuous":
        x = rng.standard_normal(n)
    elif value_kind == "quantised":
        x = np.round(rng.standard_normal(n) * 8.0) / 8.0
    elif value_kind == "constant":
        x = np.full(n, 0.375)
    elif value_kind == "saturated":                          # float32 sigmoid of N(0, 20^2): ties at exactly 0 and 1
        z = (20.0 * rng.standard_normal(n)).astype(np.float32)
        with np.errstate(over="ignore"):
            x = np.float32(1.0) / (np.float32(1.0) + np.exp(-z, dtype=np.float32))
    else:
        raise KeyError(value_kind)
    return x.astype(np.float32)


def make_targets(target_kind, score, rng):
    n = len(score)
    if target_kind == "mixed":
        t = (rng.random(n) < 0.4).astype(np.float32)
    elif target_kind == "all_pos":
        t = np.ones(n, np.float32)
    elif target_kind == "all_neg":
        t = np.zeros(n, np.float32)
    elif target_kind == "real":
        t = score.astype(np.float64) + 0.5 * rng.standard_normal(n)
    else:
        raise KeyError(target_kind)
    return t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_kind(kind, sizes=tuple(SIZES), trail=TRAIL):
    """-> (score, target) float32 [sum(sizes) + trail], read-only."""
    rng = np.random.default_rng(_seed(kind))
    n = int(sum(sizes)) + trail
    ptr = seg_ptr(sizes)
    if kind == "nan_one":
        s = make_values("continuous", n, rng)
        t = make_targets("mixed", s, rng)
        s[ptr[NAN_SEGMENT] + 17] = np.nan
    elif kind == "inf":
        s = make_values("quantised", n, rng)
        t = make_targets("mixed", s, rng)
        for g, m in enumerate(sizes):
            if m >= 3:
                s[ptr[g]], s[ptr[g] + 1] = np.inf, -np.inf
            if m >= 64:
                s[ptr[g] + 40] = np.inf                       # a tie at +inf
    else:
        v, tk = kind.split("-")
        s = make_values(v, n, rng)
        t = make_targets(tk, s, rng)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t


# ---- references --------------------------------------------------------------------------------------------------------------------------
def auroc_pairs(score, positive):
    """(#{pos > neg} + #{pos == neg} / 2) / (n_pos n_neg) by counting every pair; 0 where a class is missing."""
    p, q = score[positive], score[~positive]
    if len(p) == 0 or len(q) == 0:
        return 0.0
    wins = int((p[:, None] > q[None, :]).sum())
    ties = int((p[:, None] == q[None, :]).sum())
    return (wins + 0.5 * ties) / (len(p) * len(q))


def auroc_sklearn(score, positive):
    """sklearn's number, or None where sklearn is missing, a class is missing or a score is not finite."""
    try:
        from sklearn.metrics import roc_auc_score
    except Exception:
        return None
    if positive.all() or not positive.any() or not np.isfinite(score).all():
        return None
    return float(roc_auc_score(positive.astype(np.int64), score.astype(np.float64)))


def _corr(fn, a, b):
    if len(a) < 2:
        return float("nan")
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            return float(fn(a, b)[0])
        except ValueError:
            return float("nan")


def reference(score, target, sizes):
    """-> (rank_score [n], rank_target [n], table [G, 8]) in float64; rows of no segment and rows of a segment with a NaN rank NaN."""
    s64, t64 = score.astype(np.float64), target.astype(np.float64)
    ptr = seg_ptr(sizes)
    rs, rt = np.full(len(score), np.nan), np.full(len(score), np.nan)
    out = np.full((len(sizes), COLS), np.nan)
    for g in range(len(sizes)):
        a, b = s64[ptr[g]:ptr[g + 1]], t64[ptr[g]:ptr[g + 1]]
        out[g, N] = len(a)
        if len(a) == 0:
            continue
        out[g, NPOS] = int((b >= 0.5).sum())
        if np.isnan(a).any() or np.isnan(b).any():
            continue
        rs[ptr[g]:ptr[g + 1]] = scipy.stats.rankdata(a, method="average")
        rt[ptr[g]:ptr[g + 1]] = scipy.stats.rankdata(b, method="average")
        out[g, AUROC] = auroc_pairs(a, b >= 0.5)
        finite = np.isfinite(a).all() and np.isfinite(b).all()
        out[g, PEARSON] = _corr(scipy.stats.pearsonr, a, b) if finite else np.nan      # inf - inf in the centring: IEEE gives NaN
        out[g, SPEARMAN] = _corr(scipy.stats.spearmanr, a, b)
        with np.errstate(all="ignore"):
            out[g, MAE], out[g, MEAN_S], out[g, MEAN_T] = np.abs(a - b).mean(), a.mean(), b.mean()
    return rs, rt, out


@functools.lru_cache(maxsize=None)
def reference_of_kind(kind):
    s, t = make_kind(kind)
    ref = reference(s, t, SIZES)
    for r in ref:
        r.setflags(write=False)
    return ref


# ---- the kernel's algorithm in numpy -------------------------------------------------------------------------------------------------------
def _counts(x):
    """(less, equal) int64 per row by comparing every pair - no sort."""
    less = (x[None, :] < x[:, None]).sum(axis=1, dtype=np.int64)
    equal = (x[None, :] == x[:, None]).sum(axis=1, dtype=np.int64)
    return less, equal


def emulate(score, target, sizes):
    """csrc/oard_rank.h restated: same outputs as `reference`."""
    n = len(score)
    ptr = np.clip(seg_ptr(sizes).astype(np.int64), 0, n)
    rs, rt = np.full(n, np.nan), np.full(n, np.nan)
    out = np.full((len(sizes), COLS), np.nan)
    for g in range(len(sizes)):
        a, b = score[ptr[g]:ptr[g + 1]], target[ptr[g]:ptr[g + 1]]
        ng = len(a)
        out[g, N] = ng
        if ng == 0:
            continue
        n_pos = int((b >= np.float32(0.5)).sum())
        out[g, NPOS] = n_pos
        if np.isnan(a).any() or np.isnan(b).any():
            continue
        (ls, es), (lt, et) = _counts(a), _counts(b)
        twice_s, twice_t = 2 * ls + es + 1, 2 * lt + et + 1                   # exact integers: twice the midrank
        rs[ptr[g]:ptr[g + 1]], rt[ptr[g]:ptr[g + 1]] = twice_s / 2.0, twice_t / 2.0
        n_neg = ng - n_pos
        r_pos2 = int(twice_s[b >= np.float32(0.5)].sum())
        out[g, AUROC] = 0.0 if n_pos == 0 or n_neg == 0 else float(r_pos2 - n_pos * (n_pos + 1)) / (2.0 * n_pos * n_neg)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        with np.errstate(all="ignore"):
            mean_a, mean_b = a64.sum() / ng, b64.sum() / ng

            def pearson(x, mx, y, my):
                dx, dy = x - mx, y - my
                r = (dx * dy).sum() / (np.sqrt((dx * dx).sum()) * np.sqrt((dy * dy).sum()))
                return r if np.isnan(r) else min(max(r, -1.0), 1.0)
            out[g, PEARSON] = pearson(a64, mean_a, b64, mean_b)
            mean_r = 0.5 * (ng + 1)
            out[g, SPEARMAN] = pearson(twice_s / 2.0, mean_r, twice_t / 2.0, mean_r)
            out[g, MAE], out[g, MEAN_S], out[g, MEAN_T] = np.abs(a64 - b64).sum() / ng, mean_a, mean_b
    return rs, rt, out


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
def worst_gap(got, want):
    """max |got - want| over entries where both are finite; entries where either is not must agree exactly (NaN with NaN, inf with inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    both = np.isfinite(got) & np.isfinite(want)
    rest_same = np.array_equal(got[~both], want[~both], equal_nan=True)
    assert rest_same, ("non-finite entries differ", got[~both], want[~both])
    return float(np.abs(got[both] - want[both]).max()) if both.any() else 0.0


def check_table(got, want, what=""):
    """The gates of the issue on a [G, 8] table -> the worst gaps (auroc, float64 columns), for printing."""
    assert np.array_equal(got[:, [N, NPOS]], want[:, [N, NPOS]], equal_nan=True), what
    e_auc = worst_gap(got[:, AUROC], want[:, AUROC])
    e_f64 = max(worst_gap(got[:, c], want[:, c]) for c in (PEARSON, SPEARMAN, MAE, MEAN_S, MEAN_T))
    assert e_auc <= TOL_AUROC, (what, e_auc)
    assert e_f64 <= TOL_F64, (what, e_f64)
    return e_auc, e_f64
