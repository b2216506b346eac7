"""Validation metrics on the device: the RMSD between generated and true structures that the reference's trainer logs.

`batch_rmsd` has the signature and defaults of the reference's `batch_rmsd` (oa_reactdiff/analyze/rmsd.py:78-100), `kabsch_rmsd` is the
kernel call under it (`oard_kabsch_rmsd`, csrc/oard_kabsch.h): one wavefront per molecule, float64 arithmetic, no host synchronisation, no
copy of the coordinates out of the `[n, node_nf]` sample tensors.

`kabsch_rmsd` is the reference's `same_order=True` branch (pymatgen's `KabschMatcher`: the optimal rigid superposition with the rows
matched in the order given) plus its chirality handling (rmsd.py:66-74: the z-mirrored structure is fitted too and the smaller RMSD kept).

`matched_rmsd` (`oard_matched_rmsd`, csrc/oard_match.h) is what the reference's `rmsd_core` (rmsd.py:30-51) computes otherwise: like atoms
are matched first, then the best superposition is taken.  It is defined as the minimum over the species-preserving permutations (and the
mirror image) of the superposition RMSD.  That minimum is returned exactly when there are fewer than `exact_limit` such permutations (the
reference's brute-force branch, `< 1e4`); otherwise it is approached from above by alternating minimum-cost assignment and superposition
from five starts per chirality - the kind of bound the reference's Hungarian branch gives, and never above the same-order number.
`batch_rmsd(..., match_order=True)` uses it.  The default stays the same-order number, an UPPER BOUND on the matched one; an inpainted
transition state keeps the atom order of the fixed reactant and product, so it is well defined there.
STILL DIFFERENT from the reference: pymatgen's genetic matcher with its `threshold`, and the axis heuristics of its Hungarian matcher,
have no counterpart - they define no function of the inputs.

RANKING METRICS (`oard_rank_metrics`, csrc/oard_rank.h): `rank_metrics(score, target, sizes)` gives per segment what the reference's
`ConfModule` logs through torchmetrics - `BinaryAUROC`, `PearsonCorrCoef`, `SpearmanCorrCoef` (trainer/pl_trainer.py:475, 485-486) -, and
`midrank` the average ranks with ties they rest on (`scipy.stats.rankdata(method="average")`).  Integer compare-and-count instead of a
sort, float64 sums in a fixed order: ties are exact, ragged segments are one launch, a segment's bits depend on its own values alone, and
nothing is read back.  `binary_auroc`, `pearson_corrcoef` and `spearman_corrcoef` select one column.

DISTINCT STRUCTURES (`oard_pairwise_rmsd`, `oard_leader_cluster`, csrc/oard_pairwise.h): `pairwise_rmsd(x, sizes, groups)` is the all-pairs
RMSD matrix of every group of structures of ONE coordinate array - the reference's host loop over pymatgen (demo.py:401-480) -, one
wavefront per pair running the body of `kabsch_rmsd` / `matched_rmsd` (the same bits, nothing gathered); `leader_clusters` the reference's
greedy de-duplication on such matrices (demo.py:544-557), one wavefront per group, exact.  `confidence.distinct_candidates` combines them
with `rank_candidates`.

No CPU fallback: tensors that are not on a ROCm device raise `OardError`, as everywhere else in the package."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Union

import torch
from torch import Tensor

from . import _capi


def _coords(x: Tensor, name: str) -> Tensor:
    """A float32 `[n, >= 3]` device tensor with unit column stride, passed through as it is (a strided view of a wider tensor included);
    anything else is converted, which copies."""
    if not isinstance(x, Tensor) or x.dim() != 2 or x.shape[1] < 3:
        raise ValueError(f"{name} must be a [n, >= 3] tensor (got {tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__})")
    if not x.is_cuda:
        raise _capi.OardError(f"kabsch_rmsd needs {name} on a ROCm device (there is no CPU fallback)")
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < 3):
        x = x.contiguous()
    return x


def _segments(sizes: Union[Tensor, Sequence[int]], n: int, dev, limit: Optional[int] = None):
    """`sizes` -> (seg_ptr: int32 device [G + 1], G).  Host values are checked here, for free (ValueError; `limit`: the most rows a
    segment may have); device values are never read back: the boundaries are clamped to the rows that exist."""
    if not isinstance(sizes, Tensor):
        sizes = torch.as_tensor(list(sizes), dtype=torch.int64)
    sizes = sizes.reshape(-1)
    if not sizes.is_cuda and sizes.numel():
        if int(sizes.min()) < 0 or int(sizes.sum()) > n:
            raise ValueError(f"sizes must be non-negative and sum to at most the {n} rows given")
        if limit is not None and int(sizes.max()) > limit:
            raise ValueError(f"a segment of {int(sizes.max())} rows: at most {limit} rows per segment are matched")
    G = int(sizes.numel())
    ends = torch.cumsum(sizes.to(device=dev, dtype=torch.int64).clamp(min=0), 0).clamp_(max=n)
    seg_ptr = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    seg_ptr[1:] = ends
    return seg_ptr, G


def kabsch_rmsd(a: Tensor, b: Tensor, sizes: Union[Tensor, Sequence[int]], ignore_chirality: bool = True, cap: Optional[float] = None,
                return_rotation: bool = False, return_aligned: bool = False):
    """Optimal-superposition RMSD per segment: segment g is the next `sizes[g]` rows of `a` (the target) and `b` (fitted onto it), whose
    first three columns are the coordinates.  -> `[G]` float32 device tensor; with `return_rotation` also `[G, 3, 3]`, the map taking the
    centred `b` onto the centred `a` (improper when the mirror image fitted better); with `return_aligned` also `[n, 3]`, `b` in `a`'s
    frame (`rot (b - c_b) + c_a`).  Returned as rmsd, (rotation), (aligned).

    `ignore_chirality` (the reference's setting in `batch_rmsd`): also fit the z-mirror image, keep the smaller RMSD.  `cap`: the result
    is `min(rmsd, cap)`, and a segment with a non-finite coordinate gives `cap` (None: such a segment gives NaN).  An empty segment gives
    NaN.  Rows are matched in the order given (`matched_rmsd` matches like atoms first).

    `sizes` may be a device tensor: nothing is read back, and the segment boundaries are clamped to the rows that exist, so a wrong
    `sizes` cannot make the kernel read outside `a` / `b` (a host list or CPU tensor is checked instead and raises ValueError)."""
    a, b = _coords(a, "a"), _coords(b, "b")
    dev = a.device
    if b.device != dev:
        raise ValueError("a and b live on different devices")
    n = int(a.shape[0])
    if int(b.shape[0]) != n:
        raise ValueError(f"a has {n} rows, b has {int(b.shape[0])}")
    if cap is not None and not float(cap) > 0.0:
        raise ValueError("cap must be positive (None: no cap)")
    seg_ptr, G = _segments(sizes, n, dev)
    rmsd = torch.empty(G, dtype=torch.float32, device=dev)
    rot = torch.empty(G, 3, 3, dtype=torch.float32, device=dev) if return_rotation else None
    aligned = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev) if return_aligned else None      # rows of no segment: NaN
    if G:
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = _capi.lib().oard_kabsch_rmsd(a.data_ptr(), a.stride(0) if n > 1 else max(int(a.shape[1]), 3), b.data_ptr(),
                                              b.stride(0) if n > 1 else max(int(b.shape[1]), 3), seg_ptr.data_ptr(), G,
                                              1 if ignore_chirality else 0, 0.0 if cap is None else float(cap), rmsd.data_ptr(),
                                              None if rot is None else rot.data_ptr(), None if aligned is None else aligned.data_ptr(),
                                              stream)
        _capi.check(rc, "oard_kabsch_rmsd")
    out = (rmsd,) + ((rot,) if return_rotation else ()) + ((aligned,) if return_aligned else ())
    return out[0] if len(out) == 1 else out


MATCH_MAX_ROWS = 256          # rows per segment of matched_rmsd (MATCH_MAX of csrc/oard_match.h)
MATCH_EXACT, MATCH_SEARCH, MATCH_SPECIES, MATCH_TOO_LARGE, MATCH_NOT_FINITE = range(5)      # its status codes


def _species(x, name: str, n: int, dev) -> Tensor:
    """One int32 per row on `dev`; floating-point values (the charge column of a sample) are truncated, as `int()` does in `xh2pmg`."""
    if not isinstance(x, Tensor):
        x = torch.as_tensor(x)
    x = x.reshape(-1)
    if int(x.numel()) != n:
        raise ValueError(f"{name} must have one entry per row ({n}), got {int(x.numel())}")
    if x.is_cuda and x.device != dev:
        raise ValueError(f"{name} lives on another device than a")
    return x.to(device=dev, dtype=torch.int32).contiguous()


def matched_rmsd(a: Tensor, b: Tensor, sizes: Union[Tensor, Sequence[int]], species, species_b=None, ignore_chirality: bool = True,
                 cap: Optional[float] = None, exact_limit: int = 10000, return_perm: bool = False, return_status: bool = False,
                 return_rotation: bool = False, return_aligned: bool = False):
    """`kabsch_rmsd` with like atoms matched first: per segment the smallest superposition RMSD over the permutations that map every row
    of `a` to a row of `b` of the same species (see the module docstring).  `species`: one integer per row of `a`; `species_b`: per row
    of `b` (None: the same as `species`).  `exact_limit` (0 .. 10000): a segment with fewer species-preserving permutations than this is
    solved exactly, the others by the alternating search; 0 sends every segment to the search.
    -> `[G]` float32 device tensor, then in this order whatever is asked for:
      `return_perm`      `[n]` int64: row r of `a` is matched to row `perm[r]` of `b`, so `b[perm]` is `b` in `a`'s row order;
      `return_status`    `[G]` int32: 0 exact, 1 search, 2 the species lists differ, 3 more than 256 rows, 4 a non-finite coordinate;
      `return_rotation`  `[G, 3, 3]` and `return_aligned` `[n, 3]`: as `kabsch_rmsd`'s, `aligned` in `a`'s row order.
    A segment of status 2, 3 or 4 gives `cap` (None: NaN), NaN maps and the identity permutation; an empty segment gives NaN.
    `sizes`, strided inputs and devices as for `kabsch_rmsd`: a device `sizes` is never read back (a segment above 256 rows shows in the
    status), a host `sizes` with an entry above 256 raises ValueError."""
    a, b = _coords(a, "a"), _coords(b, "b")
    dev = a.device
    if b.device != dev:
        raise ValueError("a and b live on different devices")
    n = int(a.shape[0])
    if int(b.shape[0]) != n:
        raise ValueError(f"a has {n} rows, b has {int(b.shape[0])}")
    if cap is not None and not float(cap) > 0.0:
        raise ValueError("cap must be positive (None: no cap)")
    if not 0 <= int(exact_limit) <= 10000:
        raise ValueError("exact_limit must lie in 0 .. 10000")
    sp_a = _species(species, "species", n, dev)
    sp_b = None if species_b is None else _species(species_b, "species_b", n, dev)
    seg_ptr, G = _segments(sizes, n, dev, limit=MATCH_MAX_ROWS)
    rmsd = torch.empty(G, dtype=torch.float32, device=dev)
    rot = torch.empty(G, 3, 3, dtype=torch.float32, device=dev) if return_rotation else None
    aligned = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev) if return_aligned else None      # rows of no segment: NaN
    perm = torch.arange(n, dtype=torch.int32, device=dev) if return_perm else None                               # ... map to themselves
    status = torch.zeros(G, dtype=torch.int32, device=dev) if return_status else None
    if G:
        ptr = [None if t is None else t.data_ptr() for t in (sp_b, rot, aligned, perm, status)]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = _capi.lib().oard_matched_rmsd(a.data_ptr(), a.stride(0) if n > 1 else max(int(a.shape[1]), 3), b.data_ptr(),
                                               b.stride(0) if n > 1 else max(int(b.shape[1]), 3), sp_a.data_ptr(), ptr[0],
                                               seg_ptr.data_ptr(), G, 1 if ignore_chirality else 0, 0.0 if cap is None else float(cap),
                                               int(exact_limit), rmsd.data_ptr(), ptr[1], ptr[2], ptr[3], ptr[4], stream)
        _capi.check(rc, "oard_matched_rmsd")
    out = (rmsd,) + ((perm.long(),) if return_perm else ()) + ((status,) if return_status else ()) + \
        ((rot,) if return_rotation else ()) + ((aligned,) if return_aligned else ())
    return out[0] if len(out) == 1 else out


def batch_rmsd(fragments_nodes: List[Tensor], out_samples: List[Tensor], xh: List[Tensor], idx: int = 1, ignore_chirality: bool = True,
               cap: Optional[float] = 1.0, match_order: bool = False) -> Tensor:
    """The reference's `batch_rmsd(fragments_nodes, out_samples, xh, idx=1)` (analyze/rmsd.py:78-100) on the device: per reaction the
    RMSD between object `idx` of the generated samples (`out_samples`, per object `[n, node_nf]` as `inpaint` / `sample` return them in
    `out_samples[0]`) and of the true structures `xh`, chirality ignored, capped at 1.0 - also for a molecule whose coordinates are not
    finite, the reference's `except: rmsd = 1.0`.  -> `[B]` float32 device tensor; `.tolist()` is the reference's return value.
    `cap=None` returns the uncapped numbers (NaN for a non-finite molecule).
    `match_order=False`: atoms are compared in the order given (the reference's `same_order=True`).  `match_order=True`: like atoms are
    matched first (`matched_rmsd`; what the reference does by default), the species being the last column of `xh[idx]` and of
    `out_samples[idx]` truncated to an integer, as the reference's `xh2pmg` reads the atomic number; a molecule whose two species lists
    differ gives `cap`, like a non-finite one.  The reference's `threshold` argument belongs to pymatgen's genetic matcher and has no
    counterpart."""
    if not match_order:
        return kabsch_rmsd(xh[idx], out_samples[idx], fragments_nodes[idx], ignore_chirality=ignore_chirality, cap=cap)
    return matched_rmsd(xh[idx], out_samples[idx], fragments_nodes[idx], xh[idx][:, -1], out_samples[idx][:, -1],
                        ignore_chirality=ignore_chirality, cap=cap)


# ---- ranking metrics (csrc/oard_rank.h) --------------------------------------------------------------------------------------------------
RANK_COLS = 8                 # OARD_RANK_COLS of include/oard.h


class RankMetrics(NamedTuple):
    """Per segment, `[G]` float64 device tensors (the columns of `oard_rank_metrics`)."""
    n: Tensor
    n_pos: Tensor
    auroc: Tensor
    pearson: Tensor
    spearman: Tensor
    mae: Tensor
    mean_score: Tensor
    mean_target: Tensor


def _values(x: Tensor, name: str) -> Tensor:
    """A contiguous float32 `[n]` device tensor, passed through as it is; anything else is converted, which copies (as `_coords`)."""
    if not isinstance(x, Tensor):
        raise ValueError(f"{name} must be a tensor (got {type(x).__name__})")
    if not x.is_cuda:
        raise _capi.OardError(f"the ranking metrics need {name} on a ROCm device (there is no CPU fallback)")
    x = x.detach().reshape(-1)
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    return x.contiguous()


def _rank_call(score: Tensor, target: Tensor, sizes, want_out: bool):
    """One `oard_rank_metrics` call -> (ranks [2, n] float64: of score, of target; out [G, 8] | None).  Both rank arrays are always
    handed over: the launch-wide counting kernel then serves the columns that need ranks, whatever the segment lengths."""
    score, target = _values(score, "score"), _values(target, "target")
    dev = score.device
    if target.device != dev:
        raise ValueError("score and target live on different devices")
    n = int(score.numel())
    if int(target.numel()) != n:
        raise ValueError(f"score has {n} entries, target has {int(target.numel())}")
    if sizes is None:                                # one segment of everything: [0, n] in one launch, nothing copied from the host
        seg_ptr = torch.arange(0, n + 1, n, dtype=torch.int32, device=dev) if n else torch.zeros(2, dtype=torch.int32, device=dev)
        G = 1
    else:
        seg_ptr, G = _segments(sizes, n, dev)
    # with a segment the kernel writes every rank (NaN for the rows of no segment); without one nothing is launched
    ranks = torch.empty(2, n, dtype=torch.float64, device=dev) if G else torch.full((2, n), float("nan"), dtype=torch.float64, device=dev)
    out = torch.empty(G, RANK_COLS, dtype=torch.float64, device=dev) if want_out else None
    if G and (n or want_out):
        if n == 0:                                   # an empty tensor has no address; the kernels read nothing
            score = target = torch.zeros(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _capi.lib().oard_rank_metrics(score.data_ptr(), target.data_ptr(), n, seg_ptr.data_ptr(), G,
                                               ranks[0].data_ptr() if n else None, ranks[1].data_ptr() if n else None,
                                               None if out is None else out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(rc, "oard_rank_metrics")
    return ranks, out


def midrank(x: Tensor, sizes: Union[Tensor, Sequence[int], None] = None) -> Tensor:
    """1-based average ranks of `x` inside every segment (segment g: the next `sizes[g]` entries; None: one segment of everything) ->
    `[n]` float64 device tensor, exact half-integers: `scipy.stats.rankdata(method="average")` per segment.  Entries of no segment, and
    every entry of a segment that holds a NaN, are NaN.  `sizes` as for `kabsch_rmsd` (a device tensor is never read back)."""
    return _rank_call(x, x, sizes, False)[0][0]


def rank_metrics(score: Tensor, target: Tensor, sizes: Union[Tensor, Sequence[int], None] = None) -> RankMetrics:
    """Per segment of `score` and `target` (`[n]` each; `sizes=None`: one segment of everything): the number of entries, the number of
    positives (`target >= 0.5`), AUROC of `score` for those positives (ties count half, `BinaryAUROC(thresholds=None)`), Pearson and
    Spearman correlation, mean |score - target| and the two means -> `RankMetrics` of `[G]` float64 device tensors, no host read.
    An empty segment: n = 0, the rest NaN.  One class only: AUROC 0.  A constant argument: Pearson / Spearman NaN.  A NaN in a segment:
    everything but n and n_pos NaN there, the other segments untouched.  Inputs that are not contiguous float32 are converted."""
    out = _rank_call(score, target, sizes, True)[1]
    return RankMetrics(*out.unbind(1))


def binary_auroc(pred: Tensor, target: Tensor, sizes: Union[Tensor, Sequence[int], None] = None) -> Tensor:
    """`rank_metrics(...).auroc`: torchmetrics' `BinaryAUROC(thresholds=None)` (pl_trainer.py:475) per segment, positives `target >= 0.5`."""
    return rank_metrics(pred, target, sizes).auroc


def pearson_corrcoef(pred: Tensor, target: Tensor, sizes: Union[Tensor, Sequence[int], None] = None) -> Tensor:
    """`rank_metrics(...).pearson`: torchmetrics' `PearsonCorrCoef` (pl_trainer.py:485) per segment."""
    return rank_metrics(pred, target, sizes).pearson


def spearman_corrcoef(pred: Tensor, target: Tensor, sizes: Union[Tensor, Sequence[int], None] = None) -> Tensor:
    """`rank_metrics(...).spearman`: torchmetrics' `SpearmanCorrCoef` (pl_trainer.py:486) per segment."""
    return rank_metrics(pred, target, sizes).spearman


# ---- distinct structures: all-pairs RMSD per group and the greedy de-duplication (csrc/oard_pairwise.h) ---------------------------------
PAIR_UNEQUAL = 5              # status of a pair whose members have different row counts (0 .. 4: the MATCH_* codes above)
LEADER_MAX = 1024             # members per group of leader_clusters (OARD_LEADER_MAX of include/oard.h)


def candidate_groups(n_reactions: int, K: int) -> List[List[int]]:
    """The groups of the candidate-major layout (`confidence.rank_candidates`): K repeats of a batch of `n_reactions` reactions, segment
    `k * n_reactions + r` being candidate k of reaction r -> group r = [r, n_reactions + r, 2 n_reactions + r, ...]."""
    if n_reactions < 0 or K < 0:
        raise ValueError("n_reactions and K must be non-negative")
    return [[k * n_reactions + r for k in range(K)] for r in range(n_reactions)]


class PairwiseRmsd:
    """What `pairwise_rmsd` returns: `flat`, ONE float32 device allocation holding the `[K_g, K_g]` matrices of all groups one behind the
    other; `group_ptr` / `mat_ptr`, host tuples (group g has `group_ptr[g + 1] - group_ptr[g]` members, its matrix starts at
    `mat_ptr[g]`); `status`, packed like `flat` (int32), if it was asked for."""

    def __init__(self, flat: Tensor, group_ptr, mat_ptr, status: Optional[Tensor], tables) -> None:
        self.flat, self.group_ptr, self.mat_ptr, self.status = flat, tuple(group_ptr), tuple(mat_ptr), status
        self._tables = tables                          # (int32 device: members + group_ptr, int64 device: pair_ptr + mat_ptr)

    @property
    def n_groups(self) -> int:
        return len(self.group_ptr) - 1

    def size(self, g: int) -> int:
        return self.group_ptr[g + 1] - self.group_ptr[g]

    def _view(self, t: Tensor, g: int) -> Tensor:
        K = self.size(g)
        return t[self.mat_ptr[g]: self.mat_ptr[g] + K * K].view(K, K)

    def matrix(self, g: int) -> Tensor:
        """The `[K_g, K_g]` matrix of group g: a view of `flat`."""
        return self._view(self.flat, g)

    def status_matrix(self, g: int) -> Tensor:
        if self.status is None:
            raise ValueError("the status was not asked for (return_status=True)")
        return self._view(self.status, g)

    def stacked(self) -> Tensor:
        """`[G, K, K]`, a view of `flat`, when every group has K members; ValueError otherwise."""
        sizes = {self.size(g) for g in range(self.n_groups)}
        if len(sizes) > 1:
            raise ValueError(f"the groups have different sizes ({sorted(sizes)}): use matrix(g)")
        K = sizes.pop() if sizes else 0
        return self.flat.view(self.n_groups, K, K)


def _group_tables(groups, S: int, dev):
    """Host `groups` -> (host group_ptr, pair_ptr, mat_ptr; device int32 [members | group_ptr], device int64 [pair_ptr | mat_ptr])."""
    if isinstance(groups, Tensor):
        if groups.is_cuda:
            raise ValueError("groups fixes the shape of the result and must be host data (a sequence of sequences of segment indices), "
                             "not a device tensor")
        groups = groups.tolist()
    groups = [[int(m) for m in grp] for grp in groups]
    members, group_ptr, pair_ptr, mat_ptr = [], [0], [0], [0]
    for grp in groups:
        if any(m < 0 or m >= S for m in grp):
            raise ValueError(f"a group names a segment outside 0 .. {S - 1}")
        K = len(grp)
        members += grp
        group_ptr.append(group_ptr[-1] + K)
        pair_ptr.append(pair_ptr[-1] + K * (K - 1) // 2)
        mat_ptr.append(mat_ptr[-1] + K * K)
    if pair_ptr[-1] > 0x7fffffff or group_ptr[-1] > 0x7fffffff:
        raise ValueError(f"{pair_ptr[-1]} pairs: at most 2^31 - 1 per call")
    t32 = torch.tensor(members + group_ptr, dtype=torch.int32, device=dev)
    t64 = torch.tensor(pair_ptr + mat_ptr, dtype=torch.int64, device=dev)
    return group_ptr, pair_ptr, mat_ptr, t32, t64


def pairwise_rmsd(x: Tensor, sizes: Union[Tensor, Sequence[int]], groups, species=None, match_order: bool = False,
                  ignore_chirality: bool = True, cap: Optional[float] = None, exact_limit: int = 10000,
                  return_status: bool = False) -> PairwiseRmsd:
    """All-pairs RMSD inside every group of structures (`oard_pairwise_rmsd`; the reference's matrix over the transition states of a
    reaction, demo.py:401-480).  Segment s is the next `sizes[s]` rows of `x` (coordinates in the first three columns, read where they
    lie; `sizes` as for `kabsch_rmsd`, a device tensor is never read back).  `groups`: a HOST sequence of sequences of segment indices -
    it fixes the shape of the result -; the members of a group need not be adjacent (`candidate_groups` gives the candidate-major ones).
    Entry [i, j] of a group's matrix is `kabsch_rmsd` (or with `match_order` `matched_rmsd`, `species` one integer per row of `x`) of
    member i as the target and member j fitted onto it, bit for bit; [j, i] is the same value, the diagonal is 0.  One wavefront per pair,
    no gathered copy of the coordinates.  -> `PairwiseRmsd`.
    `return_status`: per entry 0 exact / same-order, 1 search, 2 species lists differ, 3 more than 256 rows (`match_order` only),
    4 a non-finite coordinate, 5 different row counts; 2 .. 5 give `cap` (None: NaN), and a non-finite or over-long member does so along
    its whole row and column, the diagonal included.  An empty member gives NaN."""
    x = _coords(x, "x")
    dev = x.device
    n = int(x.shape[0])
    if cap is not None and not float(cap) > 0.0:
        raise ValueError("cap must be positive (None: no cap)")
    if not 0 <= int(exact_limit) <= 10000:
        raise ValueError("exact_limit must lie in 0 .. 10000")
    if match_order and species is None:
        raise ValueError("match_order needs species (one integer per row of x)")
    sp = _species(species, "species", n, dev) if match_order else None
    seg_ptr, S = _segments(sizes, n, dev, limit=MATCH_MAX_ROWS if match_order else None)
    group_ptr, pair_ptr, mat_ptr, t32, t64 = _group_tables(groups, S, dev)
    G, M = len(group_ptr) - 1, group_ptr[-1]
    flat = torch.empty(mat_ptr[-1], dtype=torch.float32, device=dev)
    status = torch.zeros(mat_ptr[-1], dtype=torch.int32, device=dev) if return_status else None
    if G and M:
        if n == 0:                                   # an empty tensor has no address; every member is empty and nothing is read
            x = torch.zeros(1, 3, dtype=torch.float32, device=dev)
            sp = None if sp is None else torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _capi.lib().oard_pairwise_rmsd(x.data_ptr(), x.stride(0) if x.shape[0] > 1 else max(int(x.shape[1]), 3),
                                                None if sp is None else sp.data_ptr(), seg_ptr.data_ptr(), S, t32.data_ptr(),
                                                t32[M:].data_ptr(), t64.data_ptr(), t64[G + 1:].data_ptr(), G, pair_ptr[-1], M,
                                                (1 if ignore_chirality else 0) | (2 if match_order else 0),
                                                0.0 if cap is None else float(cap), int(exact_limit), flat.data_ptr(),
                                                None if status is None else status.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(rc, "oard_pairwise_rmsd")
    return PairwiseRmsd(flat, group_ptr, mat_ptr, status, (t32, t64))


def leader_clusters(dist, threshold: float = 0.1, order: Optional[Tensor] = None):
    """The reference's greedy de-duplication (demo.py:544-557) per group, on the device (`oard_leader_cluster`): the members are visited
    in index order, or in the order `order` gives (a device int tensor of group-local indices, packed by group like the members); a member
    joins the leader at the smallest distance if that distance is `<= threshold` (a tie: the leader created first; a NaN is never close),
    else it becomes a leader.  `dist`: a `PairwiseRmsd`, or a float32 device tensor `[G, K, K]` (`[K, K]`: one group).
    -> (label, n_clusters): `label` int64 `[sum K_g]` packed by group, the group-local index of every member's leader (a leader labels
    itself); `n_clusters` int64 `[G]`.  A group of more than 1024 members gets -1 throughout.  Device tensors, no host read."""
    if not (float(threshold) >= 0.0) or float(threshold) == float("inf"):
        raise ValueError("threshold must be finite and non-negative")
    if isinstance(dist, PairwiseRmsd):
        flat, group_ptr = dist.flat, dist.group_ptr
        t32, t64 = dist._tables
        G, M = dist.n_groups, group_ptr[-1]
        gp, mp = t32[M:], t64[G + 1:]
        if not flat.is_cuda:
            raise _capi.OardError("leader_clusters needs dist on a ROCm device (there is no CPU fallback)")
    else:
        if not isinstance(dist, Tensor) or dist.dim() not in (2, 3) or dist.shape[-1] != dist.shape[-2]:
            raise ValueError("dist must be a PairwiseRmsd or a [G, K, K] / [K, K] tensor")
        if not dist.is_cuda:
            raise _capi.OardError("leader_clusters needs dist on a ROCm device (there is no CPU fallback)")
        flat = dist.to(torch.float32).contiguous().reshape(-1)
        G, K = (1 if dist.dim() == 2 else int(dist.shape[0])), int(dist.shape[-1])
        M = G * K
        gp = torch.arange(0, M + 1, max(K, 1), dtype=torch.int32, device=flat.device) if K else torch.zeros(G + 1, dtype=torch.int32, device=flat.device)
        mp = torch.arange(0, G + 1, dtype=torch.int64, device=flat.device) * (K * K)
    dev = flat.device
    if order is not None:
        if not isinstance(order, Tensor) or not order.is_cuda or order.device != dev:
            raise ValueError("order must be a device int tensor on dist's device")
        if order.is_floating_point() or int(order.numel()) != M:
            raise ValueError(f"order must hold one integer per member ({M}), packed by group")
        order = order.reshape(-1).to(torch.int32).contiguous()
    label = torch.full((M,), -1, dtype=torch.int32, device=dev)
    n_clusters = torch.zeros(G, dtype=torch.int32, device=dev)
    if G:
        probe = flat if flat.numel() else torch.zeros(1, dtype=torch.float32, device=dev)
        lab = label if M else torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            rc = _capi.lib().oard_leader_cluster(probe.data_ptr(), mp.data_ptr(), gp.data_ptr(),
                                                 None if order is None or not M else order.data_ptr(), G, float(threshold),
                                                 lab.data_ptr(), n_clusters.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(rc, "oard_leader_cluster")
    return label.long(), n_clusters.long()
