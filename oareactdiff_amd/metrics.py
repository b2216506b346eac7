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
