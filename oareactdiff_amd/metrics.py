"""Validation metrics on the device: the RMSD between generated and true structures that the reference's trainer logs.

`batch_rmsd` has the signature and defaults of the reference's `batch_rmsd` (oa_reactdiff/analyze/rmsd.py:78-100), `kabsch_rmsd` is the
kernel call under it (`oard_kabsch_rmsd`, csrc/oard_kabsch.h): one wavefront per molecule, float64 arithmetic, no host synchronisation, no
copy of the coordinates out of the `[n, node_nf]` sample tensors.

A DELIBERATE DIFFERENCE from the reference: its `rmsd_core` (rmsd.py:30-51) first searches over permutations of like atoms with pymatgen's
brute-force / genetic / Hungarian matchers.  That search is not implemented here.  This module computes the reference's
`same_order=True` branch (pymatgen's `KabschMatcher`: the optimal rigid superposition with the rows matched in the order given) plus its
chirality handling (rmsd.py:66-74: the z-mirrored structure is fitted too and the smaller RMSD kept).  An inpainted transition state
keeps the atom order of the fixed reactant and product, so the same-order RMSD is well defined; it is an UPPER BOUND on the reference's
order-matched number.

No CPU fallback: tensors that are not on a ROCm device raise `OardError`, as everywhere else in the package."""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

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


def kabsch_rmsd(a: Tensor, b: Tensor, sizes: Union[Tensor, Sequence[int]], ignore_chirality: bool = True, cap: Optional[float] = None,
                return_rotation: bool = False, return_aligned: bool = False):
    """Optimal-superposition RMSD per segment: segment g is the next `sizes[g]` rows of `a` (the target) and `b` (fitted onto it), whose
    first three columns are the coordinates.  -> `[G]` float32 device tensor; with `return_rotation` also `[G, 3, 3]`, the map taking the
    centred `b` onto the centred `a` (improper when the mirror image fitted better); with `return_aligned` also `[n, 3]`, `b` in `a`'s
    frame (`rot (b - c_b) + c_a`).  Returned as rmsd, (rotation), (aligned).

    `ignore_chirality` (the reference's setting in `batch_rmsd`): also fit the z-mirror image, keep the smaller RMSD.  `cap`: the result
    is `min(rmsd, cap)`, and a segment with a non-finite coordinate gives `cap` (None: such a segment gives NaN).  An empty segment gives
    NaN.  Rows are matched in the order given - see the module docstring for the difference from the reference's order matching.

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
    if not isinstance(sizes, Tensor):
        sizes = torch.as_tensor(list(sizes), dtype=torch.int64)
    sizes = sizes.reshape(-1)
    if not sizes.is_cuda:                              # host values: check them here, for free
        if sizes.numel() and (int(sizes.min()) < 0 or int(sizes.sum()) > n):
            raise ValueError(f"sizes must be non-negative and sum to at most the {n} rows given")
    G = int(sizes.numel())
    ends = torch.cumsum(sizes.to(device=dev, dtype=torch.int64).clamp(min=0), 0).clamp_(max=n)
    seg_ptr = torch.zeros(G + 1, dtype=torch.int32, device=dev)
    seg_ptr[1:] = ends
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


def batch_rmsd(fragments_nodes: List[Tensor], out_samples: List[Tensor], xh: List[Tensor], idx: int = 1, ignore_chirality: bool = True,
               cap: Optional[float] = 1.0) -> Tensor:
    """The reference's `batch_rmsd(fragments_nodes, out_samples, xh, idx=1)` (analyze/rmsd.py:78-100) on the device: per reaction the
    RMSD between object `idx` of the generated samples (`out_samples`, per object `[n, node_nf]` as `inpaint` / `sample` return them in
    `out_samples[0]`) and of the true structures `xh`, chirality ignored, capped at 1.0 - also for a molecule whose coordinates are not
    finite, the reference's `except: rmsd = 1.0`.  -> `[B]` float32 device tensor; `.tolist()` is the reference's return value.
    `cap=None` returns the uncapped numbers (NaN for a non-finite molecule).  Same-order matching: see the module docstring (the
    reference's `threshold` argument belongs to its permutation search and has no counterpart)."""
    return kabsch_rmsd(xh[idx], out_samples[idx], fragments_nodes[idx], ignore_chirality=ignore_chirality, cap=cap)
