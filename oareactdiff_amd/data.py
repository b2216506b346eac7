"""A reaction dataset held in flat arrays on the device, and an epoch loader that assembles every batch in one kernel launch.

Replaces `ProcessedTS1x` + `BaseDataset.collate_fn` + `DataLoader` (oa_reactdiff/dataset/transition1x.py:21-150,
dataset/base_dataset.py:51-88,142-217) in front of `DDPMTrainer` / `ConfidenceTrainer`.

`ReactionStore` keeps, per source object (reactant, transition state, product), `offsets [R + 1]`, the raw float32 positions and the
atomic numbers, once.  The swapped and reflected copies the reference materialises are VIRTUAL: sample index v decodes as
    f_bit = v // (R_sel * s),  j = v % (R_sel * s),  s_bit = j // R_sel,  r = sel[j % R_sel]
(original block, swapped block, then the reflected copy of both - the reference's list order), and `k_reaction_gather`
(csrc/oard_dataset.h) builds the one-hot rows, the charge columns, the centred positions and the masks of a whole batch from them.
`sel` is ascending; the reference iterates a Python `set` (transition1x.py:62), whose order is an implementation detail - the one
deliberate deviation.  The reference's `target` / `rmsd` columns are its raw lists, neither selected nor reflected, read at the
sample's own index (transition1x.py:92-98); the store does the same and refuses a configuration in which that index runs past them.

`DeviceLoader` is `DataLoader(dataset, batch_size, sampler=DistributedSampler(...), collate_fn=...)`: per epoch ONE upload (the index
list and, per object, the prefix sums of the atom counts in epoch order), then per batch one launch that takes `(first, B)`.  Batches
carry `mask_host` / `size_host` built from the host copy of the counts, so the trainers' fused step needs no device read.
"""
from __future__ import annotations

import ctypes as C
import io
import pickle
from typing import Any, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi

OBJECTS = ("reactant", "transition_state", "product")
ELEMENTS = (1, 6, 7, 8, 9)                                   # ATOM_MAPPING (base_dataset.py:8-14)


# ---- reading the raw mapping ----------------------------------------------------------------------------------------------------
_PICKLE_GLOBALS = {
    ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
    ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
    ("numpy", "ndarray"), ("numpy", "dtype"),
}
_PICKLE_BUILTINS = {"list", "dict", "tuple", "set", "frozenset", "int", "float", "bool", "complex", "str", "bytes", "bytearray",
                    "range", "slice"}


class _DataUnpickler(pickle.Unpickler):
    """Plain containers, numbers and numpy arrays; every other global is refused (as `checkpoint.py` reads a checkpoint without
    importing what its pickle names - a data blob has no reason to name anything)."""

    def find_class(self, module: str, name: str):
        if (module, name) in _PICKLE_GLOBALS or (module == "builtins" and name in _PICKLE_BUILTINS):
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"dataset pickle names {module}.{name}: only containers, numbers and numpy arrays are read")


def load_raw(path: str) -> Dict[str, Any]:
    """The raw mapping of a data file.  `.pkl`: the reference's format (a dict of dicts), through the restricted unpickler.
    `.npz` (allow_pickle=False): the same mapping with flat keys `"<object>.<field>"` (`reactant.num_atoms`, `reactant.charges`,
    `reactant.positions`, ...) beside `single_fragment`, `use_ind`, `target`, `rmsd`; `charges` / positions either padded per reaction
    (`[R, max n]`, `[R, max n, 3]`) or concatenated (`[sum n]`, `[sum n, 3]`)."""
    p = str(path)
    if p.endswith(".npz"):
        raw: Dict[str, Any] = {}
        with np.load(p, allow_pickle=False) as z:
            for key in z.files:
                if "." in key and key.split(".", 1)[0] in OBJECTS:
                    obj, field = key.split(".", 1)
                    raw.setdefault(obj, {})[field] = z[key]
                else:
                    raw[key] = z[key]
        return raw
    if p.endswith(".pkl"):
        with open(p, "rb") as f:
            raw = _DataUnpickler(io.BytesIO(f.read())).load()
        if not isinstance(raw, Mapping):
            raise ValueError(f"{p}: not a mapping")
        return dict(raw)
    raise ValueError("data file should be either .npz or .pkl")


def _flatten(obj: Mapping, pos_key: str, name: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (counts [R] int64, atomic numbers [sum n] int32, positions [sum n, 3] float32): `x[ii][:num_atoms[ii]]` of the reference,
    the float64 positions rounded once as `torch.tensor(..., dtype=torch.float32)` rounds them."""
    for key in ("num_atoms", "charges", pos_key):
        if key not in obj:
            raise KeyError(f"{name}[{key!r}] is missing")
    n = np.asarray(obj["num_atoms"], dtype=np.int64).reshape(-1)
    if n.size and n.min() < 1:
        raise ValueError(f"{name}: a reaction without atoms")
    R, total = n.size, int(n.sum())

    def gather(x, tail):
        if isinstance(x, np.ndarray) and x.dtype != object and x.ndim == 1 + len(tail):           # concatenated
            if x.shape[0] != total:
                raise ValueError(f"{name}: {x.shape[0]} rows for {total} atoms")
            return x
        if isinstance(x, np.ndarray) and x.dtype != object and x.ndim == 2 + len(tail):           # padded per reaction
            if x.shape[0] != R or (R and x.shape[1] < n.max()):
                raise ValueError(f"{name}: padded array {x.shape} does not hold {R} reactions of up to {n.max() if R else 0} atoms")
            return x[np.arange(x.shape[1])[None, :] < n[:, None]]
        if len(x) != R:
            raise ValueError(f"{name}: {len(x)} entries for {R} reactions")
        rows = [np.asarray(x[i])[: n[i]] for i in range(R)]
        if any(r.shape[0] != n[i] for i, r in enumerate(rows)):
            raise ValueError(f"{name}: an entry shorter than its num_atoms")
        return np.concatenate(rows, axis=0) if rows else np.zeros((0,) + tail)

    z = np.ascontiguousarray(gather(obj["charges"], ()), dtype=np.int32).reshape(total)
    pos = np.ascontiguousarray(np.asarray(gather(obj[pos_key], (3,)), dtype=np.float64).astype(np.float32)).reshape(total, 3)
    return n, z, pos


class EpochPlan(NamedTuple):
    """The host side of an epoch: `indices [L]` virtual sample indices in epoch order, `batches` the `(first, B)` of every step,
    `counts [n_obj, L]` / `offsets [n_obj, L + 1]` the atom counts along `indices` and their exclusive prefix sums."""
    indices: np.ndarray
    batches: List[Tuple[int, int]]
    counts: np.ndarray
    offsets: np.ndarray

    def size_host(self, i: int) -> List[torch.Tensor]:
        first, B = self.batches[i]
        return [torch.from_numpy(self.counts[k, first: first + B].copy()) for k in range(self.counts.shape[0])]

    def atoms(self, i: int) -> List[int]:
        first, B = self.batches[i]
        return [int(self.offsets[k, first + B] - self.offsets[k, first]) for k in range(self.counts.shape[0])]

    def table(self) -> np.ndarray:
        """What an epoch uploads, as one array: row 0 the indices (one pad entry), rows 1.. the offsets."""
        t = np.zeros((1 + self.offsets.shape[0], self.offsets.shape[1]), dtype=np.int64)
        t[0, :-1] = self.indices
        t[1:] = self.offsets
        return t


class ReactionStore:
    """`ProcessedTS1x(raw, **switches)` as flat arrays; `len(store)` and the sample order are the reference's with `sel` ascending.
    `device=None` keeps the store on the host (plans, counts, decoding); `batch` needs a device."""

    def __init__(self, raw: Mapping, device=None, center: bool = True, pad_fragments: int = 0, zero_charge: bool = False,
                 remove_h: bool = False, single_frag_only: bool = True, swapping_react_prod: bool = False, append_frag: bool = False,
                 reflection: bool = False, use_by_ind: bool = False, only_ts: bool = False, confidence_model: bool = False,
                 position_key: str = "positions", ediff: Optional[str] = None):
        if pad_fragments > 0:
            raise NotImplementedError("pad_fragments > 0 is not supported (the reference's dummy molecules fail with center=True)")
        if confidence_model:
            use_by_ind = False                                                     # transition1x.py:48-49
        if "single_fragment" not in raw:
            raise KeyError("raw['single_fragment'] is missing")
        single = np.asarray(raw["single_fragment"]).reshape(-1)
        R = single.size
        keep = np.nonzero(single == 1)[0] if single_frag_only else np.arange(R)
        if use_by_ind:
            if "use_ind" not in raw:
                raise ValueError("use_by_ind=True needs raw['use_ind']")
            keep = np.intersect1d(keep, np.asarray(raw["use_ind"], dtype=np.int64).reshape(-1))
        self.sel = np.unique(keep).astype(np.int64)                                # ascending (module docstring)
        if self.sel.size == 0:
            raise ValueError("no reaction is selected")
        self.n_raw, self.n_sel = R, int(self.sel.size)
        self.swap, self.reflect = int(bool(swapping_react_prod)), int(bool(reflection))
        self.center, self.zero_charge = bool(center), bool(zero_charge)
        self.append_frag = bool(append_frag) and not self.zero_charge              # base_dataset.py:170-178: zero_charge wins
        self.only_ts, self.confidence_model, self.ediff_name = bool(only_ts), bool(confidence_model), ediff
        self.src_obj = [1] if only_ts else [0, 1, 2]
        self.n_obj = len(self.src_obj)
        # the transition state is always read from "positions" (transition1x.py:108,121,135), and reflect_z touches `position_key` only
        keys = [position_key, "positions", position_key]
        self.reflect_obj = [int(keys[s] == position_key) for s in self.src_obj]
        self.append_charge = [[0, 1, 0][s] for s in self.src_obj]
        used = sorted(set(self.src_obj) | ({2 - s for s in self.src_obj} if self.swap else set()))
        self.counts: List[Optional[np.ndarray]] = [None] * 3                       #: per source object, on the host
        self.offsets: List[Optional[np.ndarray]] = [None] * 3
        self._z: List[Optional[np.ndarray]] = [None] * 3
        self._pos: List[Optional[np.ndarray]] = [None] * 3
        for s in used:
            if OBJECTS[s] not in raw:
                raise KeyError(f"raw[{OBJECTS[s]!r}] is missing")
            n, z, pos = _flatten(raw[OBJECTS[s]], keys[s], OBJECTS[s])
            if n.size != R:
                raise ValueError(f"{OBJECTS[s]}: {n.size} reactions, single_fragment has {R}")
            off = np.zeros(R + 1, dtype=np.int64)
            np.cumsum(n, out=off[1:])
            chosen = np.zeros(R, dtype=bool)
            chosen[self.sel] = True
            bad = ~np.isin(z, ELEMENTS) & np.repeat(chosen, n)
            if bad.any():
                raise ValueError(f"{OBJECTS[s]}: atomic number {int(z[bad][0])} is outside {set(ELEMENTS)}")
            self.counts[s], self.offsets[s], self._z[s], self._pos[s] = n, off, z, pos
        self._target = self._rmsd = None
        self._ediff: Optional[List[np.ndarray]] = None
        if confidence_model:
            for key in ("target", "rmsd"):
                if key not in raw or len(raw[key]) != R:
                    raise ValueError(f"confidence_model=True needs raw[{key!r}] with one entry per raw reaction")
            if len(self) > R * (1 + self.swap):
                raise ValueError("confidence_model with reflection reads past the reference's target list")
            self._target = np.ascontiguousarray(raw["target"], dtype=np.int64).reshape(R)
            self._rmsd = np.ascontiguousarray(raw["rmsd"], dtype=np.float32).reshape(R)
        if ediff is not None:
            if ediff not in OBJECTS:
                raise ValueError(f"ediff must be one of {OBJECTS}")
            a = OBJECTS.index(ediff)
            cols = []
            for s in ([a, 2 - a] if self.swap else [a, a]):
                if OBJECTS[s] not in raw or "ediff" not in raw[OBJECTS[s]]:
                    raise KeyError(f"raw[{OBJECTS[s]!r}]['ediff'] is missing")
                cols.append(np.ascontiguousarray(raw[OBJECTS[s]]["ediff"], dtype=np.float32).reshape(R))
            self._ediff = cols
        self.device = None
        self.alloc = torch.empty                                                   #: the allocator of a batch's outputs
        self._dev: Dict[str, Any] = {}
        self._cstore = None
        if device is not None:
            self.to(device)

    @classmethod
    def from_file(cls, path: str, **switches) -> "ReactionStore":
        return cls(load_raw(path), **switches)

    def __len__(self) -> int:
        return self.n_sel * (1 + self.swap) * (1 + self.reflect)

    # ---- host arithmetic -------------------------------------------------------------------------------------------------------
    def decode(self, v) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Virtual indices -> (f_bit, s_bit, r), as the kernel decodes them."""
        v = np.asarray(v, dtype=np.int64)
        if v.size and (v.min() < 0 or v.max() >= len(self)):
            raise IndexError(f"sample index outside [0, {len(self)})")
        block = self.n_sel * (1 + self.swap)
        j = v % block
        return v // block, j // self.n_sel, self.sel[j % self.n_sel]

    def counts_of(self, v) -> np.ndarray:
        """[n_obj, len(v)] atom counts of the samples' objects (a swapped sample reads the partner's)."""
        _, s_bit, r = self.decode(v)
        out = np.empty((self.n_obj, r.size), dtype=np.int64)
        for k, s in enumerate(self.src_obj):
            own = self.counts[s][r]
            out[k] = np.where(s_bit == 1, self.counts[2 - s][r], own) if self.swap else own
        return out

    def plan(self, indices, batches: Optional[Sequence[Tuple[int, int]]] = None) -> EpochPlan:
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        counts = self.counts_of(idx)
        off = np.zeros((self.n_obj, idx.size + 1), dtype=np.int64)
        np.cumsum(counts, axis=1, out=off[:, 1:])
        return EpochPlan(idx, [(0, int(idx.size))] if batches is None else list(batches), counts, off)

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def to(self, device) -> "ReactionStore":
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("the store's batches are built by a HIP kernel: the device must be a ROCm device")
        up = lambda a: None if a is None else torch.from_numpy(a).to(device)      # noqa: E731
        d = {"offsets": [up(a) for a in self.offsets], "pos": [up(a) for a in self._pos], "z": [up(a) for a in self._z],
             "sel": up(self.sel), "target": up(self._target), "rmsd": up(self._rmsd),
             "ediff": [None, None] if self._ediff is None else [up(a) for a in self._ediff]}
        ptr = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        cs = _capi.OardReactionStore()
        for s in range(3):
            cs.offsets[s], cs.pos[s], cs.z[s] = ptr(d["offsets"][s]), ptr(d["pos"][s]), ptr(d["z"][s])
        cs.sel, cs.target, cs.rmsd = ptr(d["sel"]), ptr(d["target"]), ptr(d["rmsd"])
        cs.ediff[0], cs.ediff[1] = ptr(d["ediff"][0]), ptr(d["ediff"][1])
        cs.n_raw, cs.n_sel, cs.n_obj = self.n_raw, self.n_sel, self.n_obj
        for k in range(self.n_obj):
            cs.src_obj[k], cs.reflect_obj[k], cs.append_charge[k] = self.src_obj[k], self.reflect_obj[k], self.append_charge[k]
        cs.swap, cs.reflect, cs.center = self.swap, self.reflect, int(self.center)
        cs.zero_charge, cs.append_frag = int(self.zero_charge), int(self.append_frag)
        self.device, self._dev, self._cstore = device, d, cs
        return self

    def upload_plan(self, plan: EpochPlan) -> torch.Tensor:
        """The plan's table on the device: one blocking copy from pageable memory (the host array is free on return)."""
        if self.device is None:
            raise _capi.OardError("the store is on the host: move it with .to(device) first")
        return torch.from_numpy(plan.table()).to(self.device)

    def gather(self, table: torch.Tensor, plan: EpochPlan, i: int):
        """Batch `i` of `plan` (whose table is `table`): one launch, no copy in either direction."""
        first, B = plan.batches[i]
        if B < 1:
            raise ValueError("an empty batch")
        dev, n_obj, new = self.device, self.n_obj, self.alloc
        size_host, atoms = plan.size_host(i), plan.atoms(i)
        width = 2 if self.append_frag else 1
        i64 = dict(dtype=torch.int64, device=dev)
        reps = []
        for k in range(n_obj):
            n = atoms[k]
            reps.append({"size": new((B,), **i64), "pos": new((n, 3), dtype=torch.float32, device=dev), "one_hot": new((n, 5), **i64),
                         "charge": new((n, width), **i64), "mask": new((n,), **i64)})
        cond = new((B, 1), **i64)
        target = new((B,), **i64) if self._target is not None else None
        rmsd = new((B,), dtype=torch.float32, device=dev) if self._rmsd is not None else None
        ediff = new((B,), dtype=torch.float32, device=dev) if self._ediff is not None else None
        row = table.shape[1] * 8
        off = (C.c_void_p * n_obj)(*[table.data_ptr() + (1 + k) * row for k in range(n_obj)])
        arrays = [_capi.ptr_array([r[key] for r in reps]) for key in ("size", "pos", "one_hot", "charge", "mask")]
        ptr = lambda t: None if t is None else t.data_ptr()                        # noqa: E731
        rc = _capi.lib().oard_dataset_gather(C.byref(self._cstore), table.data_ptr(), off, first, B, *arrays, cond.data_ptr(), ptr(target),
                                             ptr(rmsd), ptr(ediff), torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(rc, "oard_dataset_gather")
        rows = torch.arange(B, dtype=torch.int64)
        for k, r in enumerate(reps):
            r["size_host"], r["mask_host"] = size_host[k], torch.repeat_interleave(rows, size_host[k])
        if target is None and ediff is None:
            return reps, cond
        res = {}                                                                   # base_dataset.py:82-88: a dict once there is more
        if target is not None:
            res["target"], res["rmsd"] = target, rmsd
        if ediff is not None:
            res["ediff"] = ediff
        res["condition"] = cond
        return reps, res

    def batch(self, indices):
        """`collate_fn([dataset[v] for v in indices])` on the device, in `DDPMTrainer.to_device`'s layout: `(representations,
        conditions)`.  `indices`: host ints (a device tensor is copied to the host once - the loader never does that)."""
        if isinstance(indices, torch.Tensor):
            indices = indices.detach().cpu().numpy()
        plan = self.plan(indices)
        return self.gather(self.upload_plan(plan), plan, 0)


class DeviceLoader:
    """Batches of `store` in the index stream of `DistributedSampler(range(len(store)), num_replicas=world_size, rank=rank,
    shuffle=shuffle, seed=seed, drop_last=False)` after `set_epoch(e)`: `randperm` under `manual_seed(seed + e)`, padded by wrapping,
    strided by rank - every rank takes the same number of steps.  `drop_last` drops the last short BATCH, as `DataLoader` does."""

    def __init__(self, store: ReactionStore, batch_size: int, shuffle: bool = False, drop_last: bool = False, seed: int = 0,
                 rank: int = 0, world_size: int = 1):
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError("batch_size >= 1 and 0 <= rank < world_size are required")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world_size, self.epoch = int(seed), int(rank), int(world_size), 0
        self.num_samples = -(-len(store) // self.world_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        full, rest = divmod(self.num_samples, self.batch_size)
        return full + (1 if rest and not self.drop_last else 0)

    def indices(self, epoch: int) -> np.ndarray:
        n = len(self.store)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + epoch)
            idx = torch.randperm(n, generator=g).numpy()
        else:
            idx = np.arange(n, dtype=np.int64)
        total = self.num_samples * self.world_size
        if total > n:
            idx = np.concatenate([idx, np.resize(idx, total - n)])                 # pad by wrapping
        return np.ascontiguousarray(idx[self.rank: total: self.world_size], dtype=np.int64)

    def epoch_plan(self, epoch: Optional[int] = None) -> EpochPlan:
        """The host side of epoch `epoch` (default: the one `set_epoch` chose); a pure host function."""
        idx = self.indices(self.epoch if epoch is None else int(epoch))
        batches = [(a, min(self.batch_size, idx.size - a)) for a in range(0, idx.size, self.batch_size)]
        if self.drop_last and batches and batches[-1][1] < self.batch_size:
            batches.pop()
        return self.store.plan(idx, batches)

    def __iter__(self):
        plan = self.epoch_plan()
        table = self.store.upload_plan(plan)
        for i in range(len(plan.batches)):
            yield self.store.gather(table, plan, i)
