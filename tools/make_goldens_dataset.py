"""Generate tests/golden/g12_dataset_<cfg>.npz: the reference's `ProcessedTS1x` + `collate_fn` on a seven-reaction raw mapping.

Run:  OA_REACTDIFF_ROOT=<checkout of the reference> python tools/make_goldens_dataset.py [cfg ...]
(imports the reference at run time, like tools/make_goldens_confidence.py; never runs on a GPU)

Raw input: 7 reactions with the unique atom counts [1, 2, 7, 23, 63, 64, 65] (equal across R / TS / P, as in Transition1x), positions
3 * randn + 5 in float64 (centring has something to remove), atomic numbers from {1, 6, 7, 8, 9}; `single_fragment` has one zero and
`use_ind` drops one more reaction.  Seven raw indices below 8 keep the reference's `set` iteration ascending; the generator asserts it
from `size`.  Every fixture holds the raw arrays (concatenated per object), the switches, the reference's collate of the WHOLE dataset
in order (`all.*`) and its collate of one reversed, strided subset (`sub.*`, `sub.index`).  A fixture is data only.
"""
from __future__ import annotations

import copy
import json
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("OA_REACTDIFF_ROOT")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "oa_reactdiff")):
    sys.exit("set OA_REACTDIFF_ROOT to a checkout of the reference (the directory that holds oa_reactdiff/)")
for p in (os.path.join(ROOT, "oracle", "_stubs"), REFERENCE):
    sys.path.insert(0, p)

from oa_reactdiff.dataset.transition1x import ProcessedTS1x  # noqa: E402  (reference)

OUT = os.path.join(ROOT, "tests", "golden")
OBJECTS = ("reactant", "transition_state", "product")
COUNTS = [1, 2, 7, 23, 63, 64, 65]

CONFIGS = {
    "default": {},
    "swap_by_ind": {"swapping_react_prod": True, "use_by_ind": True},                      # production (train_ts1x.py:76-96)
    "reflect_append_multi": {"reflection": True, "append_frag": True, "single_frag_only": False},
    "confidence": {"confidence_model": True},
    "only_ts": {"only_ts": True},
    "zero_charge": {"zero_charge": True},
    "no_center": {"center": False},
}


def make_raw():
    rng = np.random.default_rng(20240612)
    raw = {"single_fragment": [1, 1, 1, 0, 1, 1, 1], "use_ind": [0, 1, 3, 4, 5, 6],
           "target": [int(x) for x in rng.integers(0, 2, len(COUNTS))], "rmsd": [float(x) for x in rng.uniform(0.01, 1.5, len(COUNTS))]}
    for name in OBJECTS:
        raw[name] = {"num_atoms": list(COUNTS), "charges": [rng.choice([1, 6, 7, 8, 9], n).astype(np.int64) for n in COUNTS],
                     "positions": [3.0 * rng.standard_normal((n, 3)) + 5.0 for n in COUNTS]}
    return raw


def collate(ds, index):
    reps, res = ProcessedTS1x.collate_fn([ds[int(i)] for i in index])
    out = {}
    for k, r in enumerate(reps):
        for prop, val in r.items():
            out[f"{k}.{prop}"] = val.numpy()
    if isinstance(res, dict):
        for prop, val in res.items():
            out[prop] = val.numpy()
    else:
        out["condition"] = res.numpy()
    return out


def run(cfg: str) -> None:
    raw = make_raw()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "raw.pkl")
        with open(path, "wb") as f:
            pickle.dump(copy.deepcopy(raw), f)
        ds = ProcessedTS1x(path, **CONFIGS[cfg])
    sw = CONFIGS[cfg]
    keep = [i for i in range(len(COUNTS)) if (raw["single_fragment"][i] == 1 or not sw.get("single_frag_only", True))
            and (i in raw["use_ind"] or not sw.get("use_by_ind", False) or sw.get("confidence_model", False))]
    first_block = [int(x) for x in ds.data["size_0"][: len(keep)]]
    assert first_block == [COUNTS[i] for i in keep], f"{cfg}: the reference's set order is not ascending: {first_block}"
    fix = {"meta": json.dumps({"switches": sw, "n_samples": len(ds)})}
    for name in OBJECTS:
        fix[f"raw.{name}.num_atoms"] = np.asarray(raw[name]["num_atoms"], dtype=np.int64)
        fix[f"raw.{name}.charges"] = np.concatenate(raw[name]["charges"]).astype(np.int8)
        fix[f"raw.{name}.positions"] = np.concatenate(raw[name]["positions"], axis=0)
    for key, dt in (("single_fragment", np.int64), ("use_ind", np.int64), ("target", np.int64), ("rmsd", np.float64)):
        fix[f"raw.{key}"] = np.asarray(raw[key], dtype=dt)
    whole = list(range(len(ds)))
    sub = whole[::-1][::2]
    fix["sub.index"] = np.asarray(sub, dtype=np.int64)
    for tag, index in (("all", whole), ("sub", sub)):
        for key, val in collate(ds, index).items():
            assert val.dtype != object
            fix[f"{tag}.{key}"] = val.astype(np.int8) if val.dtype == np.int64 and "size" not in key and np.abs(val).max(initial=0) < 128 else val
            fix[f"{tag}.{key}.dtype"] = np.asarray(str(val.dtype))
    out = os.path.join(OUT, f"g12_dataset_{cfg}.npz")
    np.savez_compressed(out, **fix)
    assert all(v.dtype != object for v in np.load(out, allow_pickle=False).values())
    print(f"{out}: {len(ds)} samples, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    for name in (sys.argv[1:] or CONFIGS):
        run(name)
