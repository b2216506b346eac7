"""Generate tests/golden/c*_conf_*.npz: the reference's `Confidence(model=LEFTNet)` on the inputs of existing fixtures.

Run:  OA_REACTDIFF_ROOT=<checkout of the reference> python tools/make_goldens_confidence.py [case ...]
(needs the reference importable through the stand-in packages of oracle/_stubs, like oracle/make_goldens.py; never runs on a GPU)

For every case it
  1. builds the reference `Confidence` and loads `synthetic_state_dict(confidence_state_spec(...), seed=42)` with strict=True
     (pins the state-dict names and shapes, the twelve `readout.*` tensors included),
  2. runs it in float64 and in float32 - cases (a) - (d) through `forward(representations, conditions)` (t = 0,
     confidence.py:165-193), case (e) through `_forward` with a per-sample `t` column,
  3. checks the restatement the tests use (oracle trunk, float64 mean over every reaction's nodes, gated readout) against the
     float64 reference to 1e-12,
  4. writes inputs, meta, `ref64` and `ref32` logits as a compressed .npz.  A fixture is data only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("OA_REACTDIFF_ROOT")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "oa_reactdiff")):
    sys.exit("set OA_REACTDIFF_ROOT to a checkout of the reference (the directory that holds oa_reactdiff/)")
for p in (os.path.join(ROOT, "oracle", "_stubs"), REFERENCE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oa_reactdiff.dynamics.confidence import Confidence  # noqa: E402  (reference)
from oa_reactdiff.model import LEFTNet  # noqa: E402  (reference)
from oa_reactdiff.utils import get_edges_index  # noqa: E402

from _conf_cases import restate64  # noqa: E402  (the restatement the tests use)
from oareactdiff_amd.spec import confidence_state_spec, hash_uniform, synthetic_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

#: name -> (fixture whose inputs and configuration it takes, entry, purpose)
CASES = {
    "ca_conf_wrapper_small": ("g1_wrapper_small", "forward", "node_nfs = [4, 5, 6], an empty object, condition_nf = 3"),
    "cb_conf_ragged_h32": ("g3_cutoff_ragged", "forward", "B = 3 ragged, H = 32, the cutoff bites"),
    "cc_conf_prod_b1_n5": ("g2s_prod_b1_n5", "forward", "production widths, a single reaction of 15 atoms (0-d result)"),
    "cd_conf_prod_b2_n23": ("g2_prod_b2_n23", "forward", "production widths and shape"),
    "ce_conf_h32_r32_t": ("g6_h32_r32", "_forward", "per-sample t column, ragged objects, H = 32, R = 32, six layers"),
}


def run_case(name: str) -> None:
    src, entry, purpose = CASES[name]
    z = np.load(os.path.join(OUT, src + ".npz"))
    meta = json.loads(str(z["meta"]))
    cfg, node_nfs, cnf = dict(meta["model_config"]), meta["node_nfs"], meta["condition_nf"]
    frag = meta["fragments_nodes"]
    n_obj, B = len(node_nfs), len(frag[0])
    xh = [torch.from_numpy(z[f"xh{k}"]) for k in range(n_obj)]
    conditions = torch.from_numpy(z["conditions"])
    combined_mask, n_frag_switch = torch.from_numpy(z["combined_mask"]), torch.from_numpy(z["n_frag_switch"])
    starts = np.concatenate([[0], np.cumsum([x.shape[0] for x in xh])])
    masks = [combined_mask[starts[k]: starts[k + 1]] for k in range(n_obj)]
    sizes = [torch.tensor(f, dtype=torch.long) for f in frag]
    t = torch.from_numpy(hash_uniform(name + ".t", B, 1234).reshape(B, 1)).float() if entry == "_forward" else torch.tensor([0])
    edge_index = get_edges_index(combined_mask, remove_self_edge=True)

    spec = confidence_state_spec(cfg, node_nfs, cnf)
    sd32 = synthetic_state_dict(spec, cfg, seed=42, dtype=torch.float32)

    def reference(dtype):
        torch.set_default_dtype(dtype)
        ref = Confidence(model_config=dict(cfg), fragment_names=[f"o{k}" for k in range(n_obj)], node_nfs=node_nfs, edge_nf=0,
                         condition_nf=cnf, model=LEFTNet, device=torch.device("cpu"))
        ref.load_state_dict({k: v.to(dtype) for k, v in sd32.items()}, strict=True)          # pins names and shapes
        ref.eval()
        x = [v.to(dtype) for v in xh]
        with torch.no_grad():
            if entry == "forward":
                reps = [{"mask": masks[k], "size": sizes[k], "pos": x[k][:, :3], "one_hot": x[k][:, 3:-1], "charge": x[k][:, -1:]}
                        for k in range(n_obj)]
                out = ref.forward(reps, conditions.to(dtype))
            else:
                out = ref._forward(x, edge_index, t.to(dtype), conditions.to(dtype), n_frag_switch, combined_mask)
        torch.set_default_dtype(torch.float32)
        return out.reshape(-1)
    ref32, ref64 = reference(torch.float32), reference(torch.float64)

    sd64 = {k: v.double() for k, v in sd32.items()}
    restated = restate64(sd64, cfg, xh, edge_index, t, conditions, n_frag_switch, combined_mask, cnf, B)
    dev = float((restated - ref64).abs().max() / ref64.abs().max())
    f32 = float((ref32.double() - ref64).abs().max() / ref64.abs().max())
    print(f"{name}: logits {ref64.tolist()}  restatement vs reference f64 {dev:.2e}  reference f32 vs f64 {f32:.2e}")
    assert dev <= 1e-12, "the restatement disagrees with the reference"

    arrays = {f"xh{k}": xh[k].numpy() for k in range(n_obj)}
    arrays.update(conditions=conditions.numpy(), combined_mask=combined_mask.numpy(), n_frag_switch=n_frag_switch.numpy(),
                  t=t.numpy(), ref64=ref64.numpy(), ref32=ref32.numpy())
    arrays["meta"] = np.array(json.dumps(dict(
        name=name, inputs_of=src, entry=entry, purpose=purpose, model_config=cfg, node_nfs=node_nfs, condition_nf=cnf,
        fragments_nodes=frag, report={"restatement_f64_vs_ref_f64": dev, "ref_f32_vs_ref_f64": f32},
        weights={"generator": "oareactdiff_amd.spec.synthetic_state_dict", "spec": "confidence_state_spec", "seed": 42})))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)


if __name__ == "__main__":
    for case in (sys.argv[1:] or CASES):
        run_case(case)
