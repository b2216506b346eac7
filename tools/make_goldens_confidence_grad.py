"""Generate tests/golden/cg_*.npz: one training step of the reference's confidence model per c*_conf_* fixture.

Run:  OA_REACTDIFF_ROOT=<checkout of the reference> python tools/make_goldens_confidence_grad.py [case ...]
(needs the reference importable through the stand-in packages of oracle/_stubs, like tools/make_goldens_confidence.py; never runs on a GPU)

A training step is `ConfModule.training_step` (oa_reactdiff/trainer/pl_trainer.py:554-617): loss = BCELoss(sigmoid(preds), target) with
mixed 0 / 1 labels (four cases), or MSELoss(preds, target) with real-valued targets (the `_forward` case with a per-sample t), then
loss.backward().  `compute_loss` cannot be imported (Lightning, torchmetrics); its two loss lines are restated in
tests/_conf_grad_cases.conf_loss.  For every case it
  1. builds the reference `Confidence(model=LEFTNet)`, loads the fixture's synthetic weights with strict=True and runs the step in
     float64 (the parity target) and in float32 (the reference's own noise floor, `ref_f32_vs_f64` per tensor);
  2. runs the restatement the tests use (tests/_conf_cases.restate64's arithmetic under autograd, tests/_conf_grad_cases.restated_step)
     in float64 with the literal node frame and asserts its gradients equal the reference's: flat <= 1e-8, <= 1e-6 per tensor;
  3. runs the same restatement in float32 with the exact node frame - plain float32 torch on the arithmetic the HIP path implements -
     against the reference's float64 gradients (`torch32_vs_f64` per tensor);
  4. writes the targets, the float64 loss and logits, the names the reference leaves at `.grad is None`, and the float64 gradients in
     the compact layout of tests/golden/g9_grad_* (oracle/make_goldens_grad.py): tensors of up to FULL entries in full, larger ones as
     row sums, column sums and SAMPLE pseudo-randomly chosen entries - what `tests/_grad_cases.GradCase.compare` reads.
A fixture is data only; the inputs stay in the c*_conf_* fixture it names.
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

from _conf_cases import ConfCase  # noqa: E402
from _conf_grad_cases import CG_CASES, conf_loss, restated_step  # noqa: E402
from oareactdiff_amd.spec import hash_uniform  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FULL, SAMPLE = 1024, 128


def hash_name(s):
    h = 0
    for c in s.encode():
        h = (h * 131 + c) % 1000000007
    return h


def sample_index(key, n):
    g = torch.Generator().manual_seed(hash_name(key) % (2 ** 31))
    return torch.randperm(n, generator=g)[:SAMPLE].sort().values


def targets(name: str, kind: str, B: int) -> torch.Tensor:
    if kind == "bce":                              # mixed labels: 1, 0, 1, ...
        return torch.tensor([(b + 1) % 2 for b in range(B)], dtype=torch.float32)
    return torch.from_numpy(hash_uniform(name + ".target", B, 77).reshape(B)).float() * 2.0        # an RMSD-like number in [0, 2)


def gap(g, ref):
    """{name: max|g - ref| / max|ref|} over the tensors the reference has a gradient for."""
    out = {}
    for k, r in ref.items():
        v = g.get(k)
        v = torch.zeros_like(r) if v is None else v.double()
        out[k] = float((v - r).abs().max() / r.abs().max().clamp(min=1e-300))
    return out


def run_case(name: str) -> None:
    src, kind = CG_CASES[name]
    c = ConfCase(src)
    y = targets(name, kind, c.B)
    sd32 = c.state_dict()
    starts = np.concatenate([[0], np.cumsum([x.shape[0] for x in c.xh])])
    masks = [c.combined_mask[starts[k]: starts[k + 1]] for k in range(c.n_obj)]

    def reference(dtype):
        torch.set_default_dtype(dtype)
        try:
            ref = Confidence(model_config=dict(c.cfg), fragment_names=[f"o{k}" for k in range(c.n_obj)], node_nfs=c.node_nfs, edge_nf=0,
                             condition_nf=c.cnf, model=LEFTNet, device=torch.device("cpu"))
            ref.load_state_dict({k: v.to(dtype) for k, v in sd32.items()}, strict=True)
            ref.train(True)
            x = [v.to(dtype) for v in c.xh]
            if c.entry == "forward":
                reps = [{"mask": masks[k], "size": c.sizes[k], "pos": x[k][:, :3], "one_hot": x[k][:, 3:-1], "charge": x[k][:, -1:]}
                        for k in range(c.n_obj)]
                preds = ref.forward(reps, c.conditions.to(dtype))
            else:
                preds = ref._forward(x, c.edge_index, c.t.to(dtype), c.conditions.to(dtype), c.n_frag_switch, c.combined_mask)
            loss = conf_loss(preds, y, kind)
            loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
        grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
        none = [k for k, p in ref.named_parameters() if p.grad is None]
        return grads, none, float(loss.detach()), preds.detach().reshape(-1)

    g32, none32, loss32, _ = reference(torch.float32)
    g64, none64, loss64, logits64 = reference(torch.float64)
    assert none32 == none64
    assert float((logits64 - c.ref64).abs().max()) <= 1e-12 * float(c.ref64.abs().max()), "train-mode logits differ from the c*_conf fixture"

    # the restatement's backward against the reference's, float64, literal node frame
    go, loss_o, _ = restated_step(c, y, kind, torch.float64, "literal")
    per = gap(go, g64)
    num = sum(float((((torch.zeros_like(r) if go.get(k) is None else go[k]) - r) ** 2).sum()) for k, r in g64.items())
    flat = (num / sum(float((r ** 2).sum()) for r in g64.values())) ** 0.5
    worst = max(per.values())
    print(f"{name}: loss f64 {loss64:.12f} f32 {loss32:.8f}; restatement vs reference (f64): flat {flat:.2e}, worst tensor {worst:.2e}")
    assert abs(loss_o - loss64) <= 1e-10 * abs(loss64)
    assert flat <= 1e-8 and worst <= 1e-6, (flat, worst)
    assert all(go.get(k) is None for k in none64), "the restatement reaches a tensor the reference leaves without a gradient"

    ref_gap = gap(g32, g64)
    g32x, _, _ = restated_step(c, y, kind, torch.float32, "exact")
    t32_gap = gap(g32x, g64)
    rows = sorted(g64, key=lambda k: -t32_gap[k])[:4]
    print("   worst plain-float32 tensors: " + "; ".join(f"{k} torch32 {t32_gap[k]:.1e} reference f32 {ref_gap[k]:.1e}" for k in rows))

    out = {"target": y.numpy(), "f64_loss": np.array(loss64), "f32_loss": np.array(loss32), "f64_logits": logits64.numpy()}
    for k, v in g64.items():
        out[f"gnorm.{k}"] = np.array([float(v.norm()), float(v.abs().max())])
        if v.numel() <= FULL:
            out[f"gfull.{k}"] = v.numpy()
        else:
            m2 = v.reshape(v.shape[0], -1)
            out[f"grow.{k}"] = m2.sum(dim=1).numpy()
            out[f"gcol.{k}"] = m2.sum(dim=0).numpy()
            idx = sample_index(k, v.numel())
            out[f"gidx.{k}"] = idx.numpy().astype(np.int32)
            out[f"gval.{k}"] = v.reshape(-1)[idx].numpy()
    out["meta"] = np.array(json.dumps(dict(
        name=name, inputs_of=src, entry=c.entry, loss=kind, grad_none=none64, ref_f32_vs_f64=ref_gap, torch32_vs_f64=t32_gap,
        restatement_vs_ref_f64=dict(flat=flat, worst=worst), layout=dict(full=FULL, sample=SAMPLE))))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"   {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for case in (sys.argv[1:] or CG_CASES):
        run_case(case)
