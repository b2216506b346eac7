"""ms per network call of `DiffusionSampler.inpaint` (T = 100, resamplings = 5, jump_length = 5, synthetic weights, gaussian_prior_std = 1)
on B reactions of 3 x 23 atoms: the earlier launch sequence (fused=False), the fused eager loop, the fused graphed loop.  Each timed with
events on the loop's stream after a warm-up run.  On a tree whose `inpaint` has no `fused` keyword (the parent of the change that added
it) the one loop there is timed, under the name "parent".
usage (GPU box): python tools/inpaint_time.py [--root TREE] [--repeats N] [B ...]        (numbers: profiles/inpaint_loop.txt)"""
import argparse
import inspect
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree to import oareactdiff_amd from")
ap.add_argument("--repeats", type=int, default=3, help="timed runs per configuration (B <= 8; larger batches are timed once)")
ap.add_argument("batches", nargs="*", type=int, default=[1, 8, 64])
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from oareactdiff_amd.dynamics import EGNNDynamics  # noqa: E402
from oareactdiff_amd.sampler import DiffusionSampler  # noqa: E402
from oareactdiff_amd.schedule import get_repaint_schedule  # noqa: E402
from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict  # noqa: E402
from oareactdiff_amd.synthetic import make_inputs, make_topology  # noqa: E402

T, RESAMPLINGS, JUMP, NF = 100, 5, 5, 23
dev = torch.device("cuda:0")
cfg = dict(PRODUCTION_LEFTNET_CONFIG)
dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0, condition_nf=1, device=dev)
dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg, seed=42), strict=True)
calls = sum(get_repaint_schedule(RESAMPLINGS, JUMP, T)) + 1
if "fused" in inspect.signature(DiffusionSampler.inpaint).parameters:
    configs = {"fused=False": dict(fused=False), "fused eager": dict(fused=True, graph=False), "fused graphed": dict(fused=True, graph=True)}
else:
    configs = {"parent": {}}
print(f"inpaint T = {T}, resamplings = {RESAMPLINGS}, jump_length = {JUMP}: {calls} network calls per run; tree {os.path.abspath(args.root)}")
for B in args.batches:
    _, _, _, masks = make_topology(B, NF)
    xh_fixed = make_inputs(B, NF, masks, 5, "cpu")
    frag = [torch.full((B,), NF, dtype=torch.long) for _ in range(3)]
    cond = torch.zeros(B, 1)
    smp = DiffusionSampler(dyn, "polynomial_2", T, 1e-5, pos_only=True, gaussian_prior_std=1.0)
    for name, kw in configs.items():
        run = lambda **more: smp.inpaint(B, frag, conditions=cond, resamplings=RESAMPLINGS, jump_length=JUMP, xh_fixed=xh_fixed,
                                         frag_fixed=[0, 2], **kw, **more)
        torch.manual_seed(1)
        run(timesteps=10)                                   # warm-up: topology, buffers, the library's lazy state
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(args.repeats if B <= 8 else 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            torch.cuda.synchronize(dev)
            ms.append(a.elapsed_time(b) / calls)
        finite = all(bool(torch.isfinite(x).all()) for x in smp.last_x)
        print(f"B = {B:2d}  {name:14s} ms per network call: " + "  ".join(f"{v:.4f}" for v in ms) + ("" if finite else "   (NON-FINITE RESULT)"),
              flush=True)
