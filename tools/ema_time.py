"""Cost of the weights' moving average per training step (profiles/trainer_ema.txt).

Three variants of the SAME fused training step (`bench.py --mode train`'s trainer: production model, host_sync=False, a batch the
trainer has never seen at every step):
    off         DDPMTrainer(ema_decay=None)
    fused       DDPMTrainer(ema_decay=d): the average inside the AdamW kernel (oard_adamw_step_dev_ema)
    per_tensor  ema_decay=None, and after every step timm's ModelEmaV2.update as written (trainer/ema.py:37-47):
                `e.copy_(d * e + (1 - d) * p)` for each parameter tensor - the formulation of an average kept outside the trainer
Each variant runs `--repeats` timed blocks of `--steps` steps; prints one JSON line per variant with the mean of the blocks, their
min and max, and the launches of a step: the library's own (its per-family counters) plus, for per_tensor, the four element-wise torch
launches per parameter tensor (two products, one sum, one copy - counted from the expression, not traced).

    python tools/ema_time.py --batch 64 --steps 10 --repeats 5
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("gcl_edge", "equi_edge", "node", "init", "other", "gcl_edge_bwd", "equi_edge_bwd", "wgrad")


def run(variant, args, dev):
    from bench import make_training_batch
    from oareactdiff_amd import _capi
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict
    from oareactdiff_amd.trainer import DDPMTrainer
    cfg = dict(PRODUCTION_LEFTNET_CONFIG)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0, condition_nf=1, device=dev)
    dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg), strict=True)
    dyn.nan_check = "async"
    tr = DDPMTrainer(dyn, timesteps=1000, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0), pos_only=True, host_sync=False,
                     ema_decay=args.decay if variant == "fused" else None)
    shadow = [p.detach().clone() for p in tr.params] if variant == "per_tensor" else None
    d = args.decay

    def step(batch):
        tr.training_step(batch)
        if shadow is not None:
            with torch.no_grad():
                for e, p in zip(shadow, tr.params):
                    e.copy_(d * e + (1. - d) * p)
    n_b = args.warmup + args.repeats * args.steps
    batches = [make_training_batch(args.batch, args.atoms, 4321 + k, dev) for k in range(n_b)]
    for i in range(args.warmup):
        step(batches[i])
    torch.cuda.synchronize(dev)
    blocks = []
    for r in range(args.repeats):
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(batches[args.warmup + r * args.steps + i])
        torch.cuda.synchronize(dev)
        blocks.append((time.perf_counter() - t0) / args.steps * 1e3)
    # the library's launches in a step (per-family counters; the timing pass brackets every launch with events, so it is not timed)
    L = _capi.lib()
    L.oard_timing_reset()
    L.oard_timing_enable(1)
    step(batches[0])
    torch.cuda.synchronize(dev)
    L.oard_timing_enable(0)
    launches = sum(_capi.timing_get(f)[1] for f in FAMILIES)
    out = {"variant": variant, "batch": args.batch, "atoms": args.atoms, "steps": args.steps, "repeats": args.repeats,
           "ms_per_step_mean": round(sum(blocks) / len(blocks), 3), "ms_per_step_min": round(min(blocks), 3),
           "ms_per_step_max": round(max(blocks), 3), "ms_per_step_blocks": [round(b, 3) for b in blocks],
           "library_launches_per_step": int(launches), "ema_torch_launches_per_step": 4 * len(tr.params) if shadow is not None else 0,
           "parameter_tensors": len(tr.params), "bucket_bytes": int(tr.flat_grad.numel() * 4)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=23)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--variants", default="off,fused,per_tensor")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for variant in args.variants.split(","):
        if variant not in ("off", "fused", "per_tensor"):
            raise SystemExit(f"unknown variant {variant!r}")
        run(variant, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
