"""Cost of one validation batch (profiles/validation_step.txt).

Two ways to the same numbers on the production model, alternated block by block in ONE process, on batches the trainer has never seen
(a validation epoch never repeats a batch: every step builds its layout):
    fused    DDPMTrainer.validation_step(batch): oard_loss_eval_prepare, two inference network calls, oard_loss_eval_terms; no host
             read in the step, one `validation_epoch_end()` at the end of every block
    unfused  DDPMTrainer.compute_loss(batch, training=False): DiffusionLoss, the reference's ~150 eager torch ops around the same two
             network calls, and the six .item() reads the reference makes for the logged means (pl_trainer.py:265-277)
Reactions of 3 x `--atoms` atoms at every batch size of `--batches`.  Each variant runs `--repeats` timed blocks of `--steps` steps, a host
clock around work that ends in a device synchronise; prints one JSON line per (batch size, variant) with the mean of the blocks, their
min and max, and the library's own launches per step (its per-family counters; torch's launches are not counted), then the ratios.

    python tools/val_time.py --batches 1,8,64 --steps 10 --repeats 5
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


def trainer(dev):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict
    from oareactdiff_amd.trainer import DDPMTrainer
    cfg = dict(PRODUCTION_LEFTNET_CONFIG)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0, condition_nf=1, device=dev)
    dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg), strict=True)
    dyn.nan_check = "async"
    return DDPMTrainer(dyn, timesteps=1000, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0))


def run(B, args, dev):
    from bench import make_training_batch
    from oareactdiff_amd import _capi
    tr = trainer(dev)

    def fused(batch):
        tr.validation_step(batch)

    def unfused(batch):
        nll, info = tr.compute_loss(batch, training=False)       # lazy_info=False: the six .item() reads happen in there
        return nll.mean()
    variants = {"fused": fused, "unfused": unfused}
    n_b = args.warmup + args.repeats * args.steps
    batches = [make_training_batch(B, args.atoms, 8765 + k, dev) for k in range(n_b)]
    for name, step in variants.items():
        for i in range(args.warmup):
            step(batches[i])
    tr.validation_epoch_end()
    torch.cuda.synchronize(dev)
    blocks = {name: [] for name in variants}
    for r in range(args.repeats):
        for name, step in variants.items():                      # alternating: both variants see the same neighbours on the host
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(batches[args.warmup + r * args.steps + i])
            if name == "fused":
                tr.validation_epoch_end()                        # the epoch's one host read
            torch.cuda.synchronize(dev)
            blocks[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    L = _capi.lib()
    out = {}
    for name, step in variants.items():
        L.oard_timing_reset()
        L.oard_timing_enable(1)
        step(batches[0])
        torch.cuda.synchronize(dev)
        L.oard_timing_enable(0)
        b = blocks[name]
        out[name] = {"variant": name, "batch": B, "atoms": args.atoms, "steps": args.steps, "repeats": args.repeats,
                     "ms_per_step_mean": round(sum(b) / len(b), 3), "ms_per_step_min": round(min(b), 3), "ms_per_step_max": round(max(b), 3),
                     "ms_per_step_blocks": [round(x, 3) for x in b],
                     "library_launches_per_step": int(sum(_capi.timing_get(f)[1] for f in FAMILIES))}
        print(json.dumps(out[name]), flush=True)
    tr.validation_epoch_end()
    f, u = out["fused"], out["unfused"]
    print(f"B = {B}: fused {f['ms_per_step_mean']} ms (min {f['ms_per_step_min']}, max {f['ms_per_step_max']}), unfused "
          f"{u['ms_per_step_mean']} ms (min {u['ms_per_step_min']}, max {u['ms_per_step_max']}), unfused / fused "
          f"{u['ms_per_step_mean'] / f['ms_per_step_mean']:.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--atoms", type=int, default=23)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/val_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for B in (int(x) for x in args.batches.split(",")):
        run(B, args, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
