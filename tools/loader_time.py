"""Time the device-resident loader against a per-sample collate, alone and in front of `DDPMTrainer.training_step`.

Run on a ROCm device:  python tools/loader_time.py [--out profiles/loader.txt] [--batches 200] [--repeats 5] [--step-repeats 3]

Workload: a synthetic Transition1x-shaped store of 9 000 reactions, R / TS / P of the same 7 ... 23 atoms each (seeded, N(0, 1) positions
as bench.py's batches), `swapping_react_prod=True` (18 000 samples), shuffled.  Legs, each event-timed over >= `--batches` batches after a
warm-up pass, repeated `--repeats` times with the legs alternating inside every repeat (median and min .. max are reported):
  loader      `DeviceLoader` batches at B = 14 and B = 64 (the window holds one epoch start - plan and upload -, also reported by itself);
  collate     the reference's way restated in plain torch: one dict of device tensors per sample (`__getitem__`), `torch.cat` of B of them
              per property and object (`collate_fn`), then `DDPMTrainer.to_device` (its `.cpu()` of mask and size blocks per step);
  step        `training_step` (production widths, host_sync=False) fed by the loader, by the collate, and by the loader's batches built
              BEFORE the window (the pre-built-batch step bench.py --mode train times).
Nothing here reads the reference; a run without a device fails."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oareactdiff_amd.data import DeviceLoader, ReactionStore  # noqa: E402
from oareactdiff_amd.trainer import DDPMTrainer  # noqa: E402

PROPS = ("size", "pos", "one_hot", "charge", "mask")


def synthetic_raw(n_reactions=9000, seed=1234):
    rng = np.random.default_rng(seed)
    n = rng.integers(7, 24, n_reactions)
    raw = {"single_fragment": np.ones(n_reactions, dtype=np.int64), "use_ind": np.arange(n_reactions)}
    for name in ("reactant", "transition_state", "product"):
        raw[name] = {"num_atoms": n, "charges": rng.choice([1, 6, 7, 8], int(n.sum()), p=[0.5, 0.3, 0.1, 0.1]),
                     "positions": rng.standard_normal((int(n.sum()), 3))}
    return raw


class PerSampleDataset:
    """`ProcessedTS1x.data` with every item on the device, and the reference's `collate_fn`, in plain torch."""

    def __init__(self, store: ReactionStore):
        n = len(store)
        reps, cond = store.batch(np.arange(n))                       # the processed samples, once; items are views of it
        torch.cuda.synchronize()
        self.items = []
        starts = [np.concatenate([[0], np.cumsum(r["size_host"].numpy())]) for r in reps]
        zero = torch.zeros(1, 1, dtype=torch.int64, device=store.device)
        zeros = torch.zeros(64, dtype=torch.int64, device=store.device)
        for v in range(n):
            item = {"condition": zero}
            for k, r in enumerate(reps):
                a, b = int(starts[k][v]), int(starts[k][v + 1])
                item[f"size_{k}"] = r["size"][v]
                item[f"pos_{k}"], item[f"one_hot_{k}"], item[f"charge_{k}"] = r["pos"][a:b], r["one_hot"][a:b], r["charge"][a:b]
                item[f"mask_{k}"] = zeros[: b - a]
            self.items.append(item)

    @staticmethod
    def collate(batch):
        out = [{} for _ in range(3)]
        for k in range(3):
            out[k]["size"] = torch.stack([x[f"size_{k}"] for x in batch])
            out[k]["mask"] = torch.cat([i * torch.ones(len(x[f"mask_{k}"]), device=x[f"mask_{k}"].device).long() for i, x in enumerate(batch)], dim=0)
            for prop in ("pos", "one_hot", "charge"):
                out[k][prop] = torch.cat([x[f"{prop}_{k}"] for x in batch], dim=0)
        return out, torch.cat([x["condition"] for x in batch], dim=0)

    def batches(self, indices, B):
        for a in range(0, len(indices), B):
            yield DDPMTrainer.to_device(self.collate([self.items[int(v)] for v in indices[a: a + B]]), self.items[0]["condition"].device)


def timed(fn):
    """-> (ms of device time between two events around fn(), fn's count of batches)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    n = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), n


def summary(vals):
    return f"median {statistics.median(vals):9.4f}  min {min(vals):9.4f}  max {max(vals):9.4f}  (n = {len(vals)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader.txt"))
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=3)
    ap.add_argument("--step-batch", type=int, nargs="*", default=[14, 64])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loader_time.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             "store: 9000 reactions x (R, TS, P) of 7..23 atoms, swapping_react_prod -> 18000 samples, shuffle=True",
             f"every figure: ms per batch, event-timed over >= {args.batches} batches after a warm-up pass; legs alternate inside each repeat", ""]
    store = ReactionStore(synthetic_raw(), device=dev, swapping_react_prod=True)
    ref = PerSampleDataset(store)

    def loader_pass(B, epoch, consume=None):
        loader = DeviceLoader(store, batch_size=B, shuffle=True, seed=0)
        state = {"epoch": epoch}

        def run():
            n = 0
            while n < args.batches:
                loader.set_epoch(state["epoch"])
                state["epoch"] += 1
                for batch in loader:
                    if consume is not None:
                        consume(batch)
                    n += 1
                    if n >= args.batches:
                        break
            return n
        return run

    def collate_pass(B, epoch, consume=None):
        def run():
            idx = DeviceLoader(store, batch_size=B, shuffle=True, seed=0).indices(epoch)[: args.batches * B]
            n = 0
            for batch in ref.batches(idx, B):
                if consume is not None:
                    consume(batch)
                n += 1
            return n
        return run

    # ---- the loaders alone ---------------------------------------------------------------------------------------------------------
    for B in (14, 64):
        res = {"loader": [], "collate": []}
        loader_pass(B, 0)(); collate_pass(B, 0)()                                       # warm-up: code objects, allocator pools
        for rep in range(args.repeats):
            for key, make in (("loader", loader_pass), ("collate", collate_pass)):
                ms, n = timed(make(B, 1 + rep))
                res[key].append(ms / n)
        up = []
        for rep in range(args.repeats):                                                   # the epoch's one upload, host clock around a synchronise
            loader = DeviceLoader(store, batch_size=B, shuffle=True, seed=0)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            plan = loader.epoch_plan(rep); store.upload_plan(plan); torch.cuda.synchronize()
            up.append((time.perf_counter() - t0) * 1e3)
        lines += [f"B = {B:2d}  DeviceLoader          {summary(res['loader'])}",
                  f"B = {B:2d}  per-sample collate    {summary(res['collate'])}",
                  f"B = {B:2d}  epoch plan + upload   {summary(up)}   (ms per EPOCH of {len(plan.batches)} batches, host clock)", ""]
        print("\n".join(lines[-4:]), flush=True)

    # ---- in front of the training step ----------------------------------------------------------------------------------------------
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict
    cfg = dict(PRODUCTION_LEFTNET_CONFIG)
    for B in args.step_batch:
        dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0, condition_nf=1, device=dev)
        dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg), strict=True)
        dyn.nan_check = "async"
        tr = DDPMTrainer(dyn, timesteps=1000, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0), pos_only=True, host_sync=False)
        step = lambda batch: tr.training_step(batch)                                      # noqa: E731

        def prebuilt_pass(epoch):
            loader = DeviceLoader(store, batch_size=B, shuffle=True, seed=0)
            loader.set_epoch(epoch)
            batches = []
            for batch in loader:
                batches.append(batch)
                if len(batches) >= args.batches:
                    break

            def run():
                for batch in batches:
                    step(batch)
                return len(batches)
            return run
        saved = args.batches
        args.batches = 10
        loader_pass(B, 0, step)(); collate_pass(B, 0, step)()                             # warm-up
        args.batches = saved
        res = {"loader": [], "collate": [], "prebuilt": []}
        for rep in range(args.step_repeats):
            for key, make in (("prebuilt", lambda e: prebuilt_pass(e)), ("loader", lambda e: loader_pass(B, e, step)),
                              ("collate", lambda e: collate_pass(B, e, step))):
                ms, n = timed(make(1 + rep))
                res[key].append(ms / n)
        lines += [f"B = {B:2d}  training_step, batches built before the window   {summary(res['prebuilt'])}",
                  f"B = {B:2d}  training_step fed by DeviceLoader                {summary(res['loader'])}",
                  f"B = {B:2d}  training_step fed by the per-sample collate      {summary(res['collate'])}", ""]
        print("\n".join(lines[-4:]), flush=True)
        del tr, dyn
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
