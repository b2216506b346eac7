"""Device time of the ranking metrics: `metrics.rank_metrics` (`oard_rank_metrics`, csrc/oard_rank.h) against the
same numbers from torch ops on the same device, and the cost of `ConfidenceTrainer(rank_metrics=True)` in a training step.

The torch-op form, written here: midranks from one sort and two `searchsorted` per array (rank = (#less + #less-or-equal + 1) / 2), the
sums in float64, every segment of a shape at once as one [G, K] batch - the favourable case for torch ops, no loop over segments and no
padding; it has no NaN handling and no ragged segments.  Before anything is timed its numbers are compared with the kernel's.
Shapes: n = 64 in one segment (a training batch), n = 16 384 in one segment (a pooled validation set), 4096 segments of K = 16
(candidates per reaction).  Scores are rounded to 1/64, so there are ties.  Each variant: `--warmup` calls, then `--repeats` windows of
`--inner` back-to-back calls between device events; median, minimum and maximum per call.  The two variants of a shape alternate window
by window.  The training step (tests/golden cg_ragged_h32, B = 3) is timed with a host clock around the step, which ends in its host
read, rank_metrics off and on alternating.

    python tools/time_rank_metrics.py
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))             # the fixtures' helpers import the oracle

SHAPES = [("n=64, one segment", 1, 64), ("n=16384, one segment", 1, 16384), ("4096 segments of K=16", 4096, 16)]


def torch_midrank(x):
    """x: [G, K] -> [G, K] float64 average ranks, 1-based."""
    s = torch.sort(x, dim=1).values
    less = torch.searchsorted(s, x, right=False)
    less_equal = torch.searchsorted(s, x, right=True)
    return (less + less_equal + 1).double() * 0.5


def torch_pearson(a, b):
    da, db = a - a.mean(dim=1, keepdim=True), b - b.mean(dim=1, keepdim=True)
    return (da * db).sum(1) / ((da * da).sum(1).sqrt() * (db * db).sum(1).sqrt())


def torch_rank_metrics(score, target):
    """[G, K] float32 each -> [G, 8] float64: the columns of oard_rank_metrics from torch ops."""
    K = score.shape[1]
    s64, t64 = score.double(), target.double()
    rs, rt = torch_midrank(score), torch_midrank(target)
    pos = target >= 0.5
    n_pos = pos.sum(1).double()
    n_neg = K - n_pos
    auroc = ((rs * pos).sum(1) - n_pos * (n_pos + 1) * 0.5) / (n_pos * n_neg)
    auroc = torch.where((n_pos > 0) & (n_neg > 0), auroc, torch.zeros_like(auroc))
    return torch.stack([torch.full_like(n_pos, K), n_pos, auroc, torch_pearson(s64, t64), torch_pearson(rs, rt),
                        (s64 - t64).abs().mean(1), s64.mean(1), t64.mean(1)], dim=1)


def windows(fns, args):
    """Alternating windows of the given callables -> one list of ms per call for each."""
    for fn in fns:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(args.repeats):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.inner):
                fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1) / args.inner)
    return ms


def line(what, ms, unit="us"):
    f = 1000.0 if unit == "us" else 1.0
    return f"{what:<58s} median {statistics.median(ms) * f:9.1f}  min {min(ms) * f:9.1f}  max {max(ms) * f:9.1f}  {unit} per call"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--steps", type=int, default=40, help="training steps per variant")
    args = ap.parse_args()
    from oareactdiff_amd import ConfidenceTrainer, _capi
    from oareactdiff_amd.metrics import rank_metrics
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = _capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(0)
    print(f"# rank metrics: {torch.cuda.get_device_name(dev)}; warmup {args.warmup}, {args.repeats} windows of {args.inner} calls")
    for what, G, K in SHAPES:
        n = G * K
        s = np.round(rng.standard_normal(n) * 64.0) / 64.0
        score = torch.tensor(s, dtype=torch.float32, device=dev)
        target = torch.tensor(rng.random(n) < 0.4, dtype=torch.float32, device=dev)
        sizes = torch.full((G,), K, dtype=torch.int64, device=dev)
        got = torch.stack(list(rank_metrics(score, target, sizes)), dim=1)
        ref = torch_rank_metrics(score.reshape(G, K), target.reshape(G, K))
        both = torch.isfinite(got) & torch.isfinite(ref)
        assert bool((torch.isfinite(got) == torch.isfinite(ref)).all()), "the two forms disagree on where a number is defined"
        gap = float((got[both] - ref[both]).abs().max())
        assert gap <= 1e-10, gap
        # the kernel alone: every argument prepared, a call is the library entry (two launches)
        seg_ptr = (torch.arange(G + 1, dtype=torch.int32, device=dev) * K).contiguous()
        rs, rt = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        out = torch.empty(G, 8, dtype=torch.float64, device=dev)

        def kernel():
            _capi.check(L.oard_rank_metrics(score.data_ptr(), target.data_ptr(), n, seg_ptr.data_ptr(), G, rs.data_ptr(), rt.data_ptr(),
                                            out.data_ptr(), stream), "oard_rank_metrics")
        s2, t2 = score.reshape(G, K), target.reshape(G, K)
        ms = windows([kernel, lambda: rank_metrics(score, target, sizes), lambda: torch_rank_metrics(s2, t2)], args)
        print(f"{what}  (kernel vs torch ops: largest difference {gap:.1e})")
        print(line("  oard_rank_metrics, arguments prepared", ms[0]))
        print(line("  metrics.rank_metrics (seg_ptr and outputs made per call)", ms[1]))
        print(line("  torch ops (sort + searchsorted, float64 sums)", ms[2]))
        print(f"  torch ops / metrics.rank_metrics: {statistics.median(ms[2]) / statistics.median(ms[1]):.2f}", flush=True)
    # ---- the training step ------------------------------------------------------------------------------------------------------------
    from _conf_grad_cases import ConfGradCase
    g = ConfGradCase("cg_ragged_h32")
    batch = g.batch(dev)
    trainers = [ConfidenceTrainer(g.module(dev), rank_metrics=on) for on in (False, True)]
    for tr in trainers:
        for _ in range(args.warmup):
            tr.training_step(batch)
    ms = [[], []]
    for _ in range(args.steps):
        for k, tr in enumerate(trainers):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.training_step(batch)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    print("ConfidenceTrainer.training_step on cg_ragged_h32 (B = 3), host clock around the step")
    print(line("  rank_metrics=False", ms[0], "ms"))
    print(line("  rank_metrics=True", ms[1], "ms"))
    print(f"  added by rank_metrics (difference of the medians): {(statistics.median(ms[1]) - statistics.median(ms[0])) * 1e3:.0f} us", flush=True)


if __name__ == "__main__":
    main()
