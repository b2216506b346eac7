"""One Confidence call beside one denoiser call on the headline batch (B = 64 reactions x 3 objects x 23 atoms, production widths),
both timed with HIP events on the same build:  python tools/confidence_time.py [--b 64] [--n 23] [--iters 20]
--train: one `ConfidenceTrainer.training_step` beside one `DDPMTrainer.training_step` (host-sync, one micro-batch) on the same batch.
Prints one JSON line (DESIGN.md quotes it)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oareactdiff_amd import Confidence, EGNNDynamics, get_edges_index, get_mask_for_frag, get_n_frag_switch  # noqa: E402
from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, confidence_state_spec, state_spec, synthetic_state_dict  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def train_mode(a, dev):
    """One training step of either trainer on one fixed batch, alternating, three blocks each (wall time between HIP events: a step
    ends with its host read)."""
    from bench import make_training_batch
    from oareactdiff_amd import ConfidenceTrainer, DDPMTrainer
    cfg, node_nfs, cnf = dict(PRODUCTION_LEFTNET_CONFIG), [9, 9, 9], 1
    reps, cond = make_training_batch(a.b, a.n, 100, dev)
    labels = (torch.arange(a.b, device=dev) % 2).float()
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
    dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, node_nfs, cnf), cfg), strict=True)
    conf = Confidence(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=dev,
                      trainable=True)
    conf.load_state_dict(synthetic_state_dict(confidence_state_spec(cfg, node_nfs, cnf), cfg), strict=True)
    ddpm = DDPMTrainer(dyn, norm_values=(1.0, 4.0, 10.0), pos_only=True)
    ctr = ConfidenceTrainer(conf)
    rounds = []
    for _ in range(3):
        rounds.append(timed(lambda: ddpm.training_step((reps, cond)), a.iters) +
                      timed(lambda: ctr.training_step((reps, {"condition": cond, "rmsd": labels})), a.iters))
    col = lambda i: [round(r[i], 4) for r in rounds]
    print(json.dumps(dict(mode="train", batch=a.b, atoms_per_object=a.n, iters=a.iters, denoiser_step_ms_median=col(0),
                          denoiser_step_ms_min=col(1), confidence_step_ms_median=col(2), confidence_step_ms_min=col(3),
                          trained_parameters=dict(denoiser=int(ddpm.flat_grad.numel()), confidence=int(ctr.n_params)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=64)
    ap.add_argument("--n", type=int, default=23)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--train", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        return train_mode(a, dev)
    cfg, node_nfs, cnf = dict(PRODUCTION_LEFTNET_CONFIG), [9, 9, 9], 1
    frag = [torch.full((a.b,), a.n, dtype=torch.long) for _ in range(3)]
    cm = torch.cat([get_mask_for_frag(f) for f in frag]).to(dev)
    nfs, ei = get_n_frag_switch(frag).to(dev), get_edges_index(cm, remove_self_edge=True)
    g = torch.Generator().manual_seed(0)
    xh = []
    for f in frag:
        n = int(f.sum())
        onehot = torch.nn.functional.one_hot(torch.randint(0, 5, (n,), generator=g), 5).float()
        xh.append(torch.cat([torch.randn(n, 3, generator=g), onehot, torch.randint(1, 9, (n, 1), generator=g).float()], dim=1).to(dev))
    cond, t = torch.zeros(a.b, 1, device=dev), torch.zeros(1, device=dev)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
    dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, node_nfs, cnf), cfg), strict=True)
    conf = Confidence(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
    conf.load_state_dict(synthetic_state_dict(confidence_state_spec(cfg, node_nfs, cnf), cfg), strict=True)
    dyn.nan_check = "async"
    dyn.edge_precision = conf.edge_precision = a.precision
    rounds = []                                                             # the two calls alternate, three blocks each: the spread shows
    with torch.no_grad():
        for _ in range(3):
            rounds.append(timed(lambda: dyn(xh, ei, t, cond, nfs, cm), a.iters) + timed(lambda: conf._forward(xh, ei, t, cond, nfs, cm), a.iters))
    col = lambda i: [round(r[i], 4) for r in rounds]
    print(json.dumps(dict(batch=a.b, atoms_per_object=a.n, precision=a.precision or "f32", iters=a.iters,
                          forward_ms_median=col(0), forward_ms_min=col(1), confidence_ms_median=col(2), confidence_ms_min=col(3))))


if __name__ == "__main__":
    main()
