"""Cost of the all-pairs RMSD matrix: `oard_pairwise_rmsd` beside the route to the same matrix without it.

Workload: R groups (reactions) of K members (candidates) of 23 atoms with species counts (7, 12, 2, 2), stored candidate-major; every
member is its group's base conformer moved rigidly, with noise of 0.05 of the 1.5 spread, like atoms shuffled; reflection allowed.
Two routes, same-order and matched each, through the C ABI with every argument prepared beforehand:
    pairwise   oard_pairwise_rmsd on the one coordinate array: two launches (diagonal, pairs), K x K matrices out
    gathered   an explicit gather of the R K (K - 1) / 2 pairs into two arrays that line up row for row (index_select with index
               tensors made beforehand; coordinates, and species for the matched mode), then oard_kabsch_rmsd / oard_matched_rmsd:
               [pairs] values out (scattering them into matrices is NOT counted)
The two routes are alternated in one run; each sample is device events around `--inner` back-to-back calls, `--repeats` samples after
a warm-up.  One JSON line per route and mode with the median, min, max and the spread (max - min) / median, then the ratios of the
medians.  The values of the two routes are compared bit for bit before anything is timed.

    python tools/time_pairwise_rmsd.py --groups 64 --members 32
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COUNTS = (7, 12, 2, 2)


def workload(R, K, seed):
    """-> x [K R n, 3] float32, species [K R n] int32 (numpy), candidate-major: segment k * R + r is member k of group r."""
    import _kabsch_cases as kc
    import _match_cases as mc
    rng = np.random.default_rng(seed)
    n = int(sum(COUNTS))
    sp0 = np.repeat(np.array(mc.LABELS[:len(COUNTS)]), COUNTS)
    base = 1.5 * rng.standard_normal((R, n, 3))
    x, sp = np.empty((K, R, n, 3), np.float32), np.empty((K, R, n), np.int32)
    for k in range(K):
        for r in range(R):
            perm = np.arange(n)
            for idx in mc.blocks(sp0):
                perm[idx] = idx[rng.permutation(len(idx))]
            x[k, r] = base[r][perm] @ kc.random_rotation(rng).T + 3.0 * rng.standard_normal(3) + 0.05 * rng.standard_normal((n, 3))
            sp[k, r] = sp0[perm]
    return x.reshape(-1, 3), sp.reshape(-1), n


def sample(fn, inner):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(inner):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / inner


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    from oareactdiff_amd import _capi
    L = _capi.lib()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    R, K = args.groups, args.members
    xs, sps, n = workload(R, K, 0)
    x, sp = torch.from_numpy(xs).to(dev), torch.from_numpy(sps).to(dev)
    S, P = K * R, R * K * (K - 1) // 2
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    seg = torch.arange(S + 1, dtype=torch.int32, device=dev) * n
    members = i32([k * R + r for r in range(R) for k in range(K)])
    group_ptr = i32([g * K for g in range(R + 1)])
    pair_ptr, mat_ptr = i64([g * K * (K - 1) // 2 for g in range(R + 1)]), i64([g * K * K for g in range(R + 1)])
    out = torch.empty(R * K * K, device=dev)
    status = torch.empty(R * K * K, dtype=torch.int32, device=dev)
    # the gathered route: rows of member i (as a) and of member j (as b) for every pair, in the pair order of the matrix
    pairs = [(k_i * R + r, k_j * R + r) for r in range(R) for k_i in range(K) for k_j in range(k_i + 1, K)]
    rows = np.arange(n)
    ia = i64(np.concatenate([s * n + rows for s, _ in pairs]))
    ib = i64(np.concatenate([s * n + rows for _, s in pairs]))
    pseg = torch.arange(P + 1, dtype=torch.int32, device=dev) * n
    vals = torch.empty(P, device=dev)
    pstatus = torch.empty(P, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def pairwise(mode):
        _capi.check(L.oard_pairwise_rmsd(x.data_ptr(), 3, sp.data_ptr(), seg.data_ptr(), S, members.data_ptr(), group_ptr.data_ptr(),
                                         pair_ptr.data_ptr(), mat_ptr.data_ptr(), R, P, S, 1 | (2 if mode else 0), 0.0, 10000, out.data_ptr(),
                                         status.data_ptr(), stream), "oard_pairwise_rmsd")

    def gathered(mode):
        a, b = x.index_select(0, ia), x.index_select(0, ib)
        if mode:
            sa, sb = sp.index_select(0, ia), sp.index_select(0, ib)
            _capi.check(L.oard_matched_rmsd(a.data_ptr(), 3, b.data_ptr(), 3, sa.data_ptr(), sb.data_ptr(), pseg.data_ptr(), P, 1, 0.0, 10000,
                                            vals.data_ptr(), None, None, None, pstatus.data_ptr(), stream), "oard_matched_rmsd")
        else:
            _capi.check(L.oard_kabsch_rmsd(a.data_ptr(), 3, b.data_ptr(), 3, pseg.data_ptr(), P, 1, 0.0, vals.data_ptr(), None, None, stream),
                        "oard_kabsch_rmsd")
    upper = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev), 1)
    med = {}
    for mode, name in ((0, "same_order"), (1, "matched")):
        pairwise(mode)
        gathered(mode)
        torch.cuda.synchronize()
        m = out.view(R, K, K)
        assert torch.equal(m[:, upper].reshape(-1).view(torch.int32), vals.view(torch.int32)), "the two routes differ"
        assert torch.equal(m, m.transpose(1, 2)) and bool((m.diagonal(dim1=1, dim2=2) == 0).all())
        if mode:
            assert bool((pstatus == 1).all()), "the 23-atom pairs did not take the search branch"
        for _ in range(args.warmup):
            pairwise(mode)
            gathered(mode)
        torch.cuda.synchronize()
        ms = {"pairwise": [], "gathered": []}
        for _ in range(args.repeats):                           # alternated: drift of the clocks hits both alike
            ms["pairwise"].append(sample(lambda: pairwise(mode), args.inner))
            ms["gathered"].append(sample(lambda: gathered(mode), args.inner))
        for route, v in ms.items():
            med[(name, route)] = statistics.median(v)
            print(json.dumps({"mode": name, "route": route, "groups": R, "members": K, "pairs": P, "ms_per_call_median": round(med[(name, route)], 4),
                              "ms_per_call_min": round(min(v), 4), "ms_per_call_max": round(max(v), 4),
                              "spread": round((max(v) - min(v)) / med[(name, route)], 4), "inner": args.inner, "repeats": args.repeats}),
                  flush=True)
    print(json.dumps({f"{name}_gathered_over_pairwise": round(med[(name, "gathered")] / med[(name, "pairwise")], 3)
                      for name in ("same_order", "matched")}), flush=True)


if __name__ == "__main__":
    main()
