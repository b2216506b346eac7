"""`DiffusionSampler.inpaint_sharded` with two gloo processes on the CPU: the sharding logic only (`inpaint` itself needs a GPU and is
stubbed, as tests/test_shard_gloo.py stubs `sample`).  Five reactions of unequal sizes, three objects of different sizes."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

SIZES = [3, 4, 2, 5, 6]                 # atoms per reaction of R and P; TS has one more each
SEED = 100


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _global_batch():
    sizes = torch.tensor(SIZES)
    frags = [sizes, sizes + 1, sizes]
    # xh_fixed[k][row] = [k, global row of object k, 0, ...]: a rank's slice shows where it came from
    xh = []
    for k, f in enumerate(frags):
        x = torch.zeros(int(f.sum()), 9)
        x[:, 0] = float(k)
        x[:, 1] = torch.arange(int(f.sum())).float()
        xh.append(x)
    return frags, xh


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oareactdiff_amd.sampler import DiffusionSampler
        seen = {}

        class Stub(DiffusionSampler):
            def __init__(self):
                self.node_nfs = [9, 9, 9]

            def inpaint(self, n, frags, conditions=None, xh_fixed=None, **kw):
                seed = torch.initial_seed()
                assert conditions.shape[0] == n and all(x.shape[0] == int(f.sum()) for x, f in zip(xh_fixed, frags))
                seen.update(n=n, frags=[f.tolist() for f in frags], cond=conditions[:, 0].tolist(), kw=kw,
                            rows=[x[:, 1].tolist() for x in xh_fixed], objs=[x[:, 0].tolist() for x in xh_fixed])
                # every returned row carries (seed, the global row it was made from)
                outs = [torch.cat([torch.full((x.shape[0], 1), float(seed)), x[:, 1:2], torch.zeros(x.shape[0], 7)], dim=1) for x in xh_fixed]
                return [outs], [torch.repeat_interleave(torch.arange(n), f) for f in frags]
        frags, xh = _global_batch()
        given = [x.clone() for x in xh]
        cond = torch.arange(5).float().view(5, 1)
        out, masks, (lo, hi) = Stub().inpaint_sharded(frags, xh, conditions=cond, seed=SEED, gather=True, frag_fixed=[0, 2], resamplings=2)
        assert all(torch.equal(a, b) for a, b in zip(given, xh))
        q.put((rank, lo, hi, seen, [tuple(o.shape) for o in out[0]], [o[:, 0].tolist() for o in out[0]], [o[:, 1].tolist() for o in out[0]],
               [m.tolist() for m in masks]))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_inpaint_sharded_splits_the_global_batch_and_gathers_on_rank0():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    frags, _ = _global_batch()
    spans = [(0, 3), (3, 5)]
    for rank, lo, hi, seen, shapes, seeds, rows, masks in got:
        assert (lo, hi) == spans[rank]
        assert seen["n"] == hi - lo and seen["cond"] == [float(i) for i in range(lo, hi)]
        assert seen["kw"] == dict(frag_fixed=[0, 2], resamplings=2)          # everything else goes to inpaint as given
        for k, f in enumerate(frags):
            off = [0] + torch.cumsum(f, 0).tolist()
            assert seen["frags"][k] == f[lo:hi].tolist()
            assert seen["rows"][k] == [float(i) for i in range(off[lo], off[hi])], f"rank {rank} object {k}: not its slice of xh_fixed"
            assert seen["objs"][k] == [float(k)] * (off[hi] - off[lo])
            assert masks[k] == torch.repeat_interleave(torch.arange(hi - lo), f[lo:hi]).tolist()
    _, _, _, _, sh0, seeds0, rows0, _ = got[0]
    _, _, _, _, sh1, seeds1, rows1, _ = got[1]
    assert sh0 == [(20, 9), (25, 9), (20, 9)]                 # rank 0 holds the gathered batch (all 5 reactions)
    assert sh1 == [(11, 9), (13, 9), (11, 9)]                 # rank 1 keeps its own slice
    for k, f in enumerate(frags):
        n0 = int(f[:3].sum())
        assert rows0[k] == [float(i) for i in range(int(f.sum()))]                              # batch order
        assert seeds0[k] == [float(SEED)] * n0 + [float(SEED + 1)] * (int(f.sum()) - n0)        # seed + rank
        assert seeds1[k] == [float(SEED + 1)] * (int(f.sum()) - n0)
        assert rows1[k] == [float(i) for i in range(n0, int(f.sum()))]
