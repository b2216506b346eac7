"""`DDPMTrainer.validation_step` / `test_step` / `validation_epoch_end` on the path that cannot fuse (CPU): the row and the epoch's dict
from `DiffusionLoss(training=False)`, against the reference's recorded evaluation run; the nanmean over batches, the pooled mean over
reactions, the empty dict; and two gloo ranks with different batches returning the dict one process computes over both."""
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

import _vlb_cases as vc

T = 50
SIZES = [3, 4, 2, 5]                  # reactions 0 .. 2 are rank 0's batch, reaction 3 rank 1's: unequal batch sizes
SPLIT = 3
T_INT = [7.0, 1.0, 50.0, 23.0]


class ReplayModule(nn.Module):
    """The reference's recorded network outputs behind a module with one (unused) trainable parameter, which is what DDPMTrainer lays
    its flat state out over."""
    pos_dim, node_nfs = 3, [9, 9, 9]

    def __init__(self, z, dtype):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4, dtype=dtype))
        self.replay = vc.Replay(z, dtype)

    def forward(self, **kw):
        return self.replay(**kw)


def _golden_trainer(name, dtype=torch.float32):
    from oareactdiff_amd.trainer import DDPMTrainer
    z, meta = vc.load_golden(name)
    tr = DDPMTrainer(ReplayModule(z, dtype), timesteps=meta["T"], precision=1e-5, norm_values=meta["norm_values"], pos_only=meta["pos_only"])
    B = len(meta["sizes"])
    batch = (vc.golden_reps(z, dtype), torch.zeros(B, 1, dtype=dtype))
    kw = lambda: dict(t_int=torch.tensor(meta["t_int"], dtype=dtype).view(-1, 1), draw=vc.golden_draws(z, meta, dtype))      # noqa: E731
    return tr, z, meta, batch, kw


@pytest.mark.parametrize("name", ["g8_loss_eval", "g8_loss_eval_posonly"])
def test_val_totloss_is_the_recorded_mean_nll(name):
    """The unfused path with the reference's float32 network outputs replayed: test_loss.py's float32 gate (rtol 2e-5, atol 2e-4)."""
    tr, z, meta, batch, kw = _golden_trainer(name)
    assert not tr.fused and not tr._can_eval_fused()
    row = tr.validation_step(batch, **kw())
    assert row.shape == (1 + 3 + 3 + 2,) and bool(torch.isnan(row[-2:]).all())
    out = tr.validation_epoch_end()
    want = torch.from_numpy(z["f32_nll"]).double()
    assert math.isclose(out["val-totloss"], float(want.mean()), rel_tol=2e-5, abs_tol=2e-4)
    assert math.isclose(out["val-pooled-totloss"], float(want.mean()), rel_tol=2e-5, abs_tol=2e-4)
    width = 3 if meta["pos_only"] else 12
    scales = (1.0, 1.0, 1.0)                               # DDPMTrainer's default
    for k in range(3):
        e = torch.from_numpy(z[f"f32_error_t{k}"]).double()
        assert math.isclose(out[f"val-unorm_error_t_{k}"], float(e.mean()), rel_tol=2e-5, abs_tol=2e-4)
        e_n = float((e / (width * batch[0][k]["size"]) * scales[k]).mean() / (scales[k] + 1e-4))
        assert math.isclose(out[f"val-error_t_{k}"], e_n, rel_tol=2e-5, abs_tol=2e-4)
    assert math.isnan(out["val-rmsd"]) and math.isnan(out["val-rmsd-median"])
    assert set(out) == {"val-" + k for k in ["totloss", "pooled-totloss", "rmsd", "rmsd-median"]
                        + [f"{p}error_t_{k}" for p in ("", "unorm_") for k in range(3)]}
    # eval_loss's table is the case helper's, and the row is compute_loss's info
    tr2, *_ = _golden_trainer(name)
    nll, terms = tr2.eval_loss(batch, **kw())
    tr3, *_ = _golden_trainer(name)
    ref = vc.vlb_table(tr3.loss, batch[0], batch[1], **kw())
    assert torch.equal(nll, ref["nll"]) and torch.equal(terms, ref["terms"])
    tr4, *_ = _golden_trainer(name)
    nll4, info = tr4.compute_loss(batch, training=False, **kw())
    assert torch.equal(nll4, nll)
    assert row[0] == nll.mean() and all(float(row[1 + k]) == pytest.approx(info[f"error_t_{k}"], rel=1e-6) for k in range(3))
    assert all(float(row[4 + k]) == pytest.approx(info[f"unorm_error_t_{k}"], rel=1e-6) for k in range(3))


class ZeroModule(nn.Module):
    """A network that predicts zero noise: the aggregation below does not care what the loss is."""
    pos_dim, node_nfs = 3, [9, 9, 9]

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(4, dtype=torch.float64))

    def forward(self, xh, **kw):
        return [torch.zeros_like(x) for x in xh], None


def test_epoch_end_nanmean_pooled_mean_prefixes_and_the_empty_dict():
    from oareactdiff_amd.trainer import DDPMTrainer
    tr = DDPMTrainer(ZeroModule(), timesteps=T, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0))
    assert tr.validation_epoch_end() == {}
    state = {k: v.clone() for k, v in tr.dynamics.state_dict().items()}
    training = tr.dynamics.training
    torch.manual_seed(3)
    big, small = _val_batch(0, SPLIT)[0], _val_batch(SPLIT, len(SIZES))[0]           # 3 reactions and 1: unequal batch sizes
    rows = [tr.validation_step(big).clone(), tr.validation_step(small).clone()]      # t_int and the noise drawn by the trainer
    nlls = [x.clone() for x in tr._val_kept["val"][1]]
    assert [x.numel() for x in nlls] == [3, 1] and rows[0].shape == (9,)
    test_row = tr.test_step(big)
    # a NaN entry in one batch's row: the mean skips it (every batch's rmsd is NaN: that mean is NaN)
    tr._val_kept["val"][0][1] = rows[1].clone()
    tr._val_kept["val"][0][1][2] = float("nan")
    out = tr.validation_epoch_end()
    assert out["val-totloss"] == pytest.approx(float((rows[0][0] + rows[1][0]) / 2), rel=1e-14)
    assert out["val-pooled-totloss"] == pytest.approx(float(torch.cat(nlls).mean()), rel=1e-14)
    assert abs(out["val-pooled-totloss"] - out["val-totloss"]) > 1e-6 * abs(out["val-totloss"])       # not the mean of batch means
    assert out["val-error_t_1"] == pytest.approx(float(rows[0][2]), rel=1e-14)
    assert out["val-error_t_0"] == pytest.approx(float((rows[0][1] + rows[1][1]) / 2), rel=1e-14)
    assert math.isnan(out["val-rmsd"]) and math.isnan(out["val-rmsd-median"])
    assert out["test-totloss"] == pytest.approx(float(test_row[0]), rel=1e-14)
    assert out["test-pooled-totloss"] == pytest.approx(out["test-totloss"], rel=1e-14)
    assert {k.split("-")[0] for k in out} == {"val", "test"} and len(out) == 2 * 10
    assert tr.validation_epoch_end() == {}                                   # forgotten
    # no state was touched
    assert tr.dynamics.training == training and all(torch.equal(v, state[k]) for k, v in tr.dynamics.state_dict().items())
    assert tr.skipped_steps == 0 and tr.gradnorm_queue.items == [3000]
    with pytest.raises(ValueError):
        tr.validation_step(big, weights="ema")                               # no ema_decay
    with pytest.raises(ValueError):
        tr.validation_step(big, weights="other")
    assert tr.validation_epoch_end() == {}


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------------------
def _val_batch(lo, hi):
    """Reactions [lo, hi) of a synthetic batch with this shard's rows of the whole batch's draws (both noise blocks)."""
    g = torch.Generator().manual_seed(11)
    B = len(SIZES)
    full_mask = torch.repeat_interleave(torch.arange(B), torch.tensor(SIZES))
    keep = (full_mask >= lo) & (full_mask < hi)
    n = full_mask.numel()
    reps = []
    for k in range(3):
        pos = torch.randn(n, 3, generator=g, dtype=torch.float64)
        typ = torch.randint(0, 4, (n,), generator=g)
        one_hot = torch.zeros(n, 5, dtype=torch.long)
        one_hot[torch.arange(n), typ] = 1
        charge = torch.tensor([1, 6, 7, 8])[typ].view(n, 1)
        reps.append({"size": torch.tensor(SIZES[lo:hi]), "pos": pos[keep], "one_hot": one_hot[keep], "charge": charge[keep],
                     "mask": full_mask[keep] - lo})
    draws = []
    for _ in range(2):
        for k in range(3):
            draws += [torch.randn(n, 3, generator=g, dtype=torch.float64)[keep], torch.randn(n, 6, generator=g, dtype=torch.float64)[keep]]
    it = iter(draws)
    t_int = torch.tensor(T_INT, dtype=torch.float64).view(-1, 1)[lo:hi]
    return (reps, torch.zeros(hi - lo, 1, dtype=torch.float64)), dict(t_int=t_int, draw=lambda shape: next(it))


def _trainer():
    from test_trainer_gloo import _oracle_dynamics
    from oareactdiff_amd.trainer import DDPMTrainer
    return DDPMTrainer(_oracle_dynamics(), timesteps=T, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0))


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tr = _trainer()
        assert tr.collectives
        batch, kw = _val_batch(0, SPLIT) if rank == 0 else _val_batch(SPLIT, len(SIZES))
        tr.validation_step(batch, **kw)
        q.put((rank, tr.validation_epoch_end()))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_with_different_batches_return_the_single_process_dict():
    from test_trainer_gloo import _free_port
    single = _trainer()
    for lo, hi in ((0, SPLIT), (SPLIT, len(SIZES))):
        batch, kw = _val_batch(lo, hi)
        single.validation_step(batch, **kw)
    want = single.validation_epoch_end()
    assert abs(want["val-pooled-totloss"] - want["val-totloss"]) > 1e-9 * abs(want["val-totloss"])
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    def same(a, b):
        return set(a) == set(b) and all((math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)
    assert same(got[0], got[1])                                              # every rank returns the same dict
    assert set(got[0]) == set(want)
    for k, v in want.items():
        assert (math.isnan(v) and math.isnan(got[0][k])) or got[0][k] == pytest.approx(v, rel=1e-12), k
