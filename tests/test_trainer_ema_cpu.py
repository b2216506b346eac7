"""DDPMTrainer(ema_decay=...) on the generic (autograd + torch.optim.AdamW) path, on the CPU: the oracle-backed EGNNDynamics of
tests/test_trainer_gloo.py as the denoiser.  What is under test is the trainer's bookkeeping of the average (trainer/ema.py:37-47 =
timm's ModelEmaV2.update after every batch): the recursion  ema = fl(fl(d32 ema) + fl(w32 p_new))  in the parameters' own precision
with d32 = float32(d), w32 = float32(1 - d), its start at the weights, its state dict, its broadcast across ranks - and the checkpoint
adapter's `weights="ema"`.  The module's parameters are float64 here (the oracle's), so the host recursion below runs in float64 with
the two float32 scalars: the same two rounded products and one rounded sum, hence bit equality."""
import os
import socket
import sys
import types
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_trainer_gloo import SIZES, T, _batch, _oracle_dynamics

DECAY = 0.9
KW = dict(timesteps=T, norm_values=(1.0, 4.0, 10.0), scales=(1.0, 2.0, 1.0))


def _trainer(**kw):
    from oareactdiff_amd.trainer import DDPMTrainer
    return DDPMTrainer(_oracle_dynamics(), **dict(KW, **kw))


def _one_step(tr, lo=0, hi=len(SIZES)):
    batch, t_int, draw = _batch(SIZES, lo, hi)
    return tr.training_step(batch, t_int=t_int, draw=draw)


def _weights(tr):
    return torch.cat([p.detach().reshape(-1) for p in tr.params]).numpy().copy()


def _recursion(e, p, decay):
    d32, w32 = np.float32(decay), np.float32(1.0 - decay)
    a = e.dtype.type(d32) * e
    b = e.dtype.type(w32) * p
    return a + b


def test_three_generic_steps_follow_the_recursion_bit_for_bit():
    tr = _trainer(ema_decay=DECAY)
    assert not tr.fused and tr.flat_ema.dtype == tr.params[0].dtype and tr.flat_ema.numel() == tr.flat_grad.numel()
    want = _weights(tr)
    assert np.array_equal(tr.flat_ema.numpy(), want)                    # ModelEmaV2.__init__: a copy of the weights
    twin = _trainer()
    assert twin.flat_ema is None
    for step in range(3):
        info = _one_step(tr)
        _one_step(twin)
        assert info["skipped"] == 0
        want = _recursion(want, _weights(tr), DECAY)
        assert np.array_equal(tr.flat_ema.numpy(), want), step
        assert np.array_equal(_weights(tr), _weights(twin)), "the average fed back into the weights"
    assert not np.array_equal(want, _weights(tr))
    # a skipped step (NaN noise) leaves the average where it was
    before = tr.flat_ema.clone()
    batch, t_int, draw = _batch(SIZES, 0, len(SIZES))
    info = tr.training_step(batch, t_int=t_int, draw=lambda shape: draw(shape) * float("nan"))
    assert info["skipped"] == 1 and torch.equal(tr.flat_ema, before)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            _trainer(ema_decay=bad)


def test_ema_state_dict_has_the_modules_keys_and_shapes():
    tr = _trainer(ema_decay=DECAY)
    _one_step(tr)
    sd, esd = tr.dynamics.state_dict(), tr.ema_state_dict()
    assert list(esd.keys()) == list(sd.keys()) and all(esd[k].shape == sd[k].shape and esd[k].dtype == sd[k].dtype for k in sd)
    trainable = set(tr.names)
    views = dict(zip(tr.names, tr._ema_views()))
    changed = 0
    for k in sd:
        if k in trainable:
            assert torch.equal(esd[k], views[k])
            changed += int(not torch.equal(esd[k], sd[k]))
        else:                                                           # buffers and the modules the forward never uses
            assert torch.equal(esd[k], sd[k])
    assert changed > 0.9 * len(trainable)
    fresh = _oracle_dynamics()
    fresh.load_state_dict(esd, strict=True)
    # the shadow module: same class and keys, trainable tensors inside flat_ema, nothing requires a gradient
    shadow = tr.ema_dynamics
    assert tr.ema_dynamics is shadow and type(shadow) is type(tr.dynamics)
    ssd = shadow.state_dict()
    assert list(ssd.keys()) == list(sd.keys()) and all(torch.equal(ssd[k], esd[k]) for k in sd)
    lo, hi = tr.flat_ema.data_ptr(), tr.flat_ema.data_ptr() + tr.flat_ema.numel() * tr.flat_ema.element_size()
    named = dict(shadow.named_parameters())
    assert all(lo <= named[k].data_ptr() < hi for k in trainable) and not any(p.requires_grad for p in shadow.parameters())
    live = dict(tr.dynamics.named_parameters())
    assert all(named[k].data_ptr() == live[k].data_ptr() for k in named if k not in trainable)
    _one_step(tr)                                                       # views: the shadow follows the buffer
    assert all(torch.equal(shadow.state_dict()[k], tr.ema_state_dict()[k]) for k in sd)
    tr.copy_ema_to_model()
    assert np.array_equal(_weights(tr), tr.flat_ema.numpy())
    with pytest.raises(RuntimeError):
        _trainer().ema_state_dict()


def test_resume_round_trip_and_states_without_an_average():
    a = _trainer(ema_decay=DECAY)
    _one_step(a); _one_step(a)
    msd = {k: v.clone() for k, v in a.dynamics.state_dict().items()}
    tsd = a.state_dict()
    assert tsd["ema_decay"] == DECAY and torch.equal(tsd["ema"], a.flat_ema) and tsd["ema"].data_ptr() != a.flat_ema.data_ptr()
    _one_step(a)
    b = _trainer(ema_decay=DECAY)
    b.dynamics.load_state_dict(msd, strict=True)
    b.load_state_dict(tsd)
    assert torch.equal(b.flat_ema, tsd["ema"])
    _one_step(b)
    assert torch.equal(a.flat_ema, b.flat_ema) and np.array_equal(_weights(a), _weights(b))
    # EMA off: exactly the keys the state had before the average existed, and a saved average is ignored
    off = _trainer()
    assert set(off.state_dict()) == {"fused", "names", "skipped_steps", "gradnorm_queue", "optimizer"}
    _one_step(off); _one_step(off)
    off.load_state_dict(tsd)
    assert off.flat_ema is None
    # a state without an average into a trainer that keeps one: the average restarts from the weights, with one warning
    c = _trainer(ema_decay=DECAY)
    c.dynamics.load_state_dict(msd, strict=True)
    old = {k: v for k, v in tsd.items() if k not in ("ema", "ema_decay")}
    with pytest.warns(UserWarning, match="EMA"):
        c.load_state_dict(old)
    assert np.array_equal(c.flat_ema.numpy(), _weights(c))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c.load_state_dict(old)                                         # warned once


# ---- two gloo ranks ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    from oareactdiff_amd.shard import shard_range
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dyn = _oracle_dynamics()
        if rank > 0:                                                    # a replica built differently: the average starts AFTER sync_replicas
            with torch.no_grad():
                for p in dyn.parameters():
                    p.add_(0.1)
        from oareactdiff_amd.trainer import DDPMTrainer
        tr = DDPMTrainer(dyn, ema_decay=DECAY, **KW)
        start = tr.flat_ema.numpy().copy()
        lo, hi = shard_range(len(SIZES), rank, world)
        for _ in range(2):
            _one_step(tr, lo, hi)
        after = tr.flat_ema.numpy().copy()
        tr.flat_ema.add_(float(rank))                                   # ... and sync_replicas carries rank 0's average to everyone
        tr.sync_replicas()
        q.put((rank, start, after, _weights(tr), tr.flat_ema.numpy().copy()))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_keep_identical_averages_equal_to_the_single_process():
    single = _trainer(ema_decay=DECAY)
    start1 = single.flat_ema.numpy().copy()
    _one_step(single); _one_step(single)
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted((q.get(timeout=300) for _ in range(2)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, s0, e0, w0, b0), (_, s1, e1, w1, b1) = out
    assert np.array_equal(s0, start1) and np.array_equal(s1, start1)    # rank 1's perturbed weights never reached its average
    assert np.array_equal(e0, e1) and np.array_equal(w0, w1)            # bit-identical across the ranks
    assert np.array_equal(b0, e0) and np.array_equal(b1, e0)            # sync_replicas broadcasts rank 0's average
    # ... and the single process's to the degree the weights are (tests/test_trainer_gloo.py: 1e-12 after a step; the average is a
    # convex combination of weights, so the same bound holds for it)
    assert float(np.abs(w0 - _weights(single)).max()) <= 1e-12
    assert float(np.abs(e0 - single.flat_ema.numpy()).max()) <= 1e-12


# ---- checkpoint adapter -----------------------------------------------------------------------------------------------------------------
def _write_ckpt(path, sd, cfg, node_nfs, cnf, ema_sd):
    """A Lightning-style file written the way tests/test_checkpoint.py writes its own (stand-in classes under the reference's module
    paths, removed again before loading); `ema_sd`: the `state_dict()` of the reference's EMACallback (ema.py:73-75) or None."""
    created = []

    def module(name):
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            n = ".".join(parts[:i])
            if n not in sys.modules:
                sys.modules[n] = types.ModuleType(n)
                created.append(n)
        return sys.modules[name]
    leftnet = module("oa_reactdiff.model.leftnet")

    class LEFTNet(torch.nn.Module):
        pass
    LEFTNet.__module__, LEFTNet.__qualname__ = "oa_reactdiff.model.leftnet", "LEFTNet"
    leftnet.LEFTNet = LEFTNet
    callbacks = {"ModelCheckpoint{'monitor': 'val-totloss'}": {"best_model_score": torch.tensor(1.5)}}
    if ema_sd is not None:
        callbacks["EMACallback"] = {"state_dict_ema": OrderedDict(("ddpm.dynamics." + k, v) for k, v in ema_sd.items())}
        callbacks["EMACallback"]["state_dict_ema"]["ddpm.schedule.gamma_module.gamma"] = torch.linspace(-5, 5, 11)
    ckpt = {"epoch": 3, "global_step": 12, "pytorch-lightning_version": "2.0.4",
            "state_dict": {"ddpm.dynamics." + k: v for k, v in sd.items()}, "callbacks": callbacks,
            "hyper_parameters": dict(model_config=dict(cfg), node_nfs=list(node_nfs), edge_nf=0, condition_nf=cnf, fragment_names=["R", "TS", "P"],
                                     pos_dim=3, update_pocket_coords=True, condition_time=True, edge_cutoff=None, model=LEFTNet,
                                     enforce_same_encoding=None)}
    torch.save(ckpt, path)
    for n in created:
        del sys.modules[n]


def test_load_checkpoint_takes_the_callbacks_average(tmp_path):
    from _cases import Case
    from oareactdiff_amd.checkpoint import load_checkpoint
    c = Case("g3_cutoff_ragged")
    sd = c.state_dict()
    ema_sd = OrderedDict((k, v + 0.25 if v.is_floating_point() and "radial_emb" not in k else v.clone()) for k, v in sd.items())
    cpu = torch.device("cpu")
    with_ema, without = os.path.join(tmp_path, "ema.ckpt"), os.path.join(tmp_path, "plain.ckpt")
    _write_ckpt(with_ema, sd, c.cfg, c.node_nfs, c.cnf, ema_sd)
    _write_ckpt(without, sd, c.cfg, c.node_nfs, c.cnf, None)
    dyn, hp = load_checkpoint(with_ema, device=cpu, weights="ema")
    got = dyn.state_dict()
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], ema_sd[k]) for k in sd)
    assert hp["node_nfs"] == list(c.node_nfs)
    live = load_checkpoint(with_ema, device=cpu)[0].state_dict()         # the default is unchanged: the model's own weights
    assert all(torch.equal(live[k], sd[k]) for k in sd) and any(not torch.equal(live[k], got[k]) for k in sd)
    with pytest.raises(KeyError, match="EMA"):
        load_checkpoint(without, device=cpu, weights="ema")
    assert all(torch.equal(load_checkpoint(without, device=cpu)[0].state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        load_checkpoint(with_ema, device=cpu, weights="average")
    assert "oa_reactdiff" not in sys.modules
