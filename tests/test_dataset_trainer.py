"""The trainers on `DeviceLoader` batches: a `DDPMTrainer` step on a loader batch is bit for bit the step on the same batch built through
`DDPMTrainer.to_device` from host tensors; a `ConfidenceTrainer` step takes a `confidence_model` batch; an epoch of loader batches and
steps reads nothing from the device beyond the step's own read under `host_sync=True`."""
import pytest
import torch

from _dataset_cases import PROPS, DatasetCase
from _grad_cases import CNF, NODE_NFS, GradCase

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _trainer(c, **kw):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.trainer import DDPMTrainer
    dyn = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0, condition_nf=CNF, device=DEV)
    dyn.load_state_dict(c.state_dict(), strict=True)
    return DDPMTrainer(dyn, timesteps=c.meta["T"], norm_values=c.meta["norm_values"], scales=(1.0, 2.0, 1.0), pos_only=True, fused=True, **kw)


def _draws(seed):
    """The injected `draw` of tests/test_trainer_fused.py for shapes no fixture recorded: a seeded host stream, re-made per run."""
    g = torch.Generator().manual_seed(seed)
    return lambda shape: torch.randn(tuple(shape), generator=g).to(DEV)


def _host_copy(batch):
    reps, cond = batch
    return [{p: r[p].cpu() for p in PROPS} for r in reps], cond.cpu()


def _count_device_reads(monkeypatch, fn):
    """Calls `fn` and counts the device -> host reads made through the tensor methods that make them."""
    counts = {}
    for name in ("tolist", "item", "cpu", "numpy", "__bool__", "__int__", "__float__", "__index__"):
        inner = getattr(torch.Tensor, name)

        def wrapped(self, *a, _inner=inner, _name=name, **k):
            if self.is_cuda:
                counts[_name] = counts.get(_name, 0) + 1
            return _inner(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    out = fn()
    monkeypatch.undo()
    return out, counts


def test_step_on_a_loader_batch_is_bitwise_the_step_on_the_host_built_batch():
    from oareactdiff_amd.data import DeviceLoader
    from oareactdiff_amd.trainer import DDPMTrainer
    c = GradCase("g9_grad_h32")
    store = DatasetCase("swap_by_ind").store(DEV)          # production switches; molecules of 1, 2, 23, 64, 65 atoms
    loader = DeviceLoader(store, batch_size=3, shuffle=True, seed=4)
    batches = list(loader)
    B = 3
    t_int = torch.tensor([[0.0], [float(c.meta["T"]) // 2], [float(c.meta["T"])]], device=DEV)
    runs = {}
    for key in ("loader", "host"):
        tr = _trainer(c)
        infos = []
        for i, batch in enumerate(batches[:2]):
            assert batch[0][0]["size"].numel() == B
            if key == "host":
                batch = DDPMTrainer.to_device(_host_copy(batch), DEV, non_blocking=False)
            infos.append(tr.training_step(batch, t_int=t_int, draw=_draws(100 + i)))
        torch.cuda.synchronize()
        runs[key] = (infos, tr.flat_param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone())
    assert runs["loader"][0] == runs["host"][0]
    assert all(i["skipped"] == 0 for i in runs["loader"][0])
    for a, b in zip(runs["loader"][1:], runs["host"][1:]):
        assert torch.equal(a, b)
    assert not torch.equal(runs["loader"][1], _trainer(c).flat_param)          # the steps moved the weights


def test_confidence_trainer_takes_a_confidence_batch():
    from oareactdiff_amd import ConfidenceTrainer
    from oareactdiff_amd.confidence import Confidence
    from oareactdiff_amd.data import DeviceLoader
    from oareactdiff_amd.spec import confidence_state_spec, synthetic_state_dict
    c = GradCase("g9_grad_h32")
    m = Confidence(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0, condition_nf=CNF, device=DEV,
                   trainable=True)
    m.load_state_dict(synthetic_state_dict(confidence_state_spec(c.cfg, NODE_NFS, CNF), c.cfg, seed=42, dtype=torch.float32), strict=True)
    tr = ConfidenceTrainer(m, target_key="target")
    store = DatasetCase("confidence").store(DEV)
    before = tr.flat_param.clone()
    for reps, res in DeviceLoader(store, batch_size=3):
        assert set(res) == {"target", "rmsd", "condition"} and res["target"].shape == (3,) and res["condition"].shape == (3, 1)
        info = tr.training_step((reps, res))
        assert info["skipped"] == 0 and info["loss"] == info["loss"] and "acc" in info
    assert not torch.equal(before, tr.flat_param)


def test_an_epoch_of_loader_batches_and_steps_reads_nothing_from_the_device(monkeypatch):
    from oareactdiff_amd.data import DeviceLoader
    from oareactdiff_amd.trainer import DDPMTrainer
    c = GradCase("g9_grad_h32")
    store = DatasetCase("swap_by_ind").store(DEV)
    loader = DeviceLoader(store, batch_size=3, shuffle=True, seed=1)
    torch.manual_seed(0)

    def epoch(tr, e, through_host=False):
        loader.set_epoch(e)
        n = 0
        for batch in (host_batches if through_host else loader):
            tr.training_step(batch)
            n += 1
        return n
    tr = _trainer(c, host_sync=False)
    epoch(tr, 0)                                           # warm: streams, pools, first topologies
    steps, reads = _count_device_reads(monkeypatch, lambda: epoch(tr, 1))
    print(f"host_sync=False: {steps} loader batches + steps, device -> host reads {reads}")
    assert steps == len(loader) == 4 and reads == {}
    # host_sync=True: exactly the reads the same steps make on batches that came through DDPMTrainer.to_device from host tensors
    loader.set_epoch(2)
    host_batches = [DDPMTrainer.to_device(_host_copy(b), DEV, non_blocking=False) for b in loader]
    counted = {}
    for key in ("host", "loader"):
        tr = _trainer(c, host_sync=True)
        torch.manual_seed(3)
        epoch(tr, 0)
        _, counted[key] = _count_device_reads(monkeypatch, lambda: epoch(tr, 2, through_host=(key == "host")))
    print(f"host_sync=True: reads per epoch of {len(loader)} steps: {counted}")
    assert counted["loader"] == counted["host"] and sum(counted["loader"].values()) == len(loader)
