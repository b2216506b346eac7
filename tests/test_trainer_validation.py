"""`DDPMTrainer.eval_loss` / `validation_step` / `validation_epoch_end` on the device: the two evaluation kernels with the HIP network in
the loop against the reference's recorded float64 evaluation runs (tests/golden/g8_loss_eval*.npz) and against the unfused formulation
(`DiffusionLoss(training=False)` on the same draws), on the fixtures and off them; EMA weights; no training state touched; host reads;
independence of the module's workspace.

Gates on the fixtures are those of test_loss.py::test_loss_with_hip_dynamics_matches_reference_f64: 1e-5 of the largest entry per term
(at least 1), 2e-5 on nll relative to max(|ref|, 1).  Off the fixtures the fused and the unfused path run the same HIP network on inputs
that agree to float32 rounding and differ in the float32 loss arithmetic only, so the same two gates apply."""
import pytest
import torch

import _vlb_cases as vc

pytestmark = pytest.mark.gpu

NARROW = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
BLOCKS = ("error_t normalised", "error_t", "loss_0_x", "loss_0_cat", "loss_0_charge")


def _dev():
    return torch.device("cuda:0")


def _dynamics(cfg, node_nfs=(9, 9, 9)):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import state_spec, synthetic_state_dict
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=list(node_nfs), edge_nf=0, condition_nf=1,
                       device=_dev())
    dyn.load_state_dict(synthetic_state_dict(state_spec(cfg, list(node_nfs), 1), cfg, seed=42), strict=True)
    return dyn


def _golden(name):
    from oareactdiff_amd.trainer import DDPMTrainer
    z, meta = vc.load_golden(name)
    tr = DDPMTrainer(_dynamics(meta["model_config"]), timesteps=meta["T"], precision=1e-5, norm_values=meta["norm_values"],
                     pos_only=meta["pos_only"])
    B = len(meta["sizes"])
    batch = (vc.golden_reps(z, torch.float32, _dev()), torch.zeros(B, 1, device=_dev()))
    kw = lambda: dict(t_int=torch.tensor(meta["t_int"], dtype=torch.float32, device=_dev()).view(-1, 1),      # noqa: E731
                      draw=vc.golden_draws(z, meta, torch.float32, _dev()))
    return tr, z, meta, batch, kw


def _close_terms(got, ref, where, K=3):
    """Per row block: 1e-5 of the block's largest entry (at least 1)."""
    got, ref = got.cpu().double(), ref.cpu().double()
    blocks = [(name, slice(i * K, (i + 1) * K)) for i, name in enumerate(BLOCKS)] + [("SNR_weight", slice(5 * K, 5 * K + 1)),
                                                                                   ("neg_log_constants", slice(5 * K + 1, 5 * K + 2))]
    for name, rows in blocks:
        err, scale = float((got[rows] - ref[rows]).abs().max()), max(float(ref[rows].abs().max()), 1.0)
        print(f"{where} {name}: max err {err:.3e}, largest entry {scale:.3e}")
        assert err <= 1e-5 * scale, (where, name, got[rows], ref[rows])


def _close_nll(got, ref, where):
    got, ref = got.cpu().double(), ref.cpu().double()
    err = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print(f"{where} nll: rel err {err:.3e}")
    assert err <= 2e-5, (where, got, ref)


@pytest.mark.parametrize("name", ["g8_loss_eval", "g8_loss_eval_posonly"])
def test_eval_loss_matches_the_recorded_reference_and_the_unfused_path(name):
    tr, z, meta, batch, kw = _golden(name)
    assert tr._can_eval_fused()
    nll, terms = tr.eval_loss(batch, **kw())
    assert nll.shape == (2,) and terms.shape == (17, 2) and nll.is_cuda and terms.is_cuda
    ref_nll, ref_rows = vc.golden_table(z)
    _close_nll(nll, ref_nll, f"{name} vs float64 golden")
    width = 3 if meta["pos_only"] else 12                        # pl_trainer.py:236-244 on the golden's error_t: the normalised rows
    ref_norm = torch.stack([ref_rows[k] / (width * batch[0][k]["size"].cpu()) * tr.loss.scales[k] for k in range(3)])
    _close_terms(terms, torch.cat([ref_norm, ref_rows]), f"{name} vs float64 golden")
    # the same against the unfused formulation on the same draws: compute_loss(training=False) and its terms
    nll_u, info = tr.compute_loss(batch, training=False, **kw())
    _close_nll(nll, nll_u, f"{name} vs compute_loss(training=False)")
    table = vc.vlb_table(tr.loss, batch[0], batch[1], **kw())
    _close_terms(terms, table["terms"], f"{name} vs DiffusionLoss(training=False)")
    row = tr.validation_step(batch, **kw())
    for k in range(3):
        assert abs(float(row[1 + k]) - info[f"error_t_{k}"]) <= 1e-5 * max(abs(info[f"error_t_{k}"]), 1.0)
        assert abs(float(row[4 + k]) - info[f"unorm_error_t_{k}"]) <= 1e-5 * max(abs(info[f"unorm_error_t_{k}"]), 1.0)
    out = tr.validation_epoch_end()
    assert abs(out["val-totloss"] - float(ref_nll.mean())) <= 2e-5 * max(abs(float(ref_nll.mean())), 1.0)


def _narrow(**kw):
    """The trainer-level case off the fixtures: _loss_cases.TRAINER_LAYOUT, the narrow width pair, one layer, fixed_idx = [1],
    norm_biases = (0, 0.5, 0), precision = 0.05 -> (trainer, to_device batch, a factory of (t_int, draw) keyword arguments)."""
    from oareactdiff_amd.trainer import DDPMTrainer
    b = vc.Batch(vc.TRAINER)
    t_list, precision, biases, pos_only, fixed_mask = vc.TRAINER_CASE
    tr = DDPMTrainer(_dynamics(NARROW, b.node_nfs), timesteps=vc.T, precision=precision, norm_values=vc.NORM_VALUES, norm_biases=biases,
                     scales=vc.SCALES, pos_only=bool(pos_only), fixed_idx=vc.FIXED[fixed_mask], **kw)
    reps = [{"size": s, "pos": p, "one_hot": o, "charge": c, "mask": m} for s, p, o, c, m in zip(b.sizes, b.pos, b.one_hot, b.charge, b.masks)]
    batch = DDPMTrainer.to_device((reps, torch.zeros(b.B, 1)), _dev(), non_blocking=False)

    def injected():
        draw = b.draw(torch.float32)
        return dict(t_int=torch.tensor(t_list, dtype=torch.float32, device=_dev()).view(-1, 1), draw=lambda shape: draw(shape).to(_dev()))
    return tr, batch, injected, b


def test_fused_equals_unfused_off_the_fixtures():
    tr, batch, injected, b = _narrow()
    assert tr.fused and tr._can_eval_fused()
    nll, terms = tr.eval_loss(batch, **injected())
    table = vc.vlb_table(tr.loss, batch[0], batch[1], **injected())
    _close_nll(nll, table["nll"], "off the fixtures")
    _close_terms(terms, table["terms"], "off the fixtures")
    # gamma grows with t, so SNR_weight = 1 - exp(gamma_t - gamma_s) is negative (and -T/2 SNR_weight error_t positive), as is neg_log_constants
    assert float(terms[15].max()) < 0 and float(terms[16].max()) < 0
    # ... and with the trainer's own randomness (t_int drawn in [1, T], one randn for both noise blocks)
    nll2, terms2 = tr.eval_loss(batch)
    assert bool(torch.isfinite(nll2).all()) and bool(torch.isfinite(terms2).all()) and not torch.equal(nll2, nll)


def test_ema_weights_are_evaluated_without_touching_the_live_ones():
    tr, batch, injected, _ = _narrow(ema_decay=0.5)
    ema0 = [x.clone() for x in tr.eval_loss(batch, weights="ema", **injected())]
    live0 = [x.clone() for x in tr.eval_loss(batch, **injected())]
    assert all(torch.equal(a, b) for a, b in zip(ema0, live0))               # the average starts as a copy of the weights
    with torch.no_grad():
        tr.flat_param.mul_(1.05)
    tr.dynamics.invalidate_packed()
    ema1 = tr.eval_loss(batch, weights="ema", **injected())
    live1 = tr.eval_loss(batch, **injected())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ema0, ema1))
    assert not torch.equal(live0[0], live1[0]) and not torch.equal(live0[1], live1[1])
    plain, plain_batch, plain_kw, _ = _narrow()
    with pytest.raises(ValueError):
        plain.eval_loss(plain_batch, weights="ema", **plain_kw())
    with pytest.raises(ValueError):
        plain.validation_step(plain_batch, weights="both")


def _training_state(tr):
    dyn = tr.dynamics
    return {"flat_param": tr.flat_param.clone(), "ema": tr.flat_ema.clone(), "m": tr.exp_avg.clone(), "v": tr.exp_avg_sq.clone(),
            "vmax": tr.max_exp_avg_sq.clone(), "opt_step": tr.opt_step, "queue": list(tr.gradnorm_queue.items), "skipped": tr.skipped_steps,
            "training": dyn.training, "nan_check": dyn.nan_check}


def _same_state(a, b):
    for k in ("flat_param", "ema", "m", "v", "vmax"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for k in ("opt_step", "queue", "skipped", "training", "nan_check"):
        assert a[k] == b[k], k


def test_validation_between_two_training_steps_changes_nothing():
    def run(validate):
        tr, batch, injected, _ = _narrow(ema_decay=0.9)
        tr.dynamics.train()
        infos = [tr.training_step(batch, **_train_kw(injected))]
        if validate:
            before = _training_state(tr)
            tr.validation_step(batch)                              # its own randomness
            tr.validation_step(batch, weights="ema")
            tr.test_step(batch)
            out = tr.validation_epoch_end()
            assert len(out) == 20 and out["val-totloss"] == out["val-totloss"]
            _same_state(before, _training_state(tr))
        infos.append(tr.training_step(batch, **_train_kw(injected)))
        return _training_state(tr), infos

    def _train_kw(injected):
        kw = injected()
        draw = kw["draw"]
        blocks = [draw(s) for s in _shapes()]                      # the first noise block of the case serves the training step
        it = iter(blocks)
        return dict(t_int=kw["t_int"], draw=lambda shape: next(it))

    def _shapes():
        b = vc.Batch(vc.TRAINER)
        return [s for m, nf in zip(b.masks, b.node_nfs) for s in ((m.numel(), 3), (m.numel(), nf - 3))]
    plain, plain_infos = run(False)
    mixed, mixed_infos = run(True)
    _same_state(plain, mixed)
    assert plain_infos == mixed_infos and plain_infos[1]["skipped"] == 0 and plain["opt_step"] == 2


def _count_device_reads(monkeypatch, fn):
    """Calls `fn` and counts the device -> host reads made through the tensor methods that make them (as
    tests/test_confidence_trainer_metrics.py does)."""
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


def test_validation_step_reads_nothing_and_the_epoch_end_reads_once(monkeypatch):
    tr, batch, _, _ = _narrow()
    assert all("mask_host" in r and "size_host" in r for r in batch[0])
    tr.validation_step(batch)                                      # the first step builds the topology, the layout and the tables
    _, step_reads = _count_device_reads(monkeypatch, lambda: tr.validation_step(batch))
    _, test_reads = _count_device_reads(monkeypatch, lambda: tr.test_step(batch))
    out, end_reads = _count_device_reads(monkeypatch, tr.validation_epoch_end)
    print("validation_step:", step_reads, "test_step:", test_reads, "validation_epoch_end:", end_reads)
    assert step_reads == {} and test_reads == {} and end_reads == {"tolist": 1}
    assert len(out) == 20 and tr.validation_epoch_end() == {}


def test_results_do_not_depend_on_what_the_workspace_held():
    tr, batch, injected, _ = _narrow()
    first = [x.clone() for x in tr.eval_loss(batch, **injected())]
    ws = tr.dynamics._ws
    assert ws is not None and ws.numel() > 0
    ws.fill_(0xFF)                                                 # every float of the workspace becomes a NaN pattern
    second = tr.eval_loss(batch, **injected())
    assert tr.dynamics._ws is ws
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    assert bool(torch.isfinite(second[0]).all())
