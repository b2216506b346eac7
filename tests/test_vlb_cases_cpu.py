"""The case helpers of the evaluation-loss tests (tests/_vlb_cases.py) checked on the CPU: the restated terms table is the reference's,
the inputs keep clear of the two float32 discontinuities on EVERY atom, the cases cover what they claim, and the host SNR table is
the float64 expression rounded once."""
import numpy as np
import pytest
import torch

import _vlb_cases as vc
from oareactdiff_amd.loss import DiffusionLoss
from oareactdiff_amd.schedule import Schedule
from oareactdiff_amd.trainer import vlb_snr_table


@pytest.mark.parametrize("name", ["g8_loss_eval", "g8_loss_eval_posonly"])
def test_table_helper_reproduces_the_recorded_reference_f64(name):
    """`vlb_table` on DiffusionLoss(training=False) with the reference's recorded float64 network outputs replayed, against the golden's
    float64 terms and nll: 1e-11, the gate of test_loss.py."""
    z, meta = vc.load_golden(name)
    assert not meta["training"] and meta["n_net_calls"] == 2 and meta["n_randn"] == 12
    dt = torch.float64
    dl = DiffusionLoss(vc.Replay(z, dt), "polynomial_2", meta["T"], 1e-5, norm_values=meta["norm_values"], pos_only=meta["pos_only"])
    B = len(meta["sizes"])
    reps = vc.golden_reps(z, dt)
    got = vc.vlb_table(dl, reps, torch.zeros(B, 1, dtype=dt), torch.tensor(meta["t_int"], dtype=dt).view(-1, 1), vc.golden_draws(z, meta, dt))
    nll, rows = vc.golden_table(z)
    assert got["terms"].shape == (17, B) and rows.shape == (14, B)
    assert torch.allclose(got["terms"][3:], rows, rtol=1e-11, atol=1e-11)
    assert torch.allclose(got["nll"], nll, rtol=1e-11, atol=1e-11)
    # the normalised rows: pl_trainer.py:236-244 on the golden's error_t
    width = 3 if meta["pos_only"] else 12
    for k in range(3):
        want = torch.from_numpy(z[f"f64_error_t{k}"]) / (width * reps[k]["size"]) * dl.scales[k]
        assert torch.allclose(got["terms"][k], want, rtol=1e-11, atol=1e-11)
        assert abs(got["info"][f"error_t_{k}"] - float(want.mean() / (dl.scales[k] + 1e-4))) <= 1e-11 * abs(float(want.mean())) + 1e-30
    # nll really cancels: the sum of the absolute contributions is larger than |nll|
    assert bool((got["contrib"] > got["nll"].abs()).all())


@pytest.mark.parametrize("layout", list(vc.LAYOUTS) + [vc.TRAINER] + list(vc.OBJECT_LAYOUTS))
def test_inputs_keep_clear_of_the_float32_discontinuities(layout):
    """In the float64 reference, for every atom of every sample of every case (in evaluation each has the t = 0 terms): the charge
    estimate that `.long()` truncates lies at least 2^-20 |value| from every non-zero integer, and every cdf difference under a log is
    above 1e-3 or below 1e-12.  Zero exclusions: the seeds of _vlb_cases.SEEDS0 are chosen so that it holds with no case dropped."""
    batch = vc.Batch(layout)
    n_atoms = int(batch.combined_mask.numel())
    for case in vc.cases(layout):
        values, diffs = vc.discontinuity_margins(batch, case)
        assert values.numel() == n_atoms
        nearest = values.round()
        close = (nearest != 0) & ((values - nearest).abs() < 2.0 ** -20 * values.abs())
        assert not bool(close.any()), f"{layout} {vc.tag(case)}: charge estimates {values[close].tolist()}"
        grey = (diffs <= 1e-3) & (diffs >= 1e-12)
        assert not bool(grey.any()), f"{layout} {vc.tag(case)}: cdf differences {diffs[grey].tolist()}"


def test_cases_cover_what_they_are_meant_to():
    sizes = {n for frags, _ in vc.LAYOUTS.values() for f in frags for n in f}
    assert {0, 1, 64, 65, 70, 130} <= sizes
    assert {nf for _, nfs in vc.LAYOUTS.values() for nf in nfs} >= {5, 7, 9, 19}
    for layout, (frags, nfs) in vc.LAYOUTS.items():
        ts = vc.T_INTS[layout]
        assert all(len(t) == len(frags[0]) for t in ts)
        assert all(1 <= v <= vc.T for t in ts for v in t)                  # evaluation: t_int in [1, T]
        assert all(any(v in t for t in ts) for v in (1, 500, vc.T))
        cs = vc.cases(layout)
        assert len(cs) == len(ts) * 2 * 2 * 2 * 3
        assert {c[1] for c in cs} == set(vc.PRECISIONS) and {c[2] for c in cs} == set(vc.BIASES)
        assert {c[3] for c in cs} == {0, 1} and {c[4] for c in cs} == set(vc.FIXED) == {0, 0b010, 0b101}
    assert vc.NORM_VALUES[0] != 1.0                                        # delta_log_px is not 0
    s0 = [float(torch.sqrt(torch.sigmoid(Schedule("polynomial_2", vc.T, p).gamma[0].double()))) for p in vc.PRECISIONS]
    assert abs(s0[0] - 3.2e-3) <= 1e-4 and abs(s0[1] - 0.2236) <= 1e-4
    # the second block is its own draw, and the reference sees both
    b = vc.Batch("empty_group")
    assert all(not torch.equal(x, y) for x, y in zip(b.noise, b.noise0))
    ref = vc.reference(b, vc.cases("empty_group")[0], torch.float64)
    assert ref["terms"].shape == (17, b.B) and bool(torch.isfinite(ref["terms"]).all()) and ref["delta_log_px"] != 0.0
    empty = b.sizes[0] == 0
    assert int(empty.sum()) == 1 and all(float(ref["terms"][r * 3][empty].abs().sum()) == 0.0 for r in range(5))


@pytest.mark.parametrize("schedule,T,precision", [("polynomial_2", 1000, 1e-5), ("polynomial_2", 1000, 0.05), ("polynomial_2", 100, 1e-5),
                                                  ("cosine", 500, 1e-5)])
def test_host_snr_table_is_the_float64_expression_rounded_once(schedule, T, precision):
    s = Schedule(schedule, T, precision)
    table = vlb_snr_table(s)
    assert table.dtype == torch.float32 and table.shape == (T + 1,) and float(table[0]) == 0.0
    want = vc.snr_reference(s).numpy()
    got = table[1:].numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), float(np.max(np.abs(got - want) / ulp))
    # what float32 arithmetic would have given instead: off by far more than an ulp somewhere
    g32 = s.gamma
    f32 = (1 - torch.exp(-(g32[:-1] - g32[1:]))).numpy().astype(np.float64)
    assert np.max(np.abs(f32 - want) / ulp) > 4
