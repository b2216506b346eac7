"""Inputs and float64 / float32 CPU references for the tests of the evaluation loss (the variational bound: tests/test_vlb_kernels.py,
test_vlb_cases_cpu.py, test_trainer_validation*.py): the layouts of tests/_loss_cases.py - ragged (sample, object) groups of 0 to 130
atoms, node_nf of 5 / 7 / 9 / 19 - with a SECOND noise block and a second network output for the t = 0 call, evaluation-mode time
steps (t_int in [1, T]) and a position normaliser other than 1, so that delta_log_px is not 0.  `vlb_table` restates what
`oard_loss_eval_terms` writes from `oareactdiff_amd.loss.DiffusionLoss(training=False)`.  No GPU is touched here."""
import itertools
import json
import os

import numpy as np
import torch

import _loss_cases as lc
from oareactdiff_amd.loss import DiffusionLoss, _cdf
from oareactdiff_amd.schedule import Schedule

T = lc.T
POS = lc.POS
NORM_VALUES = (2.0, 4.0, 10.0)        # norm_values[0] != 1: delta_log_px = -(N - 1) 3 log 2
SCALES = lc.SCALES
LAYOUTS, OBJECT_LAYOUTS, OBJECT_MODEL = lc.LAYOUTS, lc.OBJECT_LAYOUTS, lc.OBJECT_MODEL
PRECISIONS, BIASES, FIXED = lc.PRECISIONS, lc.BIASES, lc.FIXED
#: evaluation draws t_int in [1, T]: every layout sees 1, a middle step and T
T_INTS = {
    "ragged": [[1, 500, 1000, 1, 500], [1000, 1, 500, 1000, 1]],
    "mixed_nf": [[1, 500, 1000, 1, 500], [1000, 1, 500, 1000, 1]],
    "empty_group": [[1, 1000], [500, 1]],
    "widest": [[1000, 500], [1, 1000]],
    "one_object": [[1, 500, 1000, 1], [1000, 1, 500, 1000]],
    "two_objects": [[1, 500, 1000], [1000, 1, 500]],
    "four_objects": [[1, 500, 1000], [1000, 1, 500]],
    "eight_objects": [[1, 1000], [500, 1]],
}
TRAINER = lc.TRAINER
TRAINER_CASE = ([1, 500, 1000], 0.05, (0.0, 0.5, 0.0), 0, 0b010)
#: seeds of the second noise block (z_0) and the second network output, chosen so that
#: test_vlb_cases_cpu.test_inputs_keep_clear_of_the_float32_discontinuities holds for EVERY case - in evaluation every atom of every
#: sample has the t = 0 terms, so a draw within ~3e-4 of zero on any charge column would not
SEEDS0 = {"ragged": 201, "mixed_nf": 202, "empty_group": 203, "widest": 204, TRAINER: 205,
          "one_object": 206, "two_objects": 207, "four_objects": 208, "eight_objects": 209}
TERM_KEYS = ("error_t", "loss_0_x", "loss_0_cat", "loss_0_charge")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cases(layout):
    """Every (t_int, precision, norm_biases, pos_only, fixed_mask) of a layout."""
    if layout == TRAINER:
        return [TRAINER_CASE]
    return list(itertools.product(T_INTS[layout], PRECISIONS, BIASES, (0, 1), lc.fixed_masks(layout)))


tag = lc.tag


def snr_reference(schedule):
    """1 - exp(-(gamma_s - gamma_t)) for t = 1 .. T in float64, on the schedule's table widened to float64 (what DiffusionLoss looks up
    in a float64 run)."""
    g = schedule.gamma.double()
    return 1 - torch.exp(-(g[:-1] - g[1:]))


class Batch(lc.Batch):
    """_loss_cases.Batch plus the t = 0 call's draws (`noise0`, clamped like `noise`) and network output (`net0`)."""

    def __init__(self, layout):
        super().__init__(layout)
        g = torch.Generator().manual_seed(SEEDS0[layout])
        self.noise0, self.net0 = [], []
        for m, nf in zip(self.masks, self.node_nfs):
            self.noise0.append(torch.randn(m.numel(), nf, generator=g).clamp(-2.0, 2.0))
            self.net0.append(torch.randn(m.numel(), nf, generator=g))

    def reps(self, dtype):
        """The dataset layout with the TRUE sizes (neg_log_constants and delta_log_px count atoms); `vlb_table(floor_sizes=True)`
        replaces the 0 / 0 of an empty group's normalised error by 0 / 1."""
        return [{"size": s, "pos": p.to(dtype), "one_hot": o.to(dtype), "charge": c.to(dtype), "mask": m}
                for s, p, o, c, m in zip(self.sizes, self.pos, self.one_hot, self.charge, self.masks)]

    def draw(self, dtype):
        """DiffusionLoss's protocol in evaluation: per object randn(n, 3), randn(n, nf - 3) for z_t, then the same again for z_0."""
        blocks = []
        for x in self.noise + self.noise0:
            blocks += [x[:, :POS], x[:, POS:]]
        it = iter(blocks)

        def draw(shape):
            x = next(it)
            assert tuple(x.shape) == tuple(shape)
            return x.to(dtype)
        return draw


class TwoCallStub:
    """The network: the first call returns `net_t`, the second `net_0`."""
    pos_dim = POS

    def __init__(self, node_nfs, net_t, net_0):
        self.node_nfs, self.outs, self.calls = list(node_nfs), [net_t, net_0], 0

    def __call__(self, xh, **kw):
        self.calls += 1
        return self.outs[self.calls - 1], None


def _capturing(cls):
    class Capturing(cls):
        """Keeps (z, eps) of every noised representation: z_t's first, then z_0's."""

        def _noised(self, *a, **k):
            z, eps = super()._noised(*a, **k)
            self.__dict__.setdefault("noised", []).append(([v.detach().clone() for v in z], [v.detach().clone() for v in eps]))
            return z, eps
    return Capturing


def loss_object(batch, case, dtype):
    t_int, precision, biases, pos_only, fixed_mask = case
    cls = _capturing(lc.WideLoss if max(batch.node_nfs) > 9 else DiffusionLoss)
    stub = TwoCallStub(batch.node_nfs, [x.to(dtype) for x in batch.net], [x.to(dtype) for x in batch.net0])
    return cls(stub, "polynomial_2", T, precision, norm_values=NORM_VALUES, norm_biases=biases, pos_only=bool(pos_only),
               fixed_idx=lc.fixed_idx(fixed_mask), scales=lc.scales(batch.K))


def vlb_table(dl, reps, cond, t_int, draw, floor_sizes=False):
    """`DiffusionLoss.loss_terms(training=False)` + `nll_and_info` restated as what `oard_loss_eval_terms` writes -> dict:
    nll [B]; terms [5 K + 2, B] (rows [0, K) the normalised, scaled error_t per object, [K, 2K) error_t, [2K, 3K) loss_0_x, [3K, 4K)
    loss_0_cat, [4K, 5K) loss_0_charge, row 5K SNR_weight, row 5K + 1 neg_log_constants); contrib [B] = the sum of the absolute values
    of the contributions nll adds up (it cancels: neg_log_constants is negative); info (the logged means); lt (the terms dict)."""
    lt = dl.loss_terms(reps, cond, training=False, t_int=t_int, draw=draw)
    K = len(reps)
    sized = [dict(r, size=r["size"].clamp(min=1)) for r in reps] if floor_sizes else reps
    nll, info = dl.nll_and_info(lt, sized, training=False)
    width = [POS if dl.pos_only else POS + dl.node_nfs[k] for k in range(K)]
    err_n = [lt["error_t"][k] / (width[k] * sized[k]["size"]) * dl.scales[k] for k in range(K)]
    rows = err_n + [lt[key][k] for key in TERM_KEYS for k in range(K)] + [lt["SNR_weight"], lt["neg_log_constants"]]
    contrib = sum((0.5 * dl.T * lt["SNR_weight"] * e).abs() for e in lt["error_t"])
    contrib = contrib + sum(lt[key][k].abs() for key in TERM_KEYS[1:] for k in range(K)) + lt["neg_log_constants"].abs()
    contrib = contrib + abs(float(lt["delta_log_px"]))
    return {"nll": nll.detach(), "terms": torch.stack(rows).detach(), "contrib": contrib.detach(), "info": info, "lt": lt}


def reference(batch, case, dtype):
    """DiffusionLoss(training=False) on the CPU in `dtype` -> `vlb_table`'s dict plus z_t, eps_t, z_0, eps_0 (lists per object) and
    delta_log_px (float)."""
    t_int = torch.tensor(case[0], dtype=dtype).view(-1, 1)
    dl = loss_object(batch, case, dtype)
    out = vlb_table(dl, batch.reps(dtype), torch.zeros(batch.B, 1, dtype=dtype), t_int, batch.draw(dtype), floor_sizes=True)
    assert dl.dynamics.calls == 2 and len(dl.noised) == 2
    (out["z_t"], out["eps_t"]), (out["z_0"], out["eps_0"]) = dl.noised
    out["delta_log_px"] = float(out["lt"]["delta_log_px"])
    return out


def discontinuity_margins(batch, case):
    """For EVERY atom, in float64: (charge estimates z_0[:, -1] norm_value[2] + norm_bias[2], every cdf difference of the class and charge
    terms) - the two places where a float32 rounding may legitimately flip the result."""
    t_int, precision, biases, pos_only, fixed_mask = case
    ref = reference(batch, case, torch.float64)
    sigma0 = float(torch.sqrt(torch.sigmoid(Schedule("polynomial_2", T, precision).gamma[0].double())))
    s_cat, s_chg = sigma0 * NORM_VALUES[1], sigma0 * NORM_VALUES[2]
    values, diffs = [], []
    for k in range(batch.K):
        z = ref["z_0"][k]
        v = z[:, -1] * NORM_VALUES[2] + biases[2]
        values.append(v)
        cen = (z[:, POS:-1] * NORM_VALUES[1] + biases[1]) - 1
        diffs.append((_cdf((cen + 0.5) / s_cat) - _cdf((cen - 0.5) / s_cat)).reshape(-1))
        c = batch.charge[k][:, 0].double() - v.long().double()
        diffs.append(_cdf((c + 0.5) / s_chg) - _cdf((c - 0.5) / s_chg))
    return torch.cat(values), torch.cat(diffs)


# ---- the recorded evaluation runs of the reference (tests/golden/g8_loss_eval*.npz, read as tests/test_loss.py reads them) -------------
def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def golden_reps(z, dtype, dev="cpu"):
    reps = []
    for k in range(3):
        r = {f: torch.from_numpy(z[f"rep{k}_{f}"]).to(dev) for f in ("size", "pos", "one_hot", "charge", "mask")}
        r["pos"] = r["pos"].to(dtype)
        reps.append(r)
    return reps


def golden_draws(z, meta, dtype, dev="cpu"):
    it = iter(range(meta["n_randn"]))

    def draw(shape):
        x = torch.from_numpy(z[f"randn{next(it)}"]).to(device=dev, dtype=dtype)
        assert tuple(x.shape) == tuple(shape)
        return x
    return draw


class Replay:
    """The reference's own recorded network outputs (float32 run: `net_call`, float64 run: `net64_call`)."""
    pos_dim, node_nfs = 3, [9, 9, 9]

    def __init__(self, z, dtype):
        self.z, self.dtype, self.calls = z, dtype, 0
        self.prefix = "net_call" if dtype == torch.float32 else "net64_call"

    def __call__(self, **kw):
        c, self.calls = self.calls, self.calls + 1
        return [torch.from_numpy(self.z[f"{self.prefix}{c}_{k}"]).to(self.dtype) for k in range(3)], None

    def parameters(self):
        return iter(())

    def named_parameters(self):
        return iter(())


def golden_table(z, tag="f64"):
    """The golden's own numbers laid out as `vlb_table` lays them out -> (nll [B], terms [17, B] without the normalised rows: [3, 17))."""
    rows = [torch.from_numpy(z[f"{tag}_{key}{k}"]) for key in TERM_KEYS for k in range(3)]
    rows += [torch.from_numpy(z[f"{tag}_SNR_weight"]), torch.from_numpy(z[f"{tag}_neg_log_constants"])]
    return torch.from_numpy(z[f"{tag}_nll"]), torch.stack([r.reshape(-1) for r in rows])
