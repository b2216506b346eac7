"""Inputs and float64 / float32 CPU references for the kernel-level tests of the fused loss (tests/test_loss_kernels.py): batches the
golden fixtures do not have - ragged (sample, object) groups of 1 to 130 atoms, an empty group, node_nf of 5 / 7 / 9 / 19 - and
`oareactdiff_amd.loss.DiffusionLoss` run on them with a stub in place of the network.  No GPU is touched here."""
import itertools

import torch

from oareactdiff_amd.graph_tools import get_mask_for_frag, get_n_frag_switch
from oareactdiff_amd.loss import DiffusionLoss, _cdf, _segment_sum
from oareactdiff_amd.schedule import Schedule

T = 1000
POS = 3
NORM_VALUES = (1.0, 4.0, 10.0)
SCALES = (1.0, 2.0, 1.0)
#: config_ok (csrc/oard_hip.hip) accepts node_nf - 3 <= 16, the loss entries node_nf - 4 <= 16: 19 is the widest both take
#: (test_loss_kernels.test_widest_node_nf_is_the_widest_supported asks the library)
WIDEST_NF = 19
#           atoms per sample of R, TS, P                                         node_nfs
LAYOUTS = {
    "ragged": ([[7, 23, 12, 1, 70], [9, 20, 5, 3, 16], [4, 23, 12, 2, 130]], [9, 9, 9]),
    "mixed_nf": ([[7, 23, 12, 1, 70], [9, 20, 5, 3, 16], [4, 23, 12, 2, 130]], [5, 9, 7]),
    "empty_group": ([[2, 0], [2, 3], [1, 2]], [9, 9, 9]),             # object 0 is empty in sample 1; object 2 has one atom in sample 0
    "widest": ([[3, 65], [2, 1], [64, 5]], [WIDEST_NF] * 3),          # 64 atoms: every lane once; 65: one lane twice
}
#: reactions of 1, 2, 4 and 8 objects instead of three (the library takes 1 to 8): the kernels' object loop, the per-object pointer
#: tables and the (sample, object) group table at every count.  Kept apart from LAYOUTS: their fixed masks differ (`fixed_masks`).  The loss
#: entries need a class column (node_nf >= 5), so the narrowest object of `four_objects` has 5 where the wrapper alone would take 4.
OBJECT_LAYOUTS = {
    "one_object": ([[8, 1, 17, 5]], [9]),
    "two_objects": ([[9, 0, 5], [12, 7, 5]], [7, 12]),                # object 0 is empty in sample 1
    "four_objects": ([[2, 3, 6], [1, 4, 3], [3, 0, 5], [2, 2, 7]], [5, WIDEST_NF, 9, 6]),
    "eight_objects": ([[k + 1, 8 - k] for k in range(8)], [9] * 8),   # groups of 1 to 8 atoms
}
#: layout -> (condition_nf, model_config overrides) of the module whose oard_config the kernel tests pass; default (1, {}).
#: four_objects: embedding 10 + t + 5 conditions fill all 16 columns of in_hidden_channels = 16
OBJECT_MODEL = {"two_objects": (0, {}), "four_objects": (5, {"in_hidden_channels": 16})}
#: every layout sees t = 0 (at least twice in one batch), 1, a middle step and T; ragged[0] puts t = 0 on the 70 / 130-atom sample
T_INTS = {
    "ragged": [[0, 500, 0, 1000, 0], [1, 0, 500, 0, 1000]],
    "mixed_nf": [[0, 500, 0, 1000, 0], [1, 0, 500, 0, 1000]],
    "empty_group": [[0, 0], [1, 1000], [500, 0]],
    "widest": [[0, 0], [1, 1000], [0, 500]],
    "one_object": [[0, 500, 0, 1000], [1, 0, 500, 0]],
    "two_objects": [[0, 0, 500], [1, 1000, 0]],
    "four_objects": [[0, 0, 500], [1, 1000, 0]],
    "eight_objects": [[0, 0], [1, 1000], [500, 0]],
}
#: the one trainer-level case off the fixtures (test_trainer_fused.py): the network runs, so three objects of node_nf = 9
TRAINER = "trainer_ragged"
TRAINER_LAYOUT = ([[7, 23, 12], [9, 20, 5], [4, 23, 12]], [9, 9, 9])
TRAINER_CASE = ([0, 500, 0], 0.05, (0.0, 0.5, 0.0), 0, 0b010)
PRECISIONS = (1e-5, 0.05)             # sigma_0 = 3.2e-3 (every cdf difference of the t = 0 terms is 0 or 1) and 0.2236 (none is)
BIASES = ((0.0, 0.0, 0.0), (0.0, 0.5, 0.0))
FIXED = {0: [], 0b010: [1], 0b101: [0, 2]}      # fixed_mask -> fixed_idx
#: seeds of the inputs, chosen so that test_inputs_keep_clear_of_the_float32_discontinuities holds for every case (a draw within
#: ~2e-4 of zero on the charge column of a t = 0 atom would not)
SEEDS = {"ragged": 101, "mixed_nf": 102, "empty_group": 103, "widest": 104, TRAINER: 105,
         "one_object": 106, "two_objects": 107, "four_objects": 108, "eight_objects": 109}


def scales(K):
    """1, 2, 1, 2, ... per object: SCALES at three."""
    return tuple((1.0, 2.0)[k % 2] for k in range(K))


def fixed_idx(fixed_mask):
    return [k for k in range(8) if (fixed_mask >> k) & 1]


def fixed_masks(layout):
    """LAYOUTS: FIXED's three.  OBJECT_LAYOUTS: nothing fixed, one object (the second, or the only one), every even and every odd one."""
    if layout not in OBJECT_LAYOUTS:
        return list(FIXED)
    K = len(OBJECT_LAYOUTS[layout][0])
    every = (1 << K) - 1
    return list(dict.fromkeys([0, 1 << min(1, K - 1), 0x55 & every, 0xAA & every]))


def cases(layout):
    """Every (t_int, precision, norm_biases, pos_only, fixed_mask) of a layout."""
    if layout == TRAINER:
        return [TRAINER_CASE]
    return list(itertools.product(T_INTS[layout], PRECISIONS, BIASES, (0, 1), fixed_masks(layout)))


def tag(case):
    t_int, precision, biases, pos_only, fixed_mask = case
    return f"t_int {t_int} precision {precision} biases {biases} pos_only {pos_only} fixed_mask {fixed_mask:03b}"


class Batch:
    """pos ~ 2 N(0,1), one random class per atom, integer charges in [-2, 8], net ~ N(0,1), draws ~ N(0,1) clamped to [-2, 2] (the
    kernels take the draws as an argument; the clamp keeps every cdf difference of a live t = 0 term above ~5e-3 at sigma_0 = 0.22)."""

    def __init__(self, layout):
        frags, self.node_nfs = TRAINER_LAYOUT if layout == TRAINER else (LAYOUTS.get(layout) or OBJECT_LAYOUTS[layout])
        self.layout = layout
        g = torch.Generator().manual_seed(SEEDS[layout])
        self.sizes = [torch.tensor(f) for f in frags]
        self.masks = [get_mask_for_frag(s) for s in self.sizes]
        self.combined_mask = torch.cat(self.masks)
        self.n_frag_switch = get_n_frag_switch(self.sizes)
        self.B, self.K = len(frags[0]), len(frags)
        self.pos, self.one_hot, self.charge, self.noise, self.net = [], [], [], [], []
        for m, nf in zip(self.masks, self.node_nfs):
            n = m.numel()
            self.pos.append(2.0 * torch.randn(n, POS, generator=g))
            oh = torch.zeros(n, nf - 4, dtype=torch.int64)
            oh[torch.arange(n), torch.randint(0, nf - 4, (n,), generator=g)] = 1
            self.one_hot.append(oh)
            self.charge.append(torch.randint(-2, 9, (n, 1), generator=g))
            self.noise.append(torch.randn(n, nf, generator=g).clamp(-2.0, 2.0))
            self.net.append(torch.randn(n, nf, generator=g))

    def reps(self, dtype):
        """The dataset layout, every field in `dtype` (integer fields would be normalised in float32 whatever the run's precision).
        `size` is clamped to 1: DiffusionLoss divides three sums over a group by its size, each sum is exactly 0 for an empty group,
        so 0 / 1 replaces the 0 / 0 of those three quotients by 0 and changes nothing else (the l2 training loss reads `size`
        nowhere else)."""
        return [{"size": s.clamp(min=1), "pos": p.to(dtype), "one_hot": o.to(dtype), "charge": c.to(dtype), "mask": m}
                for s, p, o, c, m in zip(self.sizes, self.pos, self.one_hot, self.charge, self.masks)]

    def draw(self, dtype):
        """DiffusionLoss's protocol: per object randn(n, 3), then randn(n, nf - 3)."""
        blocks = []
        for x in self.noise:
            blocks += [x[:, :POS], x[:, POS:]]
        it = iter(blocks)

        def draw(shape):
            x = next(it)
            assert tuple(x.shape) == tuple(shape)
            return x.to(dtype)
        return draw


class WideLoss(DiffusionLoss):
    """DiffusionLoss with log p(h | z_0) restated WITHOUT the slice of z to pos_dim + 6 columns (which the reference has, and which
    makes `_log_pxh_given_z0` usable for node_nf <= 9 only): the same formulas on all node_nf - 4 class columns and the last
    column as the charge.  For node_nf <= 9 the two are the same bits (test_loss_kernels.test_restated_likelihood_is_the_class_s)."""

    def _log_pxh_given_z0(self, reps, masks, z, eps, net, gamma, n_samples, epsilon=1e-10):
        pd = self.pos_dim
        log_px = [-0.5 * _segment_sum((e[:, :pd] - o[:, :pd]) ** 2, m, n_samples) for e, o, m in zip(eps, net, masks)]
        sigma0 = torch.sqrt(torch.sigmoid(gamma))
        s_cat, s_chg = sigma0 * self.norm_values[1], sigma0 * self.norm_values[2]
        log_cat, log_chg = [], []
        for r, m, v in zip(reps, masks, z):
            atoms = r["one_hot"] * self.norm_values[1] + self.norm_biases[1]
            centred = (v[:, pd:-1] * self.norm_values[1] + self.norm_biases[1]) - 1
            lp = torch.log(_cdf((centred + 0.5) / s_cat[m]) - _cdf((centred - 0.5) / s_cat[m]) + epsilon)
            lp = lp - torch.logsumexp(lp, dim=1, keepdim=True)
            log_cat.append(_segment_sum(lp * atoms, m, n_samples))
            charge = r["charge"][:, :1] * self.norm_values[2] + self.norm_biases[2]
            est = (v[:, -1:] * self.norm_values[2] + self.norm_biases[2]).long()
            c = charge - est
            lq = torch.log(_cdf((c + 0.5) / s_chg[m]) - _cdf((c - 0.5) / s_chg[m]) + epsilon)
            log_chg.append(_segment_sum(lq, m, n_samples))
        return log_px, log_cat, log_chg


class Stub:
    """The network: returns the given tensors (leaves of the autograd graph) and keeps the z_t it was called with."""
    pos_dim = POS

    def __init__(self, node_nfs, net):
        self.node_nfs, self.net, self.seen = list(node_nfs), net, None

    def __call__(self, xh, **kw):
        self.seen = [x.detach().clone() for x in xh]
        return self.net, None


def loss_object(batch, case, net, cls=None):
    t_int, precision, biases, pos_only, fixed_mask = case
    cls = cls or (WideLoss if max(batch.node_nfs) > 9 else DiffusionLoss)
    return cls(Stub(batch.node_nfs, net), "polynomial_2", T, precision, norm_values=NORM_VALUES, norm_biases=biases,
               pos_only=bool(pos_only), fixed_idx=fixed_idx(fixed_mask), scales=scales(batch.K))


def reference(batch, case, dtype, b_total=None, cls=None):
    """DiffusionLoss on the CPU in `dtype` -> dict of z, eps, dnet (lists per object), nll [B], terms [2 K, B] (rows 0 .. K-1 the
    normalised, scaled error per object, rows K .. the un-normalised one: what oard_loss_terms writes and `info` logs the means of).
    dnet = d(sum_b nll / b_total) / d net: oard_loss_terms takes B_total both as the row stride of `terms` and as the 1 / B of
    the mean, so a part of a larger step gets nll.mean(0).backward() times B / B_total."""
    t_int = torch.tensor(case[0], dtype=dtype).view(-1, 1)
    B, K = batch.B, batch.K
    b_total = b_total or B
    net = [x.detach().to(dtype, copy=True).requires_grad_() for x in batch.net]
    dl = loss_object(batch, case, net, cls)
    reps, cond = batch.reps(dtype), torch.zeros(B, 1, dtype=dtype)
    lt = dl.loss_terms(reps, cond, training=True, t_int=t_int, draw=batch.draw(dtype))
    z, eps = dl.dynamics.seen, [e.detach() for e in lt["eps_xh"]]
    nll, info = dl.compute_loss(reps, cond, training=True, t_int=t_int, draw=batch.draw(dtype))
    nll.mean(0).backward()
    dnet = [x.grad * (B / b_total) for x in net]
    err_t = [e.detach() for e in lt["error_t"]]
    width = [POS if dl.pos_only else POS + nf for nf in batch.node_nfs]
    err_n = [err_t[k] / (width[k] * reps[k]["size"]) * dl.scales[k] for k in range(K)]
    for k in range(K):                                     # the rows ARE what compute_loss logs
        assert abs(float(err_n[k].mean() / (dl.scales[k] + 1e-4)) - info[f"error_t_{k}"]) <= 1e-6 * abs(info[f"error_t_{k}"]) + 1e-30
        assert abs(float(err_t[k].mean()) - info[f"unorm_error_t_{k}"]) <= 1e-6 * abs(info[f"unorm_error_t_{k}"]) + 1e-30
    return {"z": z, "eps": eps, "dnet": dnet, "nll": nll.detach(), "terms": torch.stack(err_n + err_t)}


def discontinuity_margins(batch, case):
    """For every atom of a t = 0 sample, in float64: (charge estimates z_charge norm_value[2] + norm_bias[2], every cdf difference of
    the class and charge terms) - the two places where a float32 rounding may legitimately flip the result."""
    t_int, precision, biases, pos_only, fixed_mask = case
    ref = reference(batch, case, torch.float64)
    sigma0 = float(torch.sqrt(torch.sigmoid(Schedule("polynomial_2", T, precision).gamma[0].double())))
    s_cat, s_chg = sigma0 * NORM_VALUES[1], sigma0 * NORM_VALUES[2]
    tz = torch.tensor(t_int) == 0
    values, diffs = [], []
    for k, m in enumerate(batch.masks):
        z = ref["z"][k][tz[m]]
        v = z[:, -1] * NORM_VALUES[2] + biases[2]
        values.append(v)
        cen = (z[:, POS:-1] * NORM_VALUES[1] + biases[1]) - 1
        diffs.append((_cdf((cen + 0.5) / s_cat) - _cdf((cen - 0.5) / s_cat)).reshape(-1))
        c = batch.charge[k][tz[m], 0].double() - v.long().double()
        diffs.append(_cdf((c + 0.5) / s_chg) - _cdf((c - 0.5) / s_chg))
    return torch.cat(values), torch.cat(diffs)
