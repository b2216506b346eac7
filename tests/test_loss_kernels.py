"""k_loss_prep and k_loss_terms (behind oard_loss_prepare / oard_loss_terms) on their own against oareactdiff_amd.loss.DiffusionLoss in
float64 on the CPU - with tensors the golden fixtures do not have (tests/_loss_cases.py): (sample, object) groups of 1, 64, 65, 70
and 130 atoms (the lane-stride loop and the 64-lane shuffle reduction), an empty group, node_nf of 5 / 7 / 9 / 19, non-zero
norm_biases, fixed objects, several t = 0 samples in one batch, t = 1 and t = T, and a schedule (precision = 0.05, sigma_0 = 0.2236)
under which the discretised likelihoods of the t = 0 terms are not all 0 or 1.  The network is never run: `net` is a random tensor.

The gate of every output: err <= max(4 e32, 2^-21), e32 = the same DiffusionLoss in float32 on the CPU against its float64 run.  nll:
err per sample relative to that sample's own |ref| (every term of nll is non-negative: nothing cancels), the largest over the batch;
z, eps, terms, dnet: max|x - ref| / max|ref| over the tensor (z and eps also on their feature block alone, which the positions would
otherwise out-scale; terms also on its normalised and un-normalised halves alone).  The factor 4 covers the kernel's summation
order (64 lanes, then the shuffle tree).

An empty (sample, object) group: DiffusionLoss divides by the group's size and gives NaN; the kernel is written to contribute 0
(include/oard.h).  The reference is computed with the three quotients of that group replaced by 0 (_loss_cases.Batch.reps), and the
group's `terms` entries must be exact zeros.

MEASURED on an MI355X, the worst case of every output over all layouts and cases - kernel err (e32 beside it), largest err / gate:
  oard_loss_prepare   z 9.44e-08 (9.44e-08) 0.20   z features 8.84e-08 (8.84e-08) 0.19   eps 7.06e-08 (7.06e-08) 0.15   eps features 0 (0)
  oard_loss_terms     nll 2.72e-07 (8.69e-08) 0.57   terms 1.12e-07 (1.12e-07) 0.23   normalised half 1.03e-07 (7.44e-08) 0.22
                      un-normalised half 1.12e-07 (1.12e-07) 0.23   dnet 1.38e-07 (1.38e-07) 0.25
  prepare -> terms    nll 2.72e-07 (8.69e-08) 0.57   terms 1.12e-07 (1.12e-07) 0.23   dnet 1.38e-07 (1.38e-07) 0.25
e32 over all cases (this file's CPU runs): z <= 9.4e-08, eps <= 7.1e-08, dnet <= 1.4e-07, nll <= 8.7e-07, terms <= 3.6e-07.  Per layout:
the table at the end of this file; per case: run with -s."""
import ctypes as C

import pytest
import torch

import _loss_cases as lc
from _cases import rel

FLOOR = 2.0 ** -21
# the network is never run here: the narrowest built width pair, one layer
NARROW = dict(pos_require_grad=False, cutoff=5.0, num_layers=1, hidden_channels=32, num_radial=8, in_hidden_channels=8)
PAD, COL0 = 3, 2                      # `terms` has B_total = B + PAD columns, the call owns [COL0, COL0 + B) (DDPMTrainer._fused_part)


# ---- CPU-only checks of the inputs and of the restated reference --------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(lc.LAYOUTS) + [lc.TRAINER] + list(lc.OBJECT_LAYOUTS))
def test_inputs_keep_clear_of_the_float32_discontinuities(layout):
    """In the float64 reference, for every atom of a t = 0 sample of every case: the charge estimate that `.long()` truncates lies at
    least 2^-20 |value| from every non-zero integer (truncation is continuous at 0), and every cdf difference under a log is above
    1e-3 or below 1e-12 (where the 1e-10 inside the log decides).  Otherwise a float32 rounding could flip a kernel result that is
    right.  No case is dropped to get there: the seeds of _loss_cases.SEEDS are chosen so that it holds."""
    batch = lc.Batch(layout)
    n_t0 = 0
    for case in lc.cases(layout):
        values, diffs = lc.discontinuity_margins(batch, case)
        n_t0 += values.numel()
        nearest = values.round()
        close = (nearest != 0) & ((values - nearest).abs() < 2.0 ** -20 * values.abs())
        assert not bool(close.any()), f"{layout} {lc.tag(case)}: charge estimates {values[close].tolist()}"
        grey = (diffs <= 1e-3) & (diffs >= 1e-12)
        assert not bool(grey.any()), f"{layout} {lc.tag(case)}: cdf differences {diffs[grey].tolist()}"
    assert n_t0 > 0


def test_cases_cover_what_they_are_meant_to():
    for layout, (frags, nfs) in lc.LAYOUTS.items():
        ts = lc.T_INTS[layout]
        assert all(len(t) == len(frags[0]) for t in ts)
        assert any(t.count(0) >= 2 for t in ts) and all(any(v in t for t in ts) for v in (1, 500, lc.T))
    sizes = {n for frags, _ in lc.LAYOUTS.values() for f in frags for n in f}
    assert {0, 1, 64, 65, 70, 130} <= sizes
    assert lc.T_INTS["ragged"][0] == [0, 500, 0, 1000, 0] and lc.LAYOUTS["ragged"][0][0][4] == 70 and lc.LAYOUTS["ragged"][0][2][4] == 130
    # sigma_0 of the two schedules: degenerate and non-degenerate discretised likelihoods
    s0 = [float(torch.sqrt(torch.sigmoid(lc.Schedule("polynomial_2", lc.T, p).gamma[0].double()))) for p in lc.PRECISIONS]
    assert abs(s0[0] - 3.2e-3) <= 1e-4 and abs(s0[1] - 0.2236) <= 1e-4


def test_restated_likelihood_is_the_class_s():
    """WideLoss (log p(h | z_0) without the slice to 9 columns, needed for node_nf = 19) against DiffusionLoss where both apply."""
    batch = lc.Batch("mixed_nf")
    for case in lc.cases("mixed_nf")[::5]:
        a = lc.reference(batch, case, torch.float64, cls=lc.DiffusionLoss)
        b = lc.reference(batch, case, torch.float64, cls=lc.WideLoss)
        assert torch.equal(a["nll"], b["nll"]) and torch.equal(a["terms"], b["terms"])
        assert all(torch.equal(x, y) for x, y in zip(a["dnet"], b["dnet"]))


# ---- the kernels --------------------------------------------------------------------------------------------------------------------
class Rig:
    """A narrow dynamics module (for its oard_config), the one-sub-batch topology of a layout, the batch on the device."""

    def __init__(self, layout, dev):
        from oareactdiff_amd import EGNNDynamics, _capi
        self.capi, self.L = _capi, _capi.lib()
        self.batch = b = lc.Batch(layout)
        self.dev = dev
        cnf, over = lc.OBJECT_MODEL.get(layout, (1, {}))
        self.dyn = EGNNDynamics(model_config=dict(NARROW, **over), fragment_names=["R", "TS", "P"] if b.K == 3 else [f"o{k}" for k in range(b.K)],
                                node_nfs=b.node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
        self.cfg = self.dyn._config()
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev).cuda_stream
            self.topo = self.dyn._get_train_topology(self.cfg, None, b.n_frag_switch, b.combined_mask, self.stream, device=dev)
        assert self.topo.B == b.B and self.topo.N == b.combined_mask.numel()
        up = lambda ts: [t.to(dev).contiguous() for t in ts]
        self.pos, self.one_hot, self.charge, self.noise = up(b.pos), up(b.one_hot), up(b.charge), up(b.noise)
        self.gamma = {p: lc.Schedule("polynomial_2", lc.T, p).gamma.to(device=dev, dtype=torch.float32).contiguous() for p in lc.PRECISIONS}
        self.refs = {}

    def ref(self, case):
        """(float64 reference, float32 reference) of a case, computed once and shared by the tests; never written to."""
        key = lc.tag(case)
        if key not in self.refs:
            b_total = self.batch.B + PAD
            self.refs[key] = (lc.reference(self.batch, case, torch.float64, b_total), lc.reference(self.batch, case, torch.float32, b_total))
        return self.refs[key]

    def arr(self, ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    @staticmethod
    def f3(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def nan_like(self):
        return [torch.full((m.numel(), nf), float("nan"), device=self.dev) for m, nf in zip(self.batch.masks, self.batch.node_nfs)]

    def inputs_unchanged(self):
        b = self.batch
        for given, on_dev in ((b.pos, self.pos), (b.one_hot, self.one_hot), (b.charge, self.charge), (b.noise, self.noise)):
            assert all(torch.equal(x, y.cpu()) for x, y in zip(given, on_dev)), "a kernel changed an input"

    def prepare(self, case, cfg=None, topo=None, pos=True):
        """oard_loss_prepare -> (rc, z, eps) on the device; outputs NaN-prefilled."""
        t_int, precision, biases, pos_only, fixed_mask = case
        t = torch.tensor(t_int, dtype=torch.float32, device=self.dev)
        z, eps = self.nan_like(), self.nan_like()
        with torch.cuda.device(self.dev):
            rc = self.L.oard_loss_prepare(C.byref(cfg or self.cfg), topo or self.topo.handle, self.arr(self.pos) if pos else None,
                                          self.arr(self.one_hot), self.arr(self.charge), self.arr(self.noise), t.data_ptr(),
                                          self.gamma[precision].data_ptr(), lc.T, self.f3(lc.NORM_VALUES), self.f3(biases), pos_only, fixed_mask,
                                          self.arr(z), self.arr(eps), self.stream)
        torch.cuda.synchronize()
        assert torch.equal(t.cpu(), torch.tensor(t_int, dtype=torch.float32))
        return rc, z, eps

    def terms(self, case, z, eps, net, cfg=None, topo=None, B_total=None, have_eps=True):
        """oard_loss_terms as DDPMTrainer._fused_part calls it for a part of a larger step -> (rc, nll [B], terms [2 K, B_total], dnet);
        every output NaN-prefilled."""
        t_int, precision, biases, pos_only, fixed_mask = case
        b = self.batch
        B_total = b.B + PAD if B_total is None else B_total
        t = torch.tensor(t_int, dtype=torch.float32, device=self.dev)
        keep = [[x.clone() for x in ts] for ts in (z, eps, net)]
        nll = torch.full((b.B,), float("nan"), device=self.dev)
        terms = torch.full((2 * b.K, b.B + PAD), float("nan"), device=self.dev)
        dnet = self.nan_like()
        sc = (C.c_float * b.K)(*lc.scales(b.K))
        with torch.cuda.device(self.dev):
            rc = self.L.oard_loss_terms(C.byref(cfg or self.cfg), topo or self.topo.handle, self.arr(eps) if have_eps else None, self.arr(net),
                                        self.arr(z), self.arr(self.one_hot), self.arr(self.charge), t.data_ptr(),
                                        self.gamma[precision].data_ptr(), lc.T, self.f3(lc.NORM_VALUES), self.f3(biases), sc, pos_only, B_total,
                                        nll.data_ptr(), terms.data_ptr() + 4 * COL0, self.arr(dnet), self.stream)
        torch.cuda.synchronize()
        for before, after in zip(keep, (z, eps, net)):
            assert all(torch.equal(x, y) for x, y in zip(before, after)), "oard_loss_terms changed an input"
        return rc, nll, terms, dnet


_RIGS = {}


def _rig(layout):
    if layout not in _RIGS:
        _RIGS[layout] = Rig(layout, torch.device("cuda:0"))
    return _RIGS[layout]


class Worst:
    """Per output: the largest kernel error with the e32 beside it, and the largest err / max(4 e32, floor)."""

    def __init__(self):
        self.rows, self.case = {}, {}

    def add(self, name, err, e32):
        seen = self.case.get(name, (-1.0, 0.0))
        self.case[name] = (err, e32) if err > seen[0] else seen
        row = self.rows.setdefault(name, [0.0, 0.0, 0.0])
        if err >= row[0]:
            row[0], row[1] = err, e32
        row[2] = max(row[2], err / max(4 * e32, FLOOR))

    def case_done(self, where):
        """One line per case: err (e32) of every output, the largest over the objects."""
        print(where + ": " + ", ".join(f"{name} {err:.2e} ({e32:.2e})" for name, (err, e32) in self.case.items()))
        self.case = {}

    def report(self, title):
        for name, (err, e32, ratio) in self.rows.items():
            print(f"{title} {name}: worst kernel err {err:.2e} (e32 beside it {e32:.2e}), worst err / gate {ratio:.2f}")


def gate(worst, name, got, r64, r32, where):
    err, e32 = rel(got, r64), rel(r32, r64)
    worst.add(name, err, e32)
    assert err <= max(4 * e32, FLOOR), f"{where} {name}: kernel {err:.3e}, float32 DiffusionLoss {e32:.3e}"


def check_prepared(rig, case, z, eps, worst, where):
    """z and eps of oard_loss_prepare against the float64 reference, and the exact zeros of eps."""
    b = rig.batch
    t_int, precision, biases, pos_only, fixed_mask = case
    r64, r32 = rig.ref(case)
    for k in range(b.K):
        zk, ek = z[k].cpu(), eps[k].cpu()
        assert bool(torch.isfinite(zk).all()) and bool(torch.isfinite(ek).all()), f"{where} object {k}: an element was not written"
        for name, got, key in (("z", zk, "z"), ("eps", ek, "eps")):
            gate(worst, name, got, r64[key][k], r32[key][k], f"{where} object {k}")
            gate(worst, name + " features", got[:, lc.POS:], r64[key][k][:, lc.POS:], r32[key][k][:, lc.POS:], f"{where} object {k}")
        if pos_only:
            assert not bool(ek[:, lc.POS:].any()), f"{where} object {k}: feature noise under pos_only"
        if (fixed_mask >> k) & 1:
            assert not bool(ek.any()), f"{where} object {k}: noise on a fixed object"
        alone = (b.sizes[k] == 1)[b.masks[k]]                        # CoM-free noise of one atom: r - r / 1
        assert not bool(ek[alone][:, :lc.POS].any()), f"{where} object {k}: position noise on a 1-atom group"


def check_terms(rig, case, nll, terms, dnet, worst, where):
    b = rig.batch
    t_int, precision, biases, pos_only, fixed_mask = case
    r64, r32 = rig.ref(case)
    B, K = b.B, b.K
    nll = nll.cpu().double()
    assert bool(torch.isfinite(nll).all()), f"{where}: nll {nll.tolist()}"
    err = float(((nll - r64["nll"]).abs() / r64["nll"].abs()).max())
    e32 = float(((r32["nll"].double() - r64["nll"]).abs() / r64["nll"].abs()).max())
    worst.add("nll", err, e32)
    assert err <= max(4 * e32, FLOOR), f"{where} nll: kernel {err:.3e}, float32 DiffusionLoss {e32:.3e}: {nll.tolist()} vs {r64['nll'].tolist()}"
    terms = terms.cpu()
    own = terms[:, COL0: COL0 + B]
    assert bool(torch.isnan(terms[:, :COL0]).all()) and bool(torch.isnan(terms[:, COL0 + B:]).all()), f"{where}: terms written outside the call's columns"
    assert bool(torch.isfinite(own).all()), f"{where}: a terms entry was not written"
    gate(worst, "terms", own, r64["terms"], r32["terms"], where)
    gate(worst, "terms normalised", own[:K], r64["terms"][:K], r32["terms"][:K], where)
    gate(worst, "terms un-normalised", own[K:], r64["terms"][K:], r32["terms"][K:], where)
    for k in range(K):
        empty = b.sizes[k] == 0
        assert torch.equal(own[k][empty], torch.zeros(int(empty.sum()))) and torch.equal(own[K + k][empty], torch.zeros(int(empty.sum()))), \
            f"{where} object {k}: the terms of an empty group are not exact zeros"
        dk = dnet[k].cpu()
        assert bool(torch.isfinite(dk).all()), f"{where} object {k}: a dnet element was not written"
        gate(worst, "dnet", dk, r64["dnet"][k], r32["dnet"][k], f"{where} object {k}")
        if pos_only:
            assert not bool(dk[:, lc.POS:].any()), f"{where} object {k}: feature gradient under pos_only"


@pytest.mark.gpu
def test_widest_node_nf_is_the_widest_supported():
    rig = _rig("widest")
    for nf, want in ((lc.WIDEST_NF, rig.capi.OARD_OK), (lc.WIDEST_NF + 1, rig.capi.OARD_EINVAL)):
        cfg = rig.dyn._config()
        for k in range(3):
            cfg.node_nf[k] = nf
        assert rig.L.oard_supported(C.byref(cfg)) == want
    assert lc.WIDEST_NF - 4 <= 16


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(lc.LAYOUTS) + list(lc.OBJECT_LAYOUTS))
def test_prepare_matches_float64(layout):
    rig, worst = _rig(layout), Worst()
    for case in lc.cases(layout):
        rc, z, eps = rig.prepare(case)
        assert rc == rig.capi.OARD_OK
        check_prepared(rig, case, z, eps, worst, f"{layout} {lc.tag(case)}")
        worst.case_done(f"prepare {layout} {lc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"prepare {layout}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(lc.LAYOUTS) + list(lc.OBJECT_LAYOUTS))
def test_terms_match_float64(layout):
    """The kernel is fed the float32 roundings of the reference's z, eps and net."""
    rig, worst = _rig(layout), Worst()
    net = [x.to(rig.dev) for x in rig.batch.net]
    for case in lc.cases(layout):
        r64, _ = rig.ref(case)
        z, eps = [x.float().to(rig.dev) for x in r64["z"]], [x.float().to(rig.dev) for x in r64["eps"]]
        rc, nll, terms, dnet = rig.terms(case, z, eps, net)
        assert rc == rig.capi.OARD_OK
        check_terms(rig, case, nll, terms, dnet, worst, f"{layout} {lc.tag(case)}")
        worst.case_done(f"terms {layout} {lc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"terms {layout}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(lc.LAYOUTS) + list(lc.OBJECT_LAYOUTS))
def test_prepare_then_terms_chain(layout):
    """The kernel's own z and eps into oard_loss_terms: the same gates."""
    rig, worst = _rig(layout), Worst()
    net = [x.to(rig.dev) for x in rig.batch.net]
    for case in lc.cases(layout):
        rc, z, eps = rig.prepare(case)
        assert rc == rig.capi.OARD_OK
        rc, nll, terms, dnet = rig.terms(case, z, eps, net)
        assert rc == rig.capi.OARD_OK
        check_terms(rig, case, nll, terms, dnet, worst, f"{layout} {lc.tag(case)} chained")
        worst.case_done(f"chain {layout} {lc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"chain {layout}")


@pytest.mark.gpu
def test_inputs_are_not_mutated_and_bad_arguments_are_refused():
    """Every refused call returns OARD_EINVAL before anything is launched: the NaN-prefilled outputs stay NaN.  Every pointer that is
    passed is a valid device buffer of the layout."""
    rig = _rig("ragged")
    b, capi, L = rig.batch, rig.capi, rig.L
    case = lc.cases("ragged")[0]
    net = [x.to(rig.dev) for x in b.net]
    r64, _ = rig.ref(case)
    z, eps = [x.float().to(rig.dev) for x in r64["z"]], [x.float().to(rig.dev) for x in r64["eps"]]

    def with_nf(nf):
        cfg = rig.dyn._config()
        cfg.node_nf[0] = nf
        return cfg
    # a topology of two sub-batches over the same layout
    multi = C.c_void_p()
    cm, nfs = b.combined_mask.contiguous(), b.n_frag_switch.contiguous()
    with torch.cuda.device(rig.dev):
        capi.check(L.oard_topology_create_parts(C.byref(rig.cfg), C.cast(cm.data_ptr(), C.POINTER(C.c_int64)),
                                                C.cast(nfs.data_ptr(), C.POINTER(C.c_int64)), cm.numel(), 2, C.byref(multi)), "two parts")
    try:
        refused = [dict(cfg=with_nf(4)), dict(cfg=with_nf(21)), dict(topo=multi)]
        for kw in refused + [dict(pos=False)]:
            rc, zz, ee = rig.prepare(case, **kw)
            assert rc == capi.OARD_EINVAL, kw
            assert all(bool(torch.isnan(x).all()) for x in zz + ee), f"{kw}: something was launched"
        for kw in refused + [dict(B_total=0), dict(B_total=-1), dict(have_eps=False)]:
            rc, nll, terms, dnet = rig.terms(case, z, eps, net, **kw)
            assert rc == capi.OARD_EINVAL, kw
            assert all(bool(torch.isnan(x).all()) for x in [nll, terms] + dnet), f"{kw}: something was launched"
    finally:
        L.oard_topology_destroy(multi)
    # ... and the accepted call leaves every input as it was (prepare / terms assert it for t_int, z, eps, net)
    rc, zz, ee = rig.prepare(case)
    assert rc == capi.OARD_OK
    rc, *_ = rig.terms(case, zz, ee, net)
    assert rc == capi.OARD_OK
    rig.inputs_unchanged()
    assert all(torch.equal(x.cpu(), y) for x, y in zip(net, b.net))


# MEASURED on an MI355X, per layout over its 48 / 72 cases: worst kernel err (e32 beside it), worst err / max(4 e32, 2^-21).
#                 prepare: z                  eps                        terms: nll                 terms                      dnet
# ragged          7.88e-08 (7.88e-08) 0.17    7.06e-08 (7.06e-08) 0.15   2.34e-07 (1.71e-07) 0.41   7.09e-08 (1.61e-07) 0.12   8.32e-08 (8.32e-08) 0.17
# mixed_nf        9.15e-08 (7.93e-08) 0.19    4.93e-08 (4.93e-08) 0.10   2.72e-07 (8.69e-08) 0.57   6.17e-08 (3.78e-08) 0.13   8.74e-08 (5.05e-08) 0.18
# empty_group     9.44e-08 (9.44e-08) 0.20    4.48e-08 (4.48e-08) 0.09   2.30e-07 (5.37e-08) 0.48   1.12e-07 (1.12e-07) 0.23   1.38e-07 (1.38e-07) 0.25
# widest          9.35e-08 (9.35e-08) 0.20    5.13e-08 (5.13e-08) 0.11   2.12e-07 (2.12e-07) 0.34   4.27e-08 (3.50e-08) 0.09   1.11e-07 (6.13e-08) 0.23
# one_object      1.10e-07 (7.46e-08) 0.23    3.66e-08 (3.66e-08) 0.08   2.27e-07 (3.01e-07) 0.41   8.71e-08 (5.22e-08) 0.18   3.77e-08 (3.87e-08) 0.08
# two_objects     7.21e-08 (8.92e-08) 0.15    7.24e-08 (6.35e-08) 0.15   2.71e-07 (5.95e-08) 0.57   8.48e-08 (8.48e-08) 0.18   9.39e-08 (9.39e-08) 0.20
# four_objects    1.01e-07 (8.42e-08) 0.21    4.32e-08 (4.32e-08) 0.09   2.73e-07 (9.34e-08) 0.57   7.86e-08 (7.86e-08) 0.16   8.53e-08 (8.53e-08) 0.18
# eight_objects   1.14e-07 (8.72e-08) 0.24    4.09e-08 (4.09e-08) 0.09   2.48e-07 (5.61e-08) 0.52   1.17e-07 (9.80e-08) 0.25   1.20e-07 (5.10e-08) 0.25
# The chained run (the kernel's own z and eps) gives the same nll and dnet figures; its terms: ragged 7.79e-08 (3.29e-08) 0.16.
# All of it - the four layouts, 240 cases, three tests - takes 1.5 s of test time.
