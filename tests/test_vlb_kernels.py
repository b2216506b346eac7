"""k_eval_prep and k_vlb_terms (behind oard_loss_eval_prepare / oard_loss_eval_terms) on their own against
oareactdiff_amd.loss.DiffusionLoss(training=False) in float64 on the CPU, on the layouts of tests/_loss_cases.py with a second noise
block (tests/_vlb_cases.py): (sample, object) groups of 0, 1, 64, 65, 70 and 130 atoms, node_nf of 5 / 7 / 9 / 19, t = 1 / 500 / T, both
schedules, non-zero norm_biases, pos_only, fixed objects, a position normaliser of 2 (delta_log_px != 0).  The network is never run:
`net_t` / `net_0` are random tensors.

The gate of every output is the project's rule of tests/test_loss_kernels.py: err <= max(4 e32, 2^-21), e32 = the same DiffusionLoss in
float32 on the CPU against its float64 run.  Tensors (z_t, eps_t, z_0, eps_0; also on their feature block alone) and every row block of
`terms`: max|x - ref| / max|ref| of the block.  nll cancels (neg_log_constants is negative, the rest positive), so its error is taken per
sample relative to the sum of the absolute values of that sample's contributions, and e32 the same way; the largest over the batch.

`terms` has B + PAD columns and the call owns [COL0, COL0 + B); every output is NaN-filled before the call (a missing write shows) and
sits between guard cells (a write out of range shows).  The empty group's five entries are exact zeros.

MEASURED on an MI355X, the worst case of every output over the four layouts and their 48 cases each - kernel err (e32 beside it),
largest err / gate:
  oard_loss_eval_prepare  z_t 1.16e-07 (1.16e-07) 0.24   z_t features 8.84e-08 (8.84e-08) 0.19   eps_t 7.06e-08 (7.06e-08) 0.15
                          z_0 8.79e-08 (6.11e-08) 0.18   z_0 features 9.03e-08 (9.03e-08) 0.19   eps_0 7.78e-08 (7.78e-08) 0.16
                          eps_t / eps_0 features 0 (0)
  oard_loss_eval_terms    nll 7.53e-08 (2.00e-06) 0.12   error_t normalised 4.80e-08 (1.23e-07) 0.10   error_t 4.36e-08 (6.29e-08) 0.09
                          loss_0_x 1.21e-07 (1.21e-07) 0.25   loss_0_cat 6.16e-08 (3.97e-07) 0.11   loss_0_charge 3.69e-08 (6.26e-07) 0.06
                          SNR_weight 4.38e-08 (3.78e-05) 0.04   neg_log_constants 2.83e-08 (2.83e-08) 0.06
  prepare -> terms        the same figures to the digits shown (the kernel's own z_0 / eps feed it)
The float32 DiffusionLoss loses SNR_weight to cancellation (e32 up to 3.8e-05) and with it nll (2e-06); the kernel reads the float64-made
table and sums in double.  With 1, 2, 4 and 8 objects per reaction (_loss_cases.OBJECT_LAYOUTS): largest err / gate 0.23 (z_t).  All of it - four layouts, 192 cases, three tests - takes 5.5 s of test time.  Per layout: run with -s."""
import ctypes as C

import pytest
import torch

import _vlb_cases as vc
import test_loss_kernels as tlk
from _cases import rel

pytestmark = pytest.mark.gpu

FLOOR = tlk.FLOOR
PAD, COL0 = 3, 2
GUARD = 8                              # guard cells on either side of every output
BLOCKS = ("error_t normalised", "error_t", "loss_0_x", "loss_0_cat", "loss_0_charge")


class Rig:
    """A narrow dynamics module (for its oard_config), the one-sub-batch topology of a layout, the batch on the device."""

    def __init__(self, layout, dev):
        from oareactdiff_amd import EGNNDynamics, _capi
        from oareactdiff_amd.trainer import vlb_snr_table
        self.capi, self.L = _capi, _capi.lib()
        self.batch = b = vc.Batch(layout)
        self.dev = dev
        cnf, over = vc.OBJECT_MODEL.get(layout, (1, {}))
        self.dyn = EGNNDynamics(model_config=dict(tlk.NARROW, **over), fragment_names=["R", "TS", "P"] if b.K == 3 else [f"o{k}" for k in range(b.K)],
                                node_nfs=b.node_nfs, edge_nf=0, condition_nf=cnf, device=dev)
        self.cfg = self.dyn._config()
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev).cuda_stream
            self.topo = self.dyn._get_train_topology(self.cfg, None, b.n_frag_switch, b.combined_mask, self.stream, device=dev)
        assert self.topo.B == b.B and self.topo.N == b.combined_mask.numel()
        up = lambda ts: [t.to(dev).contiguous() for t in ts]              # noqa: E731
        self.pos, self.one_hot, self.charge = up(b.pos), up(b.one_hot), up(b.charge)
        self.noise, self.noise0, self.net, self.net0 = up(b.noise), up(b.noise0), up(b.net), up(b.net0)
        sch = {p: vc.Schedule("polynomial_2", vc.T, p) for p in vc.PRECISIONS}
        self.gamma = {p: s.gamma.to(device=dev, dtype=torch.float32).contiguous() for p, s in sch.items()}
        self.snr = {p: vlb_snr_table(s).to(dev) for p, s in sch.items()}
        self.refs = {}

    def ref(self, case):
        """(float64 reference, float32 reference) of a case, computed once and shared by the tests; never written to."""
        key = vc.tag(case)
        if key not in self.refs:
            self.refs[key] = (vc.reference(self.batch, case, torch.float64), vc.reference(self.batch, case, torch.float32))
        return self.refs[key]

    def arr(self, ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    @staticmethod
    def f3(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def guarded(self, shape):
        """A NaN-filled output of `shape` inside a flat buffer with GUARD cells of a sentinel on either side -> (buffer, view)."""
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), -7.25, device=self.dev)
        buf[GUARD: GUARD + n] = float("nan")
        return buf, buf[GUARD: GUARD + n].view(*shape)

    def guards_intact(self, buf):
        return bool((buf[:GUARD] == -7.25).all()) and bool((buf[-GUARD:] == -7.25).all())

    def nodes(self):
        pairs = [self.guarded((m.numel(), nf)) for m, nf in zip(self.batch.masks, self.batch.node_nfs)]
        return [p[0] for p in pairs], [p[1] for p in pairs]

    def inputs_unchanged(self):
        b = self.batch
        for given, on_dev in ((b.pos, self.pos), (b.one_hot, self.one_hot), (b.charge, self.charge), (b.noise, self.noise),
                              (b.noise0, self.noise0), (b.net, self.net), (b.net0, self.net0)):
            assert all(torch.equal(x, y.cpu()) for x, y in zip(given, on_dev)), "a kernel changed an input"

    def prepare(self, case, t_override=None):
        """oard_loss_eval_prepare -> (rc, [z_t, eps_t, z_0, eps_0], their guard buffers)."""
        t_int, precision, biases, pos_only, fixed_mask = case
        t = torch.tensor(t_int if t_override is None else t_override, dtype=torch.float32, device=self.dev)
        bufs, outs = zip(*[self.nodes() for _ in range(4)])
        with torch.cuda.device(self.dev):
            rc = self.L.oard_loss_eval_prepare(C.byref(self.cfg), self.topo.handle, self.arr(self.pos), self.arr(self.one_hot),
                                               self.arr(self.charge), self.arr(self.noise), self.arr(self.noise0), t.data_ptr(),
                                               self.gamma[precision].data_ptr(), vc.T, self.f3(vc.NORM_VALUES), self.f3(biases), pos_only,
                                               fixed_mask, self.arr(outs[0]), self.arr(outs[1]), self.arr(outs[2]), self.arr(outs[3]),
                                               self.stream)
        torch.cuda.synchronize()
        return rc, list(outs), [x for bs in bufs for x in bs]

    def terms(self, case, eps_t, eps_0, z_0, delta_log_px, t_override=None):
        """oard_loss_eval_terms for a part of a larger table -> (rc, nll [B], terms [5 K + 2, B + PAD], guard buffers)."""
        t_int, precision, biases, pos_only, fixed_mask = case
        b = self.batch
        t = torch.tensor(t_int if t_override is None else t_override, dtype=torch.float32, device=self.dev)
        keep = [[x.clone() for x in ts] for ts in (eps_t, eps_0, z_0)]
        nll_buf, nll = self.guarded((b.B,))
        terms_buf, terms = self.guarded((5 * b.K + 2, b.B + PAD))
        sc = (C.c_float * b.K)(*vc.lc.scales(b.K))
        with torch.cuda.device(self.dev):
            rc = self.L.oard_loss_eval_terms(C.byref(self.cfg), self.topo.handle, self.arr(eps_t), self.arr(self.net), self.arr(eps_0),
                                             self.arr(self.net0), self.arr(z_0), self.arr(self.one_hot), self.arr(self.charge), t.data_ptr(),
                                             self.gamma[precision].data_ptr(), self.snr[precision].data_ptr(), vc.T, self.f3(vc.NORM_VALUES),
                                             self.f3(biases), sc, pos_only, float(delta_log_px), b.B + PAD, nll.data_ptr(),
                                             terms.data_ptr() + 4 * COL0, self.stream)
        torch.cuda.synchronize()
        for before, after in zip(keep, (eps_t, eps_0, z_0)):
            assert all(torch.equal(x, y) for x, y in zip(before, after)), "oard_loss_eval_terms changed an input"
        return rc, nll, terms, [nll_buf, terms_buf]


_RIGS = {}


def _rig(layout):
    if layout not in _RIGS:
        _RIGS[layout] = Rig(layout, torch.device("cuda:0"))
    return _RIGS[layout]


def gate(worst, name, got, r64, r32, where):
    err, e32 = rel(got, r64), rel(r32, r64)
    worst.add(name, err, e32)
    assert err <= max(4 * e32, FLOOR), f"{where} {name}: kernel {err:.3e}, float32 DiffusionLoss {e32:.3e}"


def check_prepared(rig, case, outs, bufs, worst, where):
    b = rig.batch
    t_int, precision, biases, pos_only, fixed_mask = case
    r64, r32 = rig.ref(case)
    assert all(rig.guards_intact(x) for x in bufs), f"{where}: a write outside an output"
    for name, got in zip(("z_t", "eps_t", "z_0", "eps_0"), outs):
        for k in range(b.K):
            gk = got[k].cpu()
            assert bool(torch.isfinite(gk).all()), f"{where} {name} object {k}: an element was not written"
            gate(worst, name, gk, r64[name][k], r32[name][k], f"{where} object {k}")
            gate(worst, name + " features", gk[:, vc.POS:], r64[name][k][:, vc.POS:], r32[name][k][:, vc.POS:], f"{where} object {k}")
            if name.startswith("eps"):
                if pos_only:
                    assert not bool(gk[:, vc.POS:].any()), f"{where} {name} object {k}: feature noise under pos_only"
                if (fixed_mask >> k) & 1:
                    assert not bool(gk.any()), f"{where} {name} object {k}: noise on a fixed object"
                alone = (b.sizes[k] == 1)[b.masks[k]]                    # CoM-free noise of one atom: r - r / 1
                assert not bool(gk[alone][:, :vc.POS].any()), f"{where} {name} object {k}: position noise on a 1-atom group"


def check_terms(rig, case, nll, terms, bufs, worst, where):
    b = rig.batch
    r64, r32 = rig.ref(case)
    B, K = b.B, b.K
    assert all(rig.guards_intact(x) for x in bufs), f"{where}: a write outside an output"
    nll = nll.cpu().double()
    assert bool(torch.isfinite(nll).all()), f"{where}: nll {nll.tolist()}"
    err = float(((nll - r64["nll"]).abs() / r64["contrib"]).max())
    e32 = float(((r32["nll"].double() - r64["nll"]).abs() / r64["contrib"]).max())
    worst.add("nll", err, e32)
    assert err <= max(4 * e32, FLOOR), f"{where} nll: kernel {err:.3e}, float32 DiffusionLoss {e32:.3e}: {nll.tolist()} vs {r64['nll'].tolist()}"
    terms = terms.cpu()
    own = terms[:, COL0: COL0 + B]
    assert bool(torch.isnan(terms[:, :COL0]).all()) and bool(torch.isnan(terms[:, COL0 + B:]).all()), f"{where}: terms written outside the call's columns"
    assert bool(torch.isfinite(own).all()), f"{where}: a terms entry was not written"
    for i, name in enumerate(BLOCKS):
        gate(worst, name, own[i * K: (i + 1) * K], r64["terms"][i * K: (i + 1) * K], r32["terms"][i * K: (i + 1) * K], where)
    gate(worst, "SNR_weight", own[5 * K], r64["terms"][5 * K], r32["terms"][5 * K], where)
    gate(worst, "neg_log_constants", own[5 * K + 1], r64["terms"][5 * K + 1], r32["terms"][5 * K + 1], where)
    for k in range(K):
        empty = b.sizes[k] == 0
        for i in range(5):
            assert torch.equal(own[i * K + k][empty], torch.zeros(int(empty.sum()))), f"{where} object {k}: {BLOCKS[i]} of an empty group is not an exact zero"


@pytest.mark.parametrize("layout", list(vc.LAYOUTS) + list(vc.OBJECT_LAYOUTS))
def test_prepare_matches_float64(layout):
    rig, worst = _rig(layout), tlk.Worst()
    for case in vc.cases(layout):
        rc, outs, bufs = rig.prepare(case)
        assert rc == rig.capi.OARD_OK
        check_prepared(rig, case, outs, bufs, worst, f"{layout} {vc.tag(case)}")
        worst.case_done(f"prepare {layout} {vc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"eval prepare {layout}")


@pytest.mark.parametrize("layout", list(vc.LAYOUTS) + list(vc.OBJECT_LAYOUTS))
def test_terms_match_float64(layout):
    """The kernel is fed the float32 roundings of the reference's eps_t, eps_0 and z_0."""
    rig, worst = _rig(layout), tlk.Worst()
    for case in vc.cases(layout):
        r64, _ = rig.ref(case)
        f = lambda key: [x.float().to(rig.dev) for x in r64[key]]         # noqa: E731
        rc, nll, terms, bufs = rig.terms(case, f("eps_t"), f("eps_0"), f("z_0"), r64["delta_log_px"])
        assert rc == rig.capi.OARD_OK
        check_terms(rig, case, nll, terms, bufs, worst, f"{layout} {vc.tag(case)}")
        worst.case_done(f"terms {layout} {vc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"eval terms {layout}")


@pytest.mark.parametrize("layout", list(vc.LAYOUTS) + list(vc.OBJECT_LAYOUTS))
def test_prepare_then_terms_chain(layout):
    """The kernel's own eps_t, eps_0 and z_0 into oard_loss_eval_terms: the same gates."""
    rig, worst = _rig(layout), tlk.Worst()
    for case in vc.cases(layout):
        r64, _ = rig.ref(case)
        rc, outs, bufs = rig.prepare(case)
        assert rc == rig.capi.OARD_OK
        rc, nll, terms, bufs2 = rig.terms(case, outs[1], outs[3], outs[2], r64["delta_log_px"])
        assert rc == rig.capi.OARD_OK
        check_terms(rig, case, nll, terms, bufs + bufs2, worst, f"{layout} {vc.tag(case)} chained")
        worst.case_done(f"chain {layout} {vc.tag(case)}")
    rig.inputs_unchanged()
    worst.report(f"eval chain {layout}")


def test_table_indices_are_clamped():
    """t_int outside [0, T] (negative, beyond T, NaN) reads the tables' end entries and nothing else: the results are those of the
    clamped time steps (NaN: entry 0), and every guard cell is intact."""
    rig = _rig("empty_group")
    case = vc.cases("empty_group")[0]
    wild, clamped = [-3.0e9, 2.5e9], [0.0, float(vc.T)]
    a = rig.prepare(case, t_override=wild)
    b = rig.prepare(case, t_override=clamped)
    c = rig.prepare(case, t_override=[float("nan"), float("inf")])
    assert a[0] == b[0] == c[0] == rig.capi.OARD_OK
    for x, y, z in zip(a[1], b[1], c[1]):
        assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(x, y, z))
    assert all(rig.guards_intact(x) for x in a[2] + c[2])
    ta = rig.terms(case, a[1][1], a[1][3], a[1][2], 0.0, t_override=wild)
    tb = rig.terms(case, a[1][1], a[1][3], a[1][2], 0.0, t_override=clamped)
    assert ta[0] == tb[0] == rig.capi.OARD_OK
    assert torch.equal(ta[1], tb[1]) and torch.equal(ta[2][:, COL0: COL0 + 2], tb[2][:, COL0: COL0 + 2])
    assert all(rig.guards_intact(x) for x in ta[3])


def test_bad_arguments_are_refused_before_a_launch():
    rig = _rig("ragged")
    b, capi, L = rig.batch, rig.capi, rig.L
    case = vc.cases("ragged")[0]
    t_int, precision, biases, pos_only, fixed_mask = case
    t = torch.tensor(t_int, dtype=torch.float32, device=rig.dev)
    multi = C.c_void_p()
    cm, nfs = b.combined_mask.contiguous(), b.n_frag_switch.contiguous()
    with torch.cuda.device(rig.dev):
        capi.check(L.oard_topology_create_parts(C.byref(rig.cfg), C.cast(cm.data_ptr(), C.POINTER(C.c_int64)),
                                                C.cast(nfs.data_ptr(), C.POINTER(C.c_int64)), cm.numel(), 2, C.byref(multi)), "two parts")
    try:
        def with_nf(nf):
            cfg = rig.dyn._config()
            cfg.node_nf[0] = nf
            return cfg
        nll_buf, nll = rig.guarded((b.B,))
        terms_buf, terms = rig.guarded((5 * b.K + 2, b.B))
        bufs, outs = zip(*[rig.nodes() for _ in range(4)])
        sc = (C.c_float * b.K)(*vc.lc.scales(b.K))
        f3 = rig.f3
        for cfg, topo, T, B in ((with_nf(4), rig.topo.handle, vc.T, b.B), (with_nf(21), rig.topo.handle, vc.T, b.B),
                                (rig.cfg, multi, vc.T, b.B), (rig.cfg, rig.topo.handle, 0, b.B), (rig.cfg, rig.topo.handle, vc.T, 0)):
            with torch.cuda.device(rig.dev):
                if B > 0:
                    rc = L.oard_loss_eval_prepare(C.byref(cfg), topo, rig.arr(rig.pos), rig.arr(rig.one_hot), rig.arr(rig.charge),
                                                  rig.arr(rig.noise), rig.arr(rig.noise0), t.data_ptr(), rig.gamma[precision].data_ptr(), T,
                                                  f3(vc.NORM_VALUES), f3(biases), 0, 0, rig.arr(outs[0]), rig.arr(outs[1]), rig.arr(outs[2]),
                                                  rig.arr(outs[3]), rig.stream)
                    assert rc == capi.OARD_EINVAL
                rc = L.oard_loss_eval_terms(C.byref(cfg), topo, rig.arr(rig.noise), rig.arr(rig.net), rig.arr(rig.noise0), rig.arr(rig.net0),
                                            rig.arr(rig.noise0), rig.arr(rig.one_hot), rig.arr(rig.charge), t.data_ptr(),
                                            rig.gamma[precision].data_ptr(), rig.snr[precision].data_ptr(), T, f3(vc.NORM_VALUES), f3(biases), sc,
                                            0, 0.0, B, nll.data_ptr(), terms.data_ptr(), rig.stream)
                assert rc == capi.OARD_EINVAL
        torch.cuda.synchronize()
        assert bool(torch.isnan(nll).all()) and bool(torch.isnan(terms).all()), "something was launched"
        assert all(bool(torch.isnan(x).all()) for xs in outs for x in xs), "something was launched"
    finally:
        L.oard_topology_destroy(multi)
    rig.inputs_unchanged()
