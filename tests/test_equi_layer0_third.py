"""Layer 0 of an inference forward leaves out the third of EquiMessage that only multiplies vec = 0 (leftnet.py:263-270, 836):
`k_equi_edge_v1` runs 26 of its 39 T2 phases and does not write the middle third of q, the layer-0 form of `k_equi_node_v1` loads
neither that third nor vec[src].  Debug option `equi_l0_skip` (default 1) switches the shortcut off.

Every case runs the same module on the same inputs with the option off and on: the outputs are equal (`torch.equal`: +0 == -0, the
one thing that may differ), and the "on" result is inside the oracle gate of the parity tests (1e-5 of the largest entry, float64
reference).  The suite runs with the NaN-poisoned workspace (conftest), so a read of the unwritten third would not stay finite."""
import contextlib

import pytest
import torch

import leftnet_oracle as oracle
from _cases import LIB_AUTO, THROUGHPUT, Case, debug_options, rel
from test_hip_parity import _args, _dyn, _random_case

pytestmark = pytest.mark.gpu
TOL = 1e-5


@contextlib.contextmanager
def l0_skip(value):
    """The option is not one of conftest's SUITE_OPTIONS: set here, back to the library's default (on) afterwards."""
    from oareactdiff_amd import _capi
    lib = _capi.lib()
    assert lib.oard_debug_option(b"equi_l0_skip", value) == 0
    try:
        yield lib
    finally:
        lib.oard_debug_option(b"equi_l0_skip", 1)


def _off_on(run, expect_taken=True):
    """run() -> list of output tensors; -> (off, on).  The "on" run must have taken the shortcut where the launch shape has it."""
    outs = []
    for value in (0, 1):
        with l0_skip(value) as lib:
            out = run()
            torch.cuda.synchronize()
            taken = lib.oard_debug_option(b"equi_l0_taken", 0) == 0
            assert taken == bool(value and expect_taken), (value, taken)
            outs.append([o.clone() for o in out])
    for a, b in zip(*outs):
        assert torch.equal(a, b) and bool(torch.isfinite(b).all())
    return outs


def _prod_module(num_layers, dev, reflect_equiv=True):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict
    cfg = dict(PRODUCTION_LEFTNET_CONFIG, num_layers=num_layers, reflect_equiv=reflect_equiv)
    sd = synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg, seed=7)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0,
                       condition_nf=1, device=dev)
    dyn.load_state_dict(sd, strict=True)
    return dyn, cfg, sd


def _oracle_gate(out, cfg, sd, xh, ei, t, cond, nfs, cm):
    ref = oracle.dynamics_forward({k: v.double() for k, v in sd.items()}, cfg, [x.double() for x in xh], ei,
                                  t.double(), cond.double(), nfs, cm, 1, nodeframe="exact")
    v = torch.cat([o[:, :3].cpu().double().reshape(-1) for o in out])
    h = torch.cat([o[:, 3:].cpu().double().reshape(-1) for o in out])
    rv = torch.cat([o[:, :3].reshape(-1) for o in ref])
    rh = torch.cat([o[:, 3:].reshape(-1) for o in ref])
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (rel(v, rv), rel(h, rh))


# production widths (H = 196, R = 96: the 4-row 13th tile of every third exists only there), throughput launch shapes pinned
@pytest.mark.parametrize("sizes,pos_scale,num_layers", [
    ([7, 12], 1.0, 3),         # two ragged reactions, A = 522 inner edges (4 x 128 + 10: padding columns on the spare row), nothing masked
    ([9, 30, 5], 2.5, 3),      # the cutoff bites: ragged active list
    ([23, 11], 60.0, 3),       # every inner edge outside the cutoff: the edge kernel returns before its first barrier
    ([7, 12], 1.0, 1),         # layer 0 is also the last layer
    ([7, 12], 2.5, 2),
])
def test_ragged_production_dims_off_equals_on(sizes, pos_scale, num_layers):
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _prod_module(num_layers, dev)
    xh, ei, t, cond, nfs, cm = _random_case(sizes, pos_scale, 5, cfg)
    A = sum(3 * n * (n - 1) for n in sizes)
    assert A % 128 != 0

    def run():
        with torch.no_grad():
            out, _ = dyn([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
        return out
    with debug_options(**THROUGHPUT):
        off, on = _off_on(run)
        n_act = dyn.active_inner_edges()
    assert (n_act == A) if pos_scale == 1.0 else (n_act == 0) if pos_scale >= 60 else (0 < n_act < A), (n_act, A)
    _oracle_gate(on, cfg, sd, xh, ei, t, cond, nfs, cm)


@pytest.mark.parametrize("shapes", ["throughput", "auto"])
@pytest.mark.parametrize("name", ["g2_prod_b2_n23", "g3p_prod_cutoff", "g10p_noreflect_prod", "g10_noreflect_h32", "g6_h32_r32",
                                  "g13_one_object", "g13_eight_objects"])
def test_golden_cases_off_equals_on(name, shapes):
    """The committed fixtures, among them reflect_equiv = False (the XC instantiation of the node kernel) at both widths - under the
    throughput shapes, which take the shortcut, and under the library's default launch heuristics, which send these small cases to the
    latency kernels and the row-lane gather: those run the whole third, and the option must change nothing there either."""
    dev = torch.device("cuda:0")
    c = Case(name)
    dyn = _dyn(c, dev)

    def run():
        with torch.no_grad():
            out, _ = dyn(*_args(c, dev))
        return out
    with debug_options(**(LIB_AUTO if shapes == "auto" else THROUGHPUT)):
        off, on = _off_on(run, expect_taken=shapes == "throughput")
    v, h = c.split([o.cpu() for o in on])
    rv, rh = c.split(c.ref64)
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (rel(v, rv), rel(h, rh))


@pytest.mark.parametrize("reflect_equiv", [True, False])
def test_nothing_reads_the_unwritten_third(reflect_equiv):
    """Workspace poison (0xFF fill before every forward) off and on, shortcut on: the outputs are finite and equal, i.e. no kernel reads
    the third of q that layer 0 no longer writes - not through a padding column, not on a row outside the cutoff."""
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _prod_module(2, dev, reflect_equiv)
    xh, ei, t, cond, nfs, cm = _random_case([9, 30, 5], 2.5, 5, cfg)
    outs = []
    for poison in (0, 1):
        with debug_options(poison=poison, **THROUGHPUT), l0_skip(1) as lib, torch.no_grad():
            out, _ = dyn([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
            torch.cuda.synchronize()
            assert lib.oard_debug_option(b"equi_l0_taken", 0) == 0
            outs.append([o.clone() for o in out])
    for a, b in zip(*outs):
        assert torch.equal(a, b) and bool(torch.isfinite(b).all())


def test_training_mode_never_takes_the_shortcut():
    """The training-mode forward tapes all three thirds of dir_proj's output for the backward pass (which reads the middle third with a
    zero cotangent: 0 x garbage must stay impossible): with the option on, loss and gradients of the smallest gradient fixture are those
    of the option off, bit for bit, and the forward reports that it ran the whole layer."""
    from _grad_cases import CNF, NODE_NFS, GradCase
    from oareactdiff_amd.dynamics import EGNNDynamics
    dev = torch.device("cuda:0")
    c = GradCase("g9_grad_h32")
    res = []
    for value in (0, 1):
        with l0_skip(value) as lib:
            dyn = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0,
                               condition_nf=CNF, device=dev)
            dyn.load_state_dict(c.state_dict(), strict=True)
            loss = c.loss(dyn, torch.float32, dev)
            loss.backward()
            torch.cuda.synchronize()
            assert lib.oard_debug_option(b"equi_l0_taken", 0) != 0
            res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in dyn.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and bool(torch.isfinite(g1[n]).all()), n
    ref_loss = float(c.z["f64_loss"])
    assert abs(float(l1) - ref_loss) <= 2e-5 * abs(ref_loss)
