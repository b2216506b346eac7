"""EquiMessage's rbf_proj from a table in u = exp(-d) instead of an MFMA chain (csrc/oard_rbf_table.h, `k_equi_edge_v1<D, 8, false, true>`,
DESIGN.md section 5).  Debug option `equi_rbf_table` (default 1) switches it off; `equi_rbf_taken` reports whether every layer of the
last forward took it.  The tables are built, checked per layer and cached by the first inference forward on a packed blob.

The table changes the arithmetic of one factor (four FMAs on float64-built entries in place of a 96-term float32 sum), so option on
and option off differ in the last bits: the gate is the float64 golden (1e-5, the parity tests' gate) for both, and on must not be
further from off than off is from the golden.  The suite runs with the NaN-poisoned workspace (conftest)."""
import contextlib

import pytest
import torch

from _cases import THROUGHPUT, Case, debug_options, rel
from test_hip_parity import _args, _dyn, _random_case
from test_equi_layer0_third import _prod_module, l0_skip

pytestmark = pytest.mark.gpu
TOL = 1e-5


@contextlib.contextmanager
def rbf_table(value):
    """The option is not one of conftest's SUITE_OPTIONS: set here, back to the library's default (on) afterwards."""
    from oareactdiff_amd import _capi
    lib = _capi.lib()
    assert lib.oard_debug_option(b"equi_rbf_table", value) == 0
    try:
        yield lib
    finally:
        lib.oard_debug_option(b"equi_rbf_table", 1)


def _taken(lib):
    return lib.oard_debug_option(b"equi_rbf_taken", 0) == 0


def _forward(dyn, args):
    with torch.no_grad():
        out, _ = dyn(*args)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def _flat(out):
    return torch.cat([o.double().reshape(-1).cpu() for o in out])


@pytest.mark.parametrize("name,l0", [("g3_cutoff_ragged", 1), ("g2_prod_b2_n23", 1), ("g2_prod_b2_n23", 0),
                                     ("g13_one_object", 1), ("g13_eight_objects", 1)])
def test_golden_cases_on_and_off(name, l0):
    """H = 32 / R = 8 (no 4-row tiles, ragged active list) and the production widths (H = 196: the 13th tile of every third has 4 real
    rows) with layer 0's skipped third on and off."""
    dev = torch.device("cuda:0")
    c = Case(name)
    dyn = _dyn(c, dev)
    res = {}
    with debug_options(**THROUGHPUT), l0_skip(l0):
        for value in (0, 1):
            with rbf_table(value) as lib:
                res[value] = _forward(dyn, _args(c, dev))
                assert _taken(lib) == bool(value), (value, _taken(lib))
    rv, rh = c.split(c.ref64)
    err = {}
    for value in (0, 1):
        v, h = c.split([o.cpu() for o in res[value]])
        err[value] = (rel(v, rv), rel(h, rh))
        print(f"{name} l0_skip={l0} equi_rbf_table={value}: vel {err[value][0]:.3e} h {err[value][1]:.3e} of the float64 golden")
    off, on = _flat(res[0]), _flat(res[1])
    ref = torch.cat([o.double().reshape(-1) for o in c.ref64])
    d_on_off = float((on - off).abs().max() / off.abs().max())
    e_off = float((off - ref).abs().max() / ref.abs().max())
    print(f"{name} l0_skip={l0}: max|on - off| / max|off| = {d_on_off:.3e}; option off against the golden {e_off:.3e}")
    assert max(err[0]) <= TOL and max(err[1]) <= TOL, err
    assert d_on_off <= e_off, (d_on_off, e_off)


@pytest.mark.parametrize("sizes,pos_scale", [
    ([9, 30, 5], 3.0),         # the cutoff bites: ragged active list, A = 2844 = 22 x 128 + 28 (padding columns)
    ([7, 12], 1.0),            # nothing masked
    ([23, 11], 60.0),          # everything masked: the edge kernel returns before its first barrier
])
def test_ragged_lists_on_a_poisoned_workspace(sizes, pos_scale):
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _prod_module(2, dev)
    xh, ei, t, cond, nfs, cm = _random_case(sizes, pos_scale, 5, cfg)
    args = ([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
    A = sum(3 * n * (n - 1) for n in sizes)
    with debug_options(poison=1, **THROUGHPUT):
        with rbf_table(1) as lib:
            on = _forward(dyn, args)
            assert _taken(lib)
            n_act = dyn.active_inner_edges()
        with rbf_table(0):
            off = _forward(dyn, args)
    assert (n_act == A) if pos_scale == 1.0 else (n_act == 0) if pos_scale >= 60 else (0 < n_act < A), (n_act, A)
    for a in on:
        assert bool(torch.isfinite(a).all())
    d = rel(_flat(on), _flat(off))
    print(f"sizes {sizes} x {pos_scale}: n_act {n_act} of {A}, max|on - off| / max|off| = {d:.3e}")
    assert d <= TOL


def test_parts_and_graph_replay_are_bitwise():
    """Option on: one sub-batch against four, and an eager call against the replay of its captured graph (captured after the eager
    call, which built the tables: a capturing call cannot)."""
    dev = torch.device("cuda:0")
    outs = {}
    for parts in (1, 4):
        # (gcl_persist pinned: its default picks the GCL kernel by the number of sub-batches, and the two group their sums differently)
        with debug_options(parts=parts, gcl_persist=2, **THROUGHPUT), rbf_table(1) as lib:
            dyn, cfg, sd = _prod_module(2, dev)
            xh, ei, t, cond, nfs, cm = _random_case([5, 9, 6, 8], 2.0, 11, cfg)
            args = ([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
            outs[parts] = _forward(dyn, args)
            assert _taken(lib)
            if parts == 1:
                dyn.nan_check = "async"
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side), torch.no_grad():
                    dyn(*args)                                       # eager warm-up on the capture stream
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=side):
                        gout, _ = dyn(*args)
                    assert _taken(lib)
                    g.replay()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize()
                for a, b in zip(outs[1], gout):
                    assert torch.equal(a, b) and bool(torch.isfinite(b).all())
    for a, b in zip(outs[1], outs[4]):
        assert torch.equal(a, b)


def test_a_table_that_fails_its_check_is_not_used():
    """betas x 16: Gaussians four times narrower than the grid was chosen for - the pack-time check must reject every layer's table
    (2.9e-6 of the range against the 2e-7 criterion) and the forward keep the MFMA chain: bitwise the option-off result."""
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _prod_module(2, dev)
    sd = dict(sd)
    sd["model.radial_emb.betas"] = sd["model.radial_emb.betas"] * 16
    dyn.load_state_dict(sd, strict=True)
    xh, ei, t, cond, nfs, cm = _random_case([9, 12], 1.5, 3, cfg)
    args = ([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
    res = {}
    with debug_options(**THROUGHPUT):
        for value in (1, 0):
            with rbf_table(value) as lib:
                res[value] = _forward(dyn, args)
                assert not _taken(lib)
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b) and bool(torch.isfinite(b).all())


def test_training_mode_never_takes_the_table():
    """The backward pass differentiates rbf_proj as a Linear layer: the training-mode forward keeps the MFMA chain, and loss and
    gradients of the smallest gradient fixture are bitwise those of the option off."""
    from _grad_cases import CNF, NODE_NFS, GradCase
    from oareactdiff_amd.dynamics import EGNNDynamics
    dev = torch.device("cuda:0")
    c = GradCase("g9_grad_h32")
    res = []
    for value in (0, 1):
        with rbf_table(value) as lib:
            dyn = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0,
                               condition_nf=CNF, device=dev)
            dyn.load_state_dict(c.state_dict(), strict=True)
            loss = c.loss(dyn, torch.float32, dev)
            loss.backward()
            torch.cuda.synchronize()
            assert not _taken(lib)
            res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in dyn.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1) and g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]) and bool(torch.isfinite(g1[n]).all()), n
