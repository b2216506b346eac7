"""The GCL edge kernels sum the messages of a node inside the wave (`st_msum`, csrc/oard_edge_v1.h) and the node stage adds the few
partial rows they leave (`k_gcl_node_v1<.., MSUM>`) instead of gathering one row per edge (DESIGN.md sections 4, 5).  Inference, streamed
fp32 throughput shapes and the large-batch node stage only; debug option `gcl_msum` (default 1) switches it off, `gcl_msum_taken` says
what the last forward did.

The gate of every accuracy check is the one of the parity tests: 1e-5 of the largest entry against the float64 reference.  The two forms
add the same terms in different orders, so on versus off is compared to rounding and printed, not asserted bit for bit; what IS bit
for bit is the new form against itself however the batch is cut (sub-batches, persistent grid sizes): every reaction starts on a multiple
of 16 columns, so the lanes a node's messages occupy in a wave tile are a property of the reaction alone.  The suite runs with the
NaN-poisoned workspace (conftest)."""
import contextlib

import pytest
import torch

import leftnet_oracle as oracle
from _cases import LIB_AUTO, THROUGHPUT, Case, debug_options, rel
from test_hip_parity import _args, _dyn

pytestmark = pytest.mark.gpu
TOL = 1e-5


@contextlib.contextmanager
def msum(value):
    """The option is not one of conftest's SUITE_OPTIONS: set here, back to the library's default (on) afterwards."""
    from oareactdiff_amd import _capi
    lib = _capi.lib()
    assert lib.oard_debug_option(b"gcl_msum", value) == 0
    try:
        yield lib
    finally:
        lib.oard_debug_option(b"gcl_msum", 1)


def _taken(lib):
    return lib.oard_debug_option(b"gcl_msum_taken", 0) == 0


def _module(hidden, radial, num_layers, dev):
    from oareactdiff_amd.dynamics import EGNNDynamics
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG, state_spec, synthetic_state_dict
    cfg = dict(PRODUCTION_LEFTNET_CONFIG, hidden_channels=hidden, num_radial=radial, num_layers=num_layers)
    sd = synthetic_state_dict(state_spec(cfg, [9, 9, 9], 1), cfg, seed=7)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=["R", "TS", "P"], node_nfs=[9, 9, 9], edge_nf=0,
                       condition_nf=1, device=dev)
    dyn.load_state_dict(sd, strict=True)
    return dyn, cfg, sd


def _batch(natm, pos_scale, seed):
    """natm[k][b] = atoms of object k in reaction b (the objects of a reaction may differ in size); production feature layout."""
    from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
    g = torch.Generator().manual_seed(seed)
    natm = [torch.tensor(n) for n in natm]
    masks = [get_mask_for_frag(n) for n in natm]
    cm = torch.cat(masks)
    nfs = get_n_frag_switch(natm)
    ei = get_edges_index(cm, remove_self_edge=True)
    B = natm[0].numel()
    xh = []
    for m, n_of in zip(masks, natm):
        n = m.numel()
        pos = torch.randn(n, 3, generator=g)
        mean = torch.zeros(B, 3).index_add_(0, m, pos) / n_of.float().unsqueeze(1)
        pos = (pos - mean[m]) * pos_scale
        typ = torch.randint(0, 4, (n,), generator=g)
        feat = torch.zeros(n, 6)
        feat[torch.arange(n), typ] = 1.0
        feat[:, 5] = torch.tensor([1.0, 6.0, 7.0, 8.0])[typ]
        xh.append(torch.cat([pos, feat], 1))
    return xh, ei, torch.rand(B, 1, generator=g), torch.rand(B, 1, generator=g), nfs, cm


def _run(dyn, batch, dev):
    xh, ei, t, cond, nfs, cm = batch
    with torch.no_grad():
        out, _ = dyn([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def _gate(out, cfg, sd, batch):
    xh, ei, t, cond, nfs, cm = batch
    ref = oracle.dynamics_forward({k: v.double() for k, v in sd.items()}, cfg, [x.double() for x in xh], ei,
                                  t.double(), cond.double(), nfs, cm, 1, nodeframe="exact")
    v = torch.cat([o[:, :3].cpu().double().reshape(-1) for o in out])
    h = torch.cat([o[:, 3:].cpu().double().reshape(-1) for o in out])
    rv = torch.cat([o[:, :3].reshape(-1) for o in ref])
    rh = torch.cat([o[:, 3:].reshape(-1) for o in ref])
    print(f"vs float64 oracle: vel {rel(v, rv):.2e} h {rel(h, rh):.2e}")
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (rel(v, rv), rel(h, rh))


# reactions whose objects have 1 / 2 / 5, 3 / 17 / 4 and 23 / 23 / 23 atoms: a one-atom object has no inner column, the tiles of the first
# reaction hold up to eight segments, the 16 inner columns of a 17-atom object's node straddle one tile boundary, the 46 inter-object columns
# of a 23-atom reaction's node straddle two or three, and the first reaction's lists (22 inner, 34 inter-object columns) end in tiles that are mostly padding
RAGGED = [[1, 3, 23], [2, 17, 23], [5, 4, 23]]


@pytest.mark.parametrize("name", ["g6_h32_r32", "g10_noreflect_h32", "g2_prod_b2_n23", "g13_one_object", "g13_eight_objects"])
def test_golden_cases_on_and_off_pass_the_gate(name):
    """The committed fixtures (H = 32 twice, 196 x 96 once; one object: no inter-object column at all, CX = 0; eight objects), throughput shapes pinned, option off and on: both inside the fixture's gate
    against the float64 reference; the difference between the two forms is printed (profiles/gcl_msum.txt)."""
    dev = torch.device("cuda:0")
    c = Case(name)
    dyn = _dyn(c, dev)
    rv, rh = c.split(c.ref64)
    outs = []
    for value in (0, 1):
        with debug_options(**THROUGHPUT), msum(value) as lib, torch.no_grad():
            out, _ = dyn(*_args(c, dev))
            torch.cuda.synchronize()
            assert _taken(lib) == bool(value)
        v, h = c.split([o.cpu() for o in out])
        print(f"{name} gcl_msum={value}: vs ref64 vel {rel(v, rv):.2e} h {rel(h, rh):.2e}")
        assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (value, rel(v, rv), rel(h, rh))
        outs.append((v, h))
    print(f"{name}: on vs off vel {rel(outs[1][0], outs[0][0]):.2e} h {rel(outs[1][1], outs[0][1]):.2e}")


@pytest.mark.parametrize("hidden,radial", [(32, 32), (196, 96)])
def test_ragged_reactions_on_and_off_pass_the_gate(hidden, radial):
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _module(hidden, radial, 3, dev)
    batch = _batch(RAGGED, 1.5, 5)
    outs = []
    for value in (0, 1):
        with debug_options(**THROUGHPUT), msum(value) as lib:
            outs.append(_run(dyn, batch, dev))
            assert _taken(lib) == bool(value)
        _gate(outs[-1], cfg, sd, batch)
    a = torch.cat([o.reshape(-1) for o in outs[0]]).cpu()
    b = torch.cat([o.reshape(-1) for o in outs[1]]).cpu()
    print(f"ragged H={hidden}: on vs off {rel(b, a):.2e}")


@pytest.mark.parametrize("hidden,radial", [(32, 32), (196, 96)])
def test_the_sums_do_not_depend_on_how_the_batch_is_cut(hidden, radial):
    """gcl_msum = 1: sub-batches (parts 1 / 2 / 3) under the tile kernel and under the persistent kernel, and the persistent kernel over
    grids of 1, 3 and 5 workgroups (shares that end in full and in half rounds) - bit-identical, kernel by kernel."""
    dev = torch.device("cuda:0")
    dyn_layers = 2
    batch = _batch([r + [6] for r in RAGGED], 1.5, 9)           # four reactions, so that three parts are 1 + 1 + 2 of them
    for persist in (0, 2):
        outs = []
        for parts in (1, 2, 3):
            with debug_options(parts=parts, gcl_persist=persist, **THROUGHPUT), msum(1) as lib:
                dyn, cfg, sd = _module(hidden, radial, dyn_layers, dev)     # (the topology, hence the split, is made per module)
                outs.append(_run(dyn, batch, dev))
                assert _taken(lib)
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    grids = []
    for grid in (0, 1, 3, 5):
        with debug_options(parts=1, gcl_persist=2, gcl_grid=grid, **THROUGHPUT), msum(1) as lib:
            dyn, cfg, sd = _module(hidden, radial, dyn_layers, dev)
            grids.append(_run(dyn, batch, dev))
            assert _taken(lib)
    for other in grids[1:]:
        for a, b in zip(grids[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("hidden,radial", [(32, 32), (196, 96)])
def test_persistent_and_tile_kernel_group_the_sums_alike(hidden, radial):
    """The persistent kernel adds P[src] + Q[tgt] behind S1's product and the tile kernel in front of it (csrc/oard_edge_p.h: a last-bit
    difference in m itself, gated at 2e-6 by test_hip_parity), so the two can only be compared bit for bit where no launch has an S1
    stage: one layer (first and last at once) over reactions of one-atom objects, whose columns are all inter-object.  There the two
    kernels compute the same m, and equal outputs mean equal grouping of the sums (21 reactions: every wave tile holds one reaction's three
    two-column segments and ten padding columns; the persistent kernel deals the 21 wave tiles as half-tiles, the last one ragged).  With an
    S1 stage - the ragged batch, two layers - the bound is the existing one of the two kernels against each other, 2e-6."""
    dev = torch.device("cuda:0")
    ones = [[1] * 21, [1] * 21, [1] * 21]
    for layers, batch, bitwise in ((1, _batch(ones, 1.0, 3), True), (2, _batch(RAGGED, 1.5, 5), False)):
        outs = []
        for persist in (0, 2):
            with debug_options(parts=1, gcl_persist=persist, **THROUGHPUT), msum(1) as lib:
                dyn, cfg, sd = _module(hidden, radial, layers, dev)
                outs.append(_run(dyn, batch, dev))
                assert _taken(lib)
        for a, b in zip(*outs):
            if bitwise:
                assert torch.equal(a, b) and bool(torch.isfinite(a).all())
            else:
                assert (a - b).abs().max() <= 2e-6 * max(float(a.abs().max()), 1e-6)
        _gate(outs[1], cfg, sd, batch)


@pytest.mark.parametrize("persist", [0, 2])
def test_the_node_stage_reads_only_partial_rows_that_were_written(persist):
    """Workspace poison (0xFF fill before every forward) off and on, gcl_msum on: finite and equal outputs - no partial row of a padding
    column, of a lane that is not a segment head or of an earlier call is read."""
    dev = torch.device("cuda:0")
    dyn, cfg, sd = _module(196, 96, 2, dev)
    batch = _batch(RAGGED, 2.5, 5)
    outs = []
    for poison in (0, 1):
        with debug_options(poison=poison, gcl_persist=persist, **THROUGHPUT), msum(1) as lib:
            outs.append(_run(dyn, batch, dev))
            assert _taken(lib)
    for a, b in zip(*outs):
        assert torch.equal(a, b) and bool(torch.isfinite(b).all())


def test_latency_shapes_keep_the_message_rows():
    """B = 1 under the library's own launch heuristics: latency edge kernels and the row-lane node stage - the old form, inside its gate."""
    dev = torch.device("cuda:0")
    c = Case("g2s_prod_b1_n5")
    dyn = _dyn(c, dev)
    with debug_options(**LIB_AUTO), msum(1) as lib, torch.no_grad():
        out, _ = dyn(*_args(c, dev))
        torch.cuda.synchronize()
        assert not _taken(lib)
    v, h = c.split([o.cpu() for o in out])
    rv, rh = c.split(c.ref64)
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (rel(v, rv), rel(h, rh))


def test_training_mode_keeps_the_message_rows():
    """The training-mode forward tapes agg for the backward pass: it reports the old form, and loss and gradients are those of the option
    off bit for bit; the loss is inside the gradient fixture's gate."""
    from _grad_cases import CNF, NODE_NFS, GradCase
    from oareactdiff_amd.dynamics import EGNNDynamics
    dev = torch.device("cuda:0")
    c = GradCase("g9_grad_h32")
    res = []
    for value in (0, 1):
        with msum(value) as lib:
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
    ref_loss = float(c.z["f64_loss"])
    assert abs(float(l1) - ref_loss) <= 2e-5 * abs(ref_loss)
