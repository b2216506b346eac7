"""Reactions of 1, 2, 5 and 8 objects instead of three, at production width (H = 196, R = 96, three layers), and one step beyond each
limit of the wrapper.  The library takes 1 to 8 objects (OARD_MAX_OBJECTS), feature widths node_nf - 3 of 1 to 16 and in_hidden_channels
up to 16; the fixtures g13_* (tests/_cases.py) pin the small width to the reference, here the float64 oracle - which those fixtures pin to
the reference at 1, 2, 4 and 8 objects - is evaluated in the test on the same inputs, once per layout and process.

With ONE object every edge is an inner edge: E == A, the inter-object GCL launch, k_fill_edges, layer 0's u0 / c0row shortcut and the
last layer's inter-object rows all work on zero rows.  [[8, 8, 4, 2, 2]] makes E == A == 128, exactly one 128-row tile; one more two-atom
sample gives a tile plus two rows.

Gate: max|ours - ref| / max|ref| <= 1e-5 on velocities and on features, under the suite's launch shapes and under the library's own."""
import ctypes as C
import functools

import pytest
import torch

import leftnet_oracle as oracle
from _cases import LIB_AUTO, THROUGHPUT, debug_options, rel

pytestmark = pytest.mark.gpu
TOL = 1e-5
#: name -> (atoms per object and sample, pos_scale, enforce_same_encoding)
LAYOUTS = {
    "one_tile": ([[8, 8, 4, 2, 2]], 1.0, None),                         # E == A == 128
    "one_tile_plus_two": ([[8, 8, 4, 2, 2, 2]], 1.0, None),             # 130 rows
    "one_ragged": ([[23, 7, 1, 40]], 1.0, None),                        # a single-atom sample, a group larger than 32
    "one_ragged_cut": ([[23, 7, 1, 40]], 2.5, None),                    # ... and the cutoff bites
    "one_molecule": ([[2]], 1.0, None),                                 # a single two-atom molecule
    "two_aliased": ([[9, 0, 5], [12, 30, 5]], 1.0, [1]),                # an empty group; object 1 shares object 0's encoder and decoder
    "five": ([[40, 3], [1, 17], [5, 5], [2, 33], [7, 1]], 1.0, None),
    "eight": ([[k + 1, 8 - k] for k in range(8)], 1.0, None),           # groups of 1 to 8 atoms, 36 nodes per sample
    "eight_cut": ([[k + 1, 8 - k] for k in range(8)], 2.5, None),
}


def _cfg(**over):
    from oareactdiff_amd.spec import PRODUCTION_LEFTNET_CONFIG
    return dict(PRODUCTION_LEFTNET_CONFIG, num_layers=3, **over)


def _batch(natm, pos_scale, seed, node_nfs, cnf):
    """Positions N(0, 1) centred per (object, sample) times pos_scale; features uniform in [0, 1)."""
    from oareactdiff_amd.graph_tools import get_edges_index, get_mask_for_frag, get_n_frag_switch
    g = torch.Generator().manual_seed(seed)
    sizes = [torch.tensor(n) for n in natm]
    B = len(natm[0])
    masks = [get_mask_for_frag(s) for s in sizes]
    cm, nfs = torch.cat(masks), get_n_frag_switch(sizes)
    ei = get_edges_index(cm, remove_self_edge=True)
    xh = []
    for m, s, nf in zip(masks, sizes, node_nfs):
        pos = torch.randn(m.numel(), 3, generator=g)
        mean = torch.zeros(B, 3).index_add_(0, m, pos) / s.clamp(min=1).float().unsqueeze(1)
        xh.append(torch.cat([(pos - mean[m]) * pos_scale, torch.rand(m.numel(), nf - 3, generator=g)], 1))
    return xh, ei, torch.rand(B, 1, generator=g), torch.rand(B, max(cnf, 1), generator=g), nfs, cm


def _nea(natm):
    """(N, E, A) of the complete graph per sample, from the layout alone."""
    per = [[natm[k][b] for k in range(len(natm))] for b in range(len(natm[0]))]
    return (sum(sum(p) for p in per), sum(sum(p) * (sum(p) - 1) for p in per), sum(n * (n - 1) for p in per for n in p))


def _state(cfg, node_nfs, cnf, alias=None, condition_time=True, seed=7):
    from oareactdiff_amd.spec import state_spec, synthetic_state_dict
    sd = synthetic_state_dict(state_spec(cfg, node_nfs, cnf, condition_time=condition_time), cfg, seed=seed)
    for k in alias or []:                                            # the aliased slots hold object 0's tensors (_base.py:110-113)
        for name in list(sd):
            if name.startswith((f"encoders.{k}.", f"decoders.{k}.")):
                sd[name] = sd[name.replace(f".{k}.", ".0.", 1)].clone()
    return sd


def _module(cfg, node_nfs, cnf, sd, dev, alias=None, condition_time=True):
    from oareactdiff_amd.dynamics import EGNNDynamics
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=[f"o{k}" for k in range(len(node_nfs))], node_nfs=list(node_nfs), edge_nf=0,
                       condition_nf=cnf, condition_time=condition_time, enforce_same_encoding=alias, device=dev)
    dyn.load_state_dict(sd, strict=True)
    return dyn


def _split(outs):
    outs = [torch.as_tensor(o).detach().cpu().double() for o in outs]
    return torch.cat([o[:, :3].reshape(-1) for o in outs]), torch.cat([o[:, 3:].reshape(-1) for o in outs])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, state dict, float64 oracle outputs split into velocities and features) of a layout: once per process, never written to."""
    natm, pos_scale, alias = LAYOUTS[name]
    node_nfs = [9] * len(natm)
    cfg = _cfg()
    batch = _batch(natm, pos_scale, 11, node_nfs, 1)
    sd = _state(cfg, node_nfs, 1, alias)
    xh, ei, t, cond, nfs, cm = batch
    enc = None if alias is None else [0 if k in alias else k for k in range(len(natm))]
    ref = oracle.dynamics_forward({k: v.double() for k, v in sd.items()}, cfg, [x.double() for x in xh], ei, t.double(), cond.double(), nfs,
                                  cm, 1, encoder_alias=enc, nodeframe="exact")
    return batch, sd, _split(ref)


def _run(dyn, batch, dev):
    xh, ei, t, cond, nfs, cm = batch
    with torch.no_grad():
        out, _ = dyn([x.to(dev) for x in xh], ei.to(dev), t.to(dev), cond.to(dev), nfs.to(dev), cm.to(dev))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shapes", ["throughput", "auto"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_forward_matches_the_oracle_f64(name, shapes):
    dev = torch.device("cuda:0")
    natm, pos_scale, alias = LAYOUTS[name]
    batch, sd, (rv, rh) = _case(name)
    dyn = _module(_cfg(), [9] * len(natm), 1, sd, dev, alias)
    with debug_options(**(LIB_AUTO if shapes == "auto" else {})):
        out = _run(dyn, batch, dev)
    topo = dyn._last_topo
    assert topo.handle is not None and topo.graph is None                 # the production kernels, not the general path
    N, E, A = _nea(natm)
    assert (topo.n_nodes, topo.n_edges, topo.n_inner) == (N, E, A)
    if len(natm) == 1:
        assert E == A
    if name == "one_tile":
        assert E == A == 128
    if name == "one_tile_plus_two":
        assert E == A == 130
    if name.endswith("_cut"):                                             # the cutoff bites, and not everywhere
        n_act = dyn.active_inner_edges()
        assert 0 < n_act < A, (n_act, A)
    assert all(o.shape == x.shape for o, x in zip(out, batch[0])) and all(bool(torch.isfinite(o).all()) for o in out)
    v, h = _split(out)
    print(f"{name} ({shapes}): N / E / A {N} / {E} / {A}  vel {rel(v, rv):.2e}  h {rel(h, rh):.2e}  (gate {TOL:.0e})")
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (rel(v, rv), rel(h, rh))


def test_neither_time_nor_conditions():
    """condition_time = False with condition_nf = 0: all in_hidden_channels columns are the embedding.  The reference cannot run this
    (egnn_dynamics.py:145 slices h_final[:, :-0]); the oracle keeps every column there, as the library does."""
    dev = torch.device("cuda:0")
    natm, node_nfs = [[4, 2, 9], [3, 5, 1], [2, 3, 6]], [9, 7, 9]
    cfg = _cfg()
    batch = _batch(natm, 1.0, 13, node_nfs, 0)
    sd = _state(cfg, node_nfs, 0, condition_time=False)
    xh, ei, t, cond, nfs, cm = batch
    rv, rh = _split(oracle.dynamics_forward({k: v.double() for k, v in sd.items()}, cfg, [x.double() for x in xh], ei, t.double(),
                                            cond.double(), nfs, cm, 0, condition_time=False, nodeframe="exact"))
    dyn = _module(cfg, node_nfs, 0, sd, dev, condition_time=False)
    assert dyn.embed_dim == cfg["in_hidden_channels"]
    for shapes in ("throughput", "auto"):
        with debug_options(**(LIB_AUTO if shapes == "auto" else {})):
            v, h = _split(_run(dyn, batch, dev))
        print(f"no time, no conditions ({shapes}): vel {rel(v, rv):.2e}  h {rel(h, rh):.2e}  (gate {TOL:.0e})")
        assert rel(v, rv) <= TOL and rel(h, rh) <= TOL


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persist", [0, 2])
@pytest.mark.parametrize("name", ["one_ragged_cut", "eight_cut"])
def test_sub_batches_are_bitwise_identical(name, persist):
    """parts = 1, 2 and 3 (the library caps the number at the batch size) with the same GCL edge kernel on every side, as
    test_hip_parity.test_concurrent_sub_batches_are_bitwise_identical arranges: reactions never interact.  Launch shapes pinned to the
    throughput kernels: the library's own heuristics choose shapes by the load of a sub-batch (other summation orders, tests/_cases.py),
    so under them every split is held to the oracle's gate instead."""
    dev = torch.device("cuda:0")
    natm, _, alias = LAYOUTS[name]
    batch, sd, (rv, rh) = _case(name)
    outs = []
    for parts in (1, 2, 3):
        with debug_options(parts=parts, gcl_persist=persist, **THROUGHPUT):
            outs.append([o.clone() for o in _run(_module(_cfg(), [9] * len(natm), 1, sd, dev, alias), batch, dev)])
        with debug_options(parts=parts, gcl_persist=persist, **LIB_AUTO):
            v, h = _split(_run(_module(_cfg(), [9] * len(natm), 1, sd, dev, alias), batch, dev))
        assert rel(v, rv) <= TOL and rel(h, rh) <= TOL, (parts, rel(v, rv), rel(h, rh))
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    v, h = _split(outs[0])
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL


@pytest.mark.parametrize("name", ["one_tile", "one_ragged_cut", "eight_cut"])
def test_results_do_not_depend_on_the_workspace(name):
    """Workspace poison (0xFF fill before every forward) on and off: the same bits, all finite - with zero inter-object rows no kernel
    may read a row that nothing wrote."""
    dev = torch.device("cuda:0")
    natm, _, alias = LAYOUTS[name]
    batch, sd, _ = _case(name)
    outs = []
    for poison in (1, 0):
        with debug_options(poison=poison):
            dyn = _module(_cfg(), [9] * len(natm), 1, sd, dev, alias)
            if not poison:                                              # huge finite garbage instead of NaN patterns
                _run(dyn, batch, dev)
                dyn._call_buffers.ws.view(torch.int32).fill_(0x7F000000)
            outs.append([o.clone() for o in _run(dyn, batch, dev)])
    assert all(bool(torch.isfinite(a).all()) for a in outs[0])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("layout", ["one_object", "eight_objects"])
def test_nan_replace_against_its_formula(layout):
    """oard_nan_replace with one and with eight objects: the gate and the float64 formula of tests/test_sampler_step.py."""
    from test_sampler_step import check_nan_replace
    check_nan_replace(layout)


# ---- one step beyond each limit of the production kernels ---------------------------------------------------------------------------
def _h32(**over):
    return dict(dict(pos_require_grad=False, cutoff=5.0, num_layers=2, hidden_channels=32, num_radial=8, in_hidden_channels=8), **over)


@pytest.mark.parametrize("which", ["node_nf_20", "in_hidden_17"])
def test_one_past_a_width_limit_runs_the_general_path(which):
    """node_nf = 20 (17 feature columns) and in_hidden_channels = 17 are outside the production kernels' tables: the call warns, runs the
    general-edge-list kernels and matches the float64 oracle (literal node frame) at that path's gate."""
    dev = torch.device("cuda:0")
    if which == "node_nf_20":
        cfg, node_nfs, cnf = _h32(), [9, 20, 5], 1
    else:
        cfg, node_nfs, cnf = _h32(in_hidden_channels=17), [9, 19, 5], 5
    natm = [[3, 5, 2], [4, 0, 6], [2, 7, 1]]
    batch = _batch(natm, 1.5, 17, node_nfs, cnf)
    sd = _state(cfg, node_nfs, cnf)
    xh, ei, t, cond, nfs, cm = batch
    dyn = _module(cfg, node_nfs, cnf, sd, dev)
    with pytest.warns(UserWarning):
        out = _run(dyn, batch, dev)
    assert dyn._last_topo.graph is not None and dyn._last_topo.handle is None
    rv, rh = _split(oracle.dynamics_forward({k: v.double() for k, v in sd.items()}, cfg, [x.double() for x in xh], ei, t.double(),
                                            cond.double(), nfs, cm, cnf, nodeframe="literal"))
    v, h = _split(out)
    print(f"{which}: general path vel {rel(v, rv):.2e}  h {rel(h, rh):.2e}  (gate {TOL:.0e})")
    assert all(bool(torch.isfinite(o).all()) for o in out)
    assert rel(v, rv) <= TOL and rel(h, rh) <= TOL


def test_nine_objects_are_refused():
    """One object more than OARD_MAX_OBJECTS: the module refuses the call before anything is launched (the outputs it was handed stay
    untouched), and so does the C ABI for a hand-made configuration."""
    from oareactdiff_amd import _capi
    from oareactdiff_amd.dynamics import EGNNDynamics
    dev = torch.device("cuda:0")
    cfg, node_nfs = _h32(), [9] * 9
    batch = _batch([[2, 1]] * 9, 1.0, 19, node_nfs, 1)
    dyn = EGNNDynamics(model_config=dict(cfg), fragment_names=[f"o{k}" for k in range(9)], node_nfs=node_nfs, edge_nf=0, condition_nf=1,
                       device=dev)
    with pytest.raises(_capi.OardError):
        _run(dyn, batch, dev)
    assert dyn._last_topo is None and dyn._ws is None                      # no topology was built, no workspace was asked for
    eight = EGNNDynamics(model_config=dict(cfg), fragment_names=[f"o{k}" for k in range(8)], node_nfs=[9] * 8, edge_nf=0, condition_nf=1,
                         device=dev)
    c = eight._config()
    L = _capi.lib()
    assert L.oard_supported(C.byref(c)) == _capi.OARD_OK
    c.n_obj = 9
    assert L.oard_supported(C.byref(c)) != _capi.OARD_OK
    cm, nfs = batch[5].contiguous(), batch[4].contiguous()
    h = C.c_void_p()
    rc = L.oard_topology_create(C.byref(c), C.cast(cm.data_ptr(), C.POINTER(C.c_int64)), C.cast(nfs.data_ptr(), C.POINTER(C.c_int64)),
                                cm.numel(), C.byref(h))
    assert rc != _capi.OARD_OK and not h.value
