"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/oard.h declares, the module reproduces the reference state-dict layout, and the product path
fails loudly (no CPU fallback) when asked to run without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

from _cases import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    return _capi, _capi.lib()


def test_library_exports_every_declared_symbol():
    _capi, L = _lib()
    header = open(os.path.join(ROOT, "include", "oard.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(oard_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(L, name), f"{name} declared in include/oard.h but not exported"
    assert set(_capi.EXPORTS) <= declared
    assert L.oard_version() >= 2000


def test_config_support_and_param_count():
    _capi, L = _lib()
    from oareactdiff_amd.dynamics import EGNNDynamics
    for name in ("g1_wrapper_small", "g2_prod_b2_n23", "g6_h32_r32"):
        c = Case(name)
        d = EGNNDynamics(model_config=dict(c.cfg), fragment_names=[f"o{k}" for k in range(c.n_obj)],
                         node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=torch.device("cpu"))
        cfg = d._config()
        assert L.oard_supported(C.byref(cfg)) == 0
        assert L.oard_param_count(C.byref(cfg)) == len(c.spec) == len(d._ordered_tensors())
        assert L.oard_packed_bytes(C.byref(cfg)) > 4 * sum(v.numel() for v in c.state_dict().values()) // 2
    bad = _capi.OardConfig()
    bad.hidden, bad.num_radial, bad.num_layers, bad.in_hidden, bad.n_obj, bad.pos_dim, bad.reflect_equiv = 100, 96, 6, 8, 3, 3, 1
    assert L.oard_supported(C.byref(bad)) != 0


def test_state_dict_layout_matches_reference_names():
    """Names/shapes are those of the reference's EGNNDynamics(model=LEFTNet).state_dict() (pinned when the
    goldens were generated: the reference loaded this spec's tensors with strict=True)."""
    from oareactdiff_amd.dynamics import EGNNDynamics
    c = Case("g2_prod_b2_n23")
    d = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=c.node_nfs, edge_nf=0,
                     condition_nf=c.cnf, device=torch.device("cpu"))
    sd = c.state_dict()
    assert list(d.state_dict().keys()) == list(sd.keys())
    assert all(d.state_dict()[k].shape == sd[k].shape for k in sd)
    d.load_state_dict(sd, strict=True)
    assert sum(p.numel() for p in d.parameters()) == 10645719
    assert d.pos_dim == 3 and d.node_nfs == c.node_nfs and d.embed_dim == 6 and d.edge_encoder is None
    # enforce_same_encoding aliases encoder/decoder 0 (reference _base.py:110-113)
    d2 = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=c.node_nfs, edge_nf=0,
                      condition_nf=c.cnf, device=torch.device("cpu"), enforce_same_encoding=[1, 2])
    assert d2.encoders[1] is d2.encoders[0] and d2.decoders[2] is d2.decoders[0]
    assert len(d2.state_dict()) == len(sd)
    # the constructor mutates model_config exactly like the reference (_base.py:47-51)
    cfg = dict(c.cfg)
    EGNNDynamics(model_config=cfg, fragment_names=["R", "TS", "P"], node_nfs=c.node_nfs, edge_nf=0,
                 condition_nf=c.cnf, device=torch.device("cpu"))
    assert cfg["act_fn"] == "swish" and cfg["in_node_nf"] == cfg["in_hidden_channels"]


def test_no_cpu_fallback_and_config_errors():
    from oareactdiff_amd._capi import OardError
    from oareactdiff_amd.dynamics import EGNNDynamics
    c = Case("g1_wrapper_small")
    d = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["a", "b", "c"], node_nfs=c.node_nfs, edge_nf=0,
                     condition_nf=c.cnf, device=torch.device("cpu"))
    d.load_state_dict(c.state_dict())
    with torch.no_grad(), pytest.raises(OardError):
        d(c.xh, c.edge_index, c.t, c.conditions, c.n_frag_switch, c.combined_mask)
    with pytest.raises(OardError):                              # the training path has no CPU fallback either
        d(c.xh, c.edge_index, c.t, c.conditions, c.n_frag_switch, c.combined_mask)
    with pytest.raises(NotImplementedError):                    # update_pocket_coords=False (egnn_dynamics.py:125)
        d2 = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["a", "b", "c"], node_nfs=c.node_nfs, edge_nf=0,
                          condition_nf=c.cnf, update_pocket_coords=False, device=torch.device("cpu"))
        with torch.no_grad():
            d2(c.xh, c.edge_index, c.t, c.conditions, c.n_frag_switch, c.combined_mask)
    with pytest.raises(AssertionError):                         # _base.py:44-46
        EGNNDynamics(model_config=dict(c.cfg), fragment_names=["a"], node_nfs=c.node_nfs, edge_nf=0,
                     device=torch.device("cpu"))
    with pytest.raises(NotImplementedError):                    # a LEFTNet switch outside the production setting
        EGNNDynamics(model_config=dict(c.cfg, legacy=False), fragment_names=["a", "b", "c"],
                     node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=torch.device("cpu"))
    # reflect_equiv: both settings are implemented since round 4 and travel to the library in oard_config
    for flag in (True, False):
        dd = EGNNDynamics(model_config=dict(c.cfg, reflect_equiv=flag), fragment_names=["a", "b", "c"],
                          node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=torch.device("cpu"))
        assert dd._config().reflect_equiv == int(flag)


def test_checkpoint_adapter_round_trip():
    """A Lightning-style checkpoint dict (prefix `ddpm.dynamics.`, hyper_parameters as pl_trainer.py:147 saves them)
    loads with strict=True; unrelated entries (EMA, optimiser state) are ignored."""
    from oareactdiff_amd.checkpoint import dynamics_from_checkpoint, extract_dynamics_state
    c = Case("g3_cutoff_ragged")
    sd = c.state_dict()
    ckpt = {
        "state_dict": {**{"ddpm.dynamics." + k: v for k, v in sd.items()},
                       "ddpm.schedule.gamma_module.gamma": torch.zeros(11), "some.other.module.weight": torch.ones(2)},
        "hyper_parameters": dict(model_config=dict(c.cfg), node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf,
                                 fragment_names=["R", "TS", "P"], pos_dim=3, update_pocket_coords=True,
                                 condition_time=True, edge_cutoff=None, enforce_same_encoding=None),
    }
    dyn, hp = dynamics_from_checkpoint(ckpt, device=torch.device("cpu"))
    got = dyn.state_dict()
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert set(extract_dynamics_state({"dynamics." + k: v for k, v in sd.items()})) == set(sd)
    with pytest.raises(KeyError):
        extract_dynamics_state({"foo.bar": torch.zeros(1)})


def test_call_buffers_grow_only_and_keep_the_sticky_flag():
    """`dynamics._CallBuffers`, the one owner of what a network call scribbles on, on the host (it only allocates and ORs): a buffer is
    reused while it is large enough and replaced when it is not, the tape is a view of exactly the requested bytes over ONE buffer
    with 1/8 headroom, the NaN flag accumulates with OR and is cleared in place."""
    from oareactdiff_amd.dynamics import EGNNDynamics, _CallBuffers
    cpu = torch.device("cpu")
    b = _CallBuffers()
    assert b.ws is None and b.tape_buf is None and b.scratch_buf is None and b.nan_seen is None
    b.reset()                                                   # nothing to clear yet
    w = b.workspace(100, cpu)
    assert w.dtype == torch.uint8 and w.numel() >= 100
    assert b.workspace(50, cpu) is w and b.ws is w
    w2 = b.workspace(200, cpu)
    assert w2 is not w and w2.numel() >= 200 and b.ws is w2
    s = b.scratch(64, cpu)
    assert b.scratch(64, cpu) is s and b.scratch(65, cpu) is not s and b.scratch_buf.numel() >= 65
    n = 1000
    t = b.tape(n, cpu)
    assert t.numel() == n and b.tape_buf.numel() >= n + n // 8 and t.data_ptr() == b.tape_buf.data_ptr()
    buf = b.tape_buf
    t2 = b.tape(400, cpu)
    assert b.tape_buf is buf and t2.numel() == 400 and t2.data_ptr() == buf.data_ptr()
    assert b.tape(n + n // 8 + 1, cpu).numel() == n + n // 8 + 1 and b.tape_buf is not buf
    b.note(torch.tensor([1, 0], dtype=torch.int32))
    flag = b.nan_seen
    b.note(torch.tensor([0, 4], dtype=torch.int32))
    b.note(torch.tensor([2, 0], dtype=torch.int32))
    assert b.nan_seen is flag and flag.tolist() == [3, 4]
    ptr = flag.data_ptr()
    b.reset()
    assert b.nan_seen is flag and flag.data_ptr() == ptr and flag.tolist() == [0, 0]
    # the module's `_ws` / `nan_seen` are views onto its own set, readable and writable
    c = Case("g1_wrapper_small")
    d = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["a", "b", "c"], node_nfs=c.node_nfs, edge_nf=0, condition_nf=c.cnf, device=cpu)
    assert d._ws is None and d.nan_seen is None
    d.reset_nan_seen()
    d.nan_seen = torch.tensor([5, 0], dtype=torch.int32)
    d._ws = w2
    assert d._call_buffers.nan_seen is d.nan_seen and d._call_buffers.ws is w2 and d._ws is w2
    d.reset_nan_seen()
    assert d.nan_seen.tolist() == [0, 0]


def test_ptr_array_maps_none_to_null():
    from oareactdiff_amd import _capi
    assert _capi.ptr_array(None) is None
    a, b = torch.zeros(3), torch.zeros(2, 2)
    arr = _capi.ptr_array([a, None, b])
    assert isinstance(arr, C.Array) and arr._type_ is C.c_void_p and len(arr) == 3
    assert arr[0] == a.data_ptr() and arr[1] is None and arr[2] == b.data_ptr()
    padded = _capi.ptr_array([a], 4)
    assert len(padded) == 4 and padded[0] == a.data_ptr() and padded[1] is None and padded[3] is None
    assert len(_capi.ptr_array([], 2)) == 2 and len(_capi.ptr_array([])) == 0
