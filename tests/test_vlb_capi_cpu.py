"""`oard_loss_eval_prepare` / `oard_loss_eval_terms` at the C boundary without a device: exported, declared, versioned, and every
argument check returns OARD_EINVAL before any HIP call."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oard_loss_eval_prepare", "oard_loss_eval_terms")


def _lib():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    return _capi, _capi.lib()


def test_exported_declared_and_versioned():
    _capi, L = _lib()
    header = open(os.path.join(ROOT, "include", "oard.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert hasattr(L, name) and name in _capi.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes
    assert L.oard_version() == _capi.ABI_VERSION >= 2047
    src = open(os.path.join(ROOT, "oareactdiff_amd", "csrc", "oard_hip.hip")).read()
    assert re.search(r"#define OARD_VERSION %d\b" % _capi.ABI_VERSION, src)
    # every entry cites the reference lines it replaces
    block = header[header.index("The evaluation half of the loss"): header.index("int oard_loss_eval_prepare(")]
    assert "en_diffusion.py:56-248" in block and "pl_trainer.py:246-282" in block
    # the kernels' header is part of exactly one translation unit
    csrc = os.path.join(ROOT, "oareactdiff_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip")) and '#include "oard_loss_eval.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["oard_hip.hip"]


def _config(_capi, n_obj=3, node_nf=9):
    """A configuration the library is built for (the production widths), made without the module."""
    c = _capi.OardConfig()
    c.hidden, c.num_radial, c.num_layers, c.in_hidden, c.n_obj, c.pos_dim, c.reflect_equiv = 196, 96, 9, 8, n_obj, 3, 1
    c.condition_nf, c.condition_time, c.cutoff = 1, 1, 10.0
    for k in range(min(n_obj, _capi.OARD_MAX_OBJECTS)):
        c.node_nf[k] = node_nf
    return c


def test_invalid_arguments_return_without_a_device():
    """Host memory stands in for every table and pointer list: a valid address that no refused call may touch.  The topology is a zeroed
    block larger than the library's struct (n_parts = 0: not a one-sub-batch topology), so even the call with every other argument
    in order is refused - after the checks under test, and still before any HIP call."""
    _capi, L = _lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ptrs = (C.c_void_p * _capi.OARD_MAX_OBJECTS)(*[p] * _capi.OARD_MAX_OBJECTS)
    topo_block = (C.c_char * (1 << 16))()
    topo = C.addressof(topo_block)
    f3 = (C.c_float * 3)(1.0, 4.0, 10.0)
    z3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    ok_cfg = _config(_capi)
    assert L.oard_supported(C.byref(ok_cfg)) == _capi.OARD_OK
    T = 1000

    def prep(cfg=ok_cfg, topo=topo, lists=None, t_int=p, gamma=p, T=T):
        a = [ptrs] * 9 if lists is None else lists
        return L.oard_loss_eval_prepare(C.byref(cfg) if cfg is not None else None, topo, a[0], a[1], a[2], a[3], a[4], t_int, gamma, T, f3, z3,
                                        0, 0, a[5], a[6], a[7], a[8], None)

    def terms(cfg=ok_cfg, topo=topo, lists=None, t_int=p, gamma=p, snr=p, T=T, B=2, nll=p, out=p):
        a = [ptrs] * 7 if lists is None else lists
        return L.oard_loss_eval_terms(C.byref(cfg) if cfg is not None else None, topo, a[0], a[1], a[2], a[3], a[4], a[5], a[6], t_int, gamma,
                                      snr, T, f3, z3, f3, 0, 0.0, B, nll, out, None)

    def without(n, i):
        return [None if j == i else ptrs for j in range(n)]

    bad = {"prepare: no config": prep(cfg=None), "prepare: no topology": prep(topo=None), "prepare: null t_int": prep(t_int=None),
           "prepare: null gamma table": prep(gamma=None), "prepare: T = 0": prep(T=0), "prepare: T < 0": prep(T=-5),
           "prepare: too many objects": prep(cfg=_config(_capi, n_obj=_capi.OARD_MAX_OBJECTS + 1)),
           "prepare: no object": prep(cfg=_config(_capi, n_obj=0)),
           "prepare: node_nf - 4 > 16": prep(cfg=_config(_capi, node_nf=21)), "prepare: node_nf < 5": prep(cfg=_config(_capi, node_nf=4)),
           "terms: no config": terms(cfg=None), "terms: no topology": terms(topo=None), "terms: null t_int": terms(t_int=None),
           "terms: null gamma table": terms(gamma=None), "terms: null SNR table": terms(snr=None), "terms: T = 0": terms(T=0),
           "terms: B = 0": terms(B=0), "terms: B < 0": terms(B=-1), "terms: no nll": terms(nll=None), "terms: no terms": terms(out=None),
           "terms: too many objects": terms(cfg=_config(_capi, n_obj=_capi.OARD_MAX_OBJECTS + 1)),
           "terms: node_nf - 4 > 16": terms(cfg=_config(_capi, node_nf=21)), "terms: node_nf < 5": terms(cfg=_config(_capi, node_nf=4)),
           "prepare: not a one-sub-batch topology": prep(), "terms: not a one-sub-batch topology": terms()}
    for i in range(9):
        bad[f"prepare: null pointer list {i}"] = prep(lists=without(9, i))
    for i in range(7):
        bad[f"terms: null pointer list {i}"] = terms(lists=without(7, i))
    for what, rc in bad.items():
        assert rc == _capi.OARD_EINVAL, what
    assert all(v == 0.0 for v in buf) and not any(topo_block.raw)
