"""`oard_dataset_gather` at the C boundary without a device: exported, declared, versioned, and its argument checks return before any HIP
call (the pattern of tests/test_rank_capi_cpu.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    return _capi, _capi.lib()


def test_exported_declared_and_versioned():
    _capi, L = _lib()
    assert hasattr(L, "oard_dataset_gather") and "oard_dataset_gather" in _capi.EXPORTS
    assert L.oard_version() == _capi.ABI_VERSION >= 2048
    header = open(os.path.join(ROOT, "include", "oard.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+oard_dataset_gather\s*\(", code)
    assert re.search(r"#define\s+OARD_STORE_OBJECTS\s+3\b", header) and _capi.OARD_STORE_OBJECTS == 3
    # the ctypes mirror has the header's fields in the header's order
    body = re.search(r"typedef struct oard_reaction_store \{(.*?)\} oard_reaction_store;", code, flags=re.S).group(1)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip().replace("\n", " "))]
    assert names == [f[0] for f in _capi.OardReactionStore._fields_]
    source = open(os.path.join(ROOT, "oareactdiff_amd", "csrc", "oard_hip.hip")).read()
    assert re.search(r"#define\s+OARD_VERSION\s+2048\b", source)


class _Args:
    """A valid call on HOST memory: every pointer is an address inside `buf`, which no accepted or refused call may touch."""

    def __init__(self, _capi, n_obj=3):
        self.buf = (C.c_int64 * 64)()
        p = C.addressof(self.buf)
        s = _capi.OardReactionStore()
        for k in range(3):
            s.offsets[k], s.pos[k], s.z[k] = p, p, p
            s.src_obj[k] = k
            s.reflect_obj[k] = 1
        s.sel, s.n_raw, s.n_sel, s.n_obj, s.center = p, 4, 3, n_obj, 1
        if n_obj == 1:
            s.src_obj[0] = 1
        self.store, self.p = s, p
        self.arr = (C.c_void_p * 3)(p, p, p)
        self.index, self.off, self.first, self.B = p, self.arr, 0, 2
        self.out = [self.arr] * 5
        self.condition, self.target, self.rmsd, self.ediff = p, None, None, None

    def call(self, L):
        return L.oard_dataset_gather(C.byref(self.store) if self.store is not None else None, self.index, self.off, self.first, self.B,
                                     *self.out, self.condition, self.target, self.rmsd, self.ediff, None)


def test_invalid_arguments_return_without_a_device():
    _capi, L = _lib()
    null3 = (C.c_void_p * 3)(None, None, None)

    def case(**kw):
        a = _Args(_capi)
        for key, val in kw.items():
            if key.startswith("s_"):
                setattr(a.store, key[2:], val)
            else:
                setattr(a, key, val)
        return a

    bad = {
        "null store": case(store=None), "null index": case(index=None), "null epoch_off": case(off=None),
        "null epoch_off entry": case(off=null3), "null condition": case(condition=None),
        "negative first": case(first=-1), "negative B": case(B=-1), "B beyond int32": case(B=1 << 31),
        "first + B beyond int32": case(first=(1 << 31) - 2), "n_obj 2": case(s_n_obj=2), "n_obj 0": case(s_n_obj=0),
        "n_raw 0": case(s_n_raw=0), "n_sel 0": case(s_n_sel=0), "n_sel > n_raw": case(s_n_sel=5),
        "B beyond int64 arithmetic": case(B=(1 << 63) - 1), "first beyond int32": case(first=1 << 40), "null sel": case(s_sel=None),
        "flag 2": case(s_swap=2), "flag -1": case(s_center=-1), "append 3": case(s_append_frag=3),
        "target output without a column": case(target=C.addressof(_Args(_capi).buf)),
        "ediff output without a column": case(ediff=C.addressof(_Args(_capi).buf)),
    }
    a = case(); a.store.target = a.p; bad["target column without an output"] = a
    a = case(); a.store.rmsd = a.p; bad["rmsd column without an output"] = a
    a = case(); a.store.ediff[0] = a.p; a.ediff = a.p; bad["half an ediff column"] = a
    a = case(); a.store.src_obj[1] = 3; bad["src_obj 3"] = a
    a = case(); a.store.src_obj[2] = -1; bad["src_obj -1"] = a
    a = case(); a.store.reflect_obj[0] = 2; bad["reflect_obj 2"] = a
    a = case(); a.store.pos[1] = None; bad["null positions of a used source"] = a
    a = case(); a.store.swap = 1; a.store.src_obj[0] = a.store.src_obj[1] = a.store.src_obj[2] = 0; a.store.z[2] = None
    bad["null swap partner"] = a
    for i, name in enumerate(("size", "pos", "one_hot", "charge", "mask")):
        a = case(); a.out = list(a.out); a.out[i] = None; bad[f"null {name} array"] = a
        a = case(); a.out = list(a.out); a.out[i] = null3; bad[f"null {name} entry"] = a
    for what, a in bad.items():
        assert a.call(L) == _capi.OARD_EINVAL, what
        assert all(v == 0 for v in a.buf), what
    # B == 0 is refused too when an argument is wrong: the checks come first
    assert case(B=0, index=None).call(L) == _capi.OARD_EINVAL


def test_empty_batch_is_success_without_a_launch():
    _capi, L = _lib()
    for n_obj in (3, 1):
        a = _Args(_capi, n_obj)
        a.B = 0
        assert a.call(L) == _capi.OARD_OK
        a.first = 5
        assert a.call(L) == _capi.OARD_OK
        assert all(v == 0 for v in a.buf)
    a = _Args(_capi)                                       # every column present
    a.B = 0
    a.store.target = a.store.rmsd = a.p
    a.store.ediff[0] = a.store.ediff[1] = a.p
    a.target = a.rmsd = a.ediff = a.p
    assert a.call(L) == _capi.OARD_OK and all(v == 0 for v in a.buf)
