"""`oard_rank_metrics` at the C boundary without a device: exported, declared, versioned, and its argument checks return before any HIP
call."""
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
    assert hasattr(L, "oard_rank_metrics") and "oard_rank_metrics" in _capi.EXPORTS
    assert L.oard_version() == _capi.ABI_VERSION >= 2046
    header = open(os.path.join(ROOT, "include", "oard.h")).read()
    assert re.search(r"#define\s+OARD_RANK_COLS\s+8\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+oard_rank_metrics\s*\(", code)
    from oareactdiff_amd import metrics
    assert metrics.RANK_COLS == 8 and len(metrics.RankMetrics._fields) == 8


def test_invalid_arguments_return_without_a_device():
    _capi, L = _lib()
    f = L.oard_rank_metrics
    buf = (C.c_double * 16)()                          # host memory: a valid address that no accepted call below may touch
    p = C.addressof(buf)
    ok = (p, p, 4, p, 1, p, p, p, None)
    bad = {
        "null score": (None,) + ok[1:],
        "null target": ok[:1] + (None,) + ok[2:],
        "null seg_ptr": ok[:3] + (None,) + ok[4:],
        "negative n": ok[:2] + (-1,) + ok[3:],
        "n beyond int32": ok[:2] + (1 << 31,) + ok[3:],
        "negative n_segments": ok[:4] + (-1,) + ok[5:],
        "no output": ok[:5] + (None, None, None, None),
        "no output, no segments": (None, None, 0, None, 0, None, None, None, None),
    }
    for what, args in bad.items():
        assert f(*args) == _capi.OARD_EINVAL, what
    assert all(v == 0.0 for v in buf)


def test_no_segments_is_success_without_a_launch():
    _capi, L = _lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert L.oard_rank_metrics(None, None, 0, None, 0, None, None, p, None) == _capi.OARD_OK
    assert L.oard_rank_metrics(p, p, 5, p, 0, p, p, p, None) == _capi.OARD_OK
    assert all(v == 0.0 for v in buf)
