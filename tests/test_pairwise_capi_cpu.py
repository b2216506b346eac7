"""`oard_pairwise_rmsd` and `oard_leader_cluster` at the C boundary without a device: exported, declared, listed, the version unchanged,
and their argument checks return before any HIP call.  A build-time check of the new kernels' scratch use rides along (no device
either): the pair kernels may use no more than the kernels whose bodies they share, the clustering kernel none."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oard_pairwise_rmsd", "oard_leader_cluster")


def _lib():
    from oareactdiff_amd import _capi
    from oareactdiff_amd.build import build
    build()
    return _capi, _capi.lib()


def test_exported_declared_and_listed():
    _capi, L = _lib()
    header = open(os.path.join(ROOT, "include", "oard.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name) and name in _capi.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", code)
    assert L.oard_version() == _capi.ABI_VERSION == 2048       # exports were added, no layout changed
    assert re.search(r"#define\s+OARD_LEADER_MAX\s+1024\b", header)
    from oareactdiff_amd import metrics
    assert metrics.LEADER_MAX == 1024 and metrics.PAIR_UNEQUAL == 5


def test_pairwise_invalid_arguments_return_without_a_device():
    _capi, L = _lib()
    f = L.oard_pairwise_rmsd
    buf = (C.c_double * 16)()                          # host memory: a valid address that no accepted call below may touch
    p = C.addressof(buf)
    #     x  ldx sp seg S  mem gp pp mp G  P  M  flags cap exact out status stream
    ok = (p, 3, p, p, 2, p, p, p, p, 1, 1, 2, 3, 0.0, 10000, p, p, None)
    bad = {
        "null x": (None,) + ok[1:],
        "ldx below 3": ok[:1] + (2,) + ok[2:],
        "matched mode without species": ok[:2] + (None,) + ok[3:],
        "null seg_ptr": ok[:3] + (None,) + ok[4:],
        "negative n_segments": ok[:4] + (-1,) + ok[5:],
        "null group_members": ok[:5] + (None,) + ok[6:],
        "null group_ptr": ok[:6] + (None,) + ok[7:],
        "null pair_ptr": ok[:7] + (None,) + ok[8:],
        "null mat_ptr": ok[:8] + (None,) + ok[9:],
        "negative n_groups": ok[:9] + (-1,) + ok[10:],
        "negative n_pairs": ok[:10] + (-1,) + ok[11:],
        "n_pairs beyond int32": ok[:10] + (1 << 31,) + ok[11:],
        "negative n_members": ok[:11] + (-1,) + ok[12:],
        "negative exact_limit": ok[:14] + (-1,) + ok[15:],
        "exact_limit above 10000": ok[:14] + (10001,) + ok[15:],
        "null out": ok[:15] + (None,) + ok[16:],
    }
    for what, args in bad.items():
        assert f(*args) == _capi.OARD_EINVAL, what
    # ... and with flags bit 1 alone (bit 0 clear)
    assert f(*(ok[:2] + (None,) + ok[3:12] + (2,) + ok[13:])) == _capi.OARD_EINVAL
    assert all(v == 0.0 for v in buf)


def test_leader_invalid_arguments_return_without_a_device():
    _capi, L = _lib()
    f = L.oard_leader_cluster
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    ok = (p, p, p, None, 1, 0.1, p, p, None)
    bad = {
        "null dist": (None,) + ok[1:],
        "null mat_ptr": ok[:1] + (None,) + ok[2:],
        "null group_ptr": ok[:2] + (None,) + ok[3:],
        "negative n_groups": ok[:4] + (-1,) + ok[5:],
        "negative threshold": ok[:5] + (-0.5,) + ok[6:],
        "NaN threshold": ok[:5] + (float("nan"),) + ok[6:],
        "infinite threshold": ok[:5] + (float("inf"),) + ok[6:],
        "null label": ok[:6] + (None,) + ok[7:],
        "null n_clusters": ok[:7] + (None,) + ok[8:],
    }
    for what, args in bad.items():
        assert f(*args) == _capi.OARD_EINVAL, what
    assert all(v == 0.0 for v in buf)


def test_no_groups_is_success_without_a_launch():
    _capi, L = _lib()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    assert L.oard_pairwise_rmsd(p, 3, None, p, 0, p, p, p, p, 0, 0, 0, 1, 0.0, 10000, p, None, None) == _capi.OARD_OK
    assert L.oard_pairwise_rmsd(p, 10, p, p, 4, p, p, p, p, 0, 0, 0, 3, 0.5, 0, p, p, None) == _capi.OARD_OK
    assert L.oard_leader_cluster(p, p, p, None, 0, 0.1, p, p, None) == _capi.OARD_OK
    assert L.oard_leader_cluster(p, p, p, p, 0, 0.0, p, p, None) == _capi.OARD_OK
    assert all(v == 0.0 for v in buf)


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_a_library_without_the_symbols_is_refused_by_name(tmp_path):
    """`_capi.lib()` on a library of the right version that predates the two exports: OardError naming the rebuild, not AttributeError."""
    import sys
    stub = os.path.join(tmp_path, "stub.cpp")
    with open(stub, "w") as f:
        f.write('extern "C" int oard_version() { return 2048; }\n')
    lib = os.path.join(tmp_path, "liboard_stub.so")
    subprocess.run([HIPCC, "-x", "c++", "-shared", "-fPIC", stub, "-o", lib], check=True, capture_output=True, timeout=300)
    prog = ("from oareactdiff_amd import _capi\n"
            "try:\n    _capi.lib()\nexcept _capi.OardError as e:\n    print('OardError:', e)\n")
    r = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, env=dict(os.environ, OARD_LIB=lib), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("OardError:") and all(name in r.stdout for name in NAMES) and "rebuild" in r.stdout, r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_use_no_more_scratch_than_the_bodies_they_share(tmp_path):
    from test_kernel_budgets import _compile_unit
    _, rc, err = _compile_unit(("oard_hip.hip", os.path.join(tmp_path, "oard_hip.o")))
    assert rc == 0, err[-2000:]
    blocks = err.split("Function Name: ")[1:]
    names = subprocess.run(["c++filt"], input="\n".join(b.split("\n")[0].split()[0] for b in blocks), capture_output=True,
                           text=True).stdout.splitlines()
    scratch = {}
    for dem, b in zip(names, blocks):
        m = re.match(r"^(k_\w+)\(", dem)
        if m:
            scratch[m.group(1)] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
    for new, old in (("k_pairwise_kabsch", "k_kabsch_rmsd"), ("k_pairwise_matched", "k_matched_rmsd")):
        print(new, scratch[new], old, scratch[old])
        assert scratch[new] <= scratch[old], (new, scratch[new], old, scratch[old])
    assert scratch["k_leader_cluster"] == 0 and scratch["k_pairwise_diag"] == 0
