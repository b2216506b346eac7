"""k_matched_rmsd through the C ABI alone (`oard_matched_rmsd`, include/oard.h): one launch of mixed segments (tests/_match_cases.py) -
the exact branch against `brute` (every permutation, SVD fit), the search branch against `search` (scipy's assignment, SVD fit, the same
starts), both with the gate of tests/_kabsch_cases.py, |k - r| <= 2^-23 r + 1e-10 rho; and on every segment, the degenerate kinds
included, the properties that need no yardstick: `perm` is a species-preserving permutation of the segment's rows, `oard_kabsch_rmsd` of
a against b[perm] (in the chirality that `rot` reports) reproduces the number, the number is not above the same-order one, the status is
as tabulated, and a segment's bits do not depend on the rest of the launch.

Measured on an MI355X (worst over the four generic kinds, all segments and both flags): |k - r| = 0.346 of the gate."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _kabsch_cases as kc
import _match_cases as mc

pytestmark = pytest.mark.gpu
GUARD = 8
SENTINEL = -7


def _dev():
    return torch.device("cuda:0")


def _lib():
    from oareactdiff_amd import _capi
    return _capi, _capi.lib()


@functools.lru_cache(maxsize=None)
def _case(kind):
    return mc.make_kind(kind)


@functools.lru_cache(maxsize=None)
def _reference(kind, flags):
    """Per segment (r, rho, same-order r); r is None where there is no yardstick (special segments, degenerate kinds)."""
    case = _case(kind)
    out = []
    for g, name in enumerate(mc.NAMES):
        if name in mc.NO_REFERENCE:
            out.append((None, None, None))
            continue
        a, b, sp, _ = mc.segment(case, g)
        r = None
        if kind in mc.KINDS:
            r = mc.brute(a, b, sp, bool(flags))[0] if mc.STATUS[name] == 0 else mc.search(a, b, sp, bool(flags))[0]
        out.append((r, mc.rho(a, b), mc.same_order(a, b, bool(flags))))
    return out


def _wide(x, ld, dev):
    w = torch.full((max(len(x), 1), ld), float("nan"), device=dev)
    w[:len(x), :3] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return w


def _launch(a, b, sp_a, sp_b, sizes, flags=1, cap=0.0, exact_limit=10000, lda=3, ldb=3, outputs=True):
    """a, b float32 [n, 3] and species int32 [n] as numpy (sp_b None: NULL).  The outputs carry GUARD rows behind them that must come back
    untouched.  -> dict of numpy arrays (rmsd [G], status [G], rot [G, 3, 3], aligned [n, 3], perm [n])."""
    _capi, L = _lib()
    dev = _dev()
    n, G = len(a), len(sizes)
    wa, wb = _wide(a, lda, dev), _wide(b, ldb, dev)
    da = torch.from_numpy(np.ascontiguousarray(sp_a, dtype=np.int32)).to(dev)
    db = None if sp_b is None else torch.from_numpy(np.ascontiguousarray(sp_b, dtype=np.int32)).to(dev)
    ptr = torch.from_numpy(kc.seg_ptr(sizes).astype(np.int32)).to(dev)
    nan = float("nan")
    o_r = torch.full((G + GUARD,), nan, device=dev)
    o_m = torch.full((G + GUARD, 9), nan, device=dev) if outputs else None
    o_a = torch.full((n + GUARD, 3), nan, device=dev) if outputs else None
    o_p = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev) if outputs else None
    o_s = torch.full((G + GUARD,), SENTINEL, dtype=torch.int32, device=dev) if outputs else None
    opt = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = L.oard_matched_rmsd(wa.data_ptr(), lda, wb.data_ptr(), ldb, da.data_ptr(), opt(db), ptr.data_ptr(), G, flags, cap, exact_limit,
                                 o_r.data_ptr(), opt(o_m), opt(o_a), opt(o_p), opt(o_s), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    for w, ld in ((wa, lda), (wb, ldb)):                         # inputs untouched, the padding columns still NaN
        assert ld == 3 or bool(torch.isnan(w[:, 3:]).all())
    assert bool(torch.isnan(o_r[G:]).all())
    res = {"rmsd": o_r[:G].cpu().numpy()}
    if outputs:
        assert bool(torch.isnan(o_m[G:]).all()) and bool(torch.isnan(o_a[n:]).all()), "a guard row behind an output was written"
        assert bool((o_p[n:] == SENTINEL).all()) and bool((o_s[G:] == SENTINEL).all()), "a guard row behind an output was written"
        res.update(rot=o_m[:G].cpu().numpy().reshape(G, 3, 3), aligned=o_a[:n].cpu().numpy(), perm=o_p[:n].cpu().numpy(),
                   status=o_s[:G].cpu().numpy())
    return res


@functools.lru_cache(maxsize=None)
def _mixed(kind, flags):
    c = _case(kind)
    return _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], flags)


def _kabsch(a, b, sizes, flags):
    _capi, L = _lib()
    dev = _dev()
    da, db = _wide(a, 3, dev), _wide(b, 3, dev)
    ptr = torch.from_numpy(kc.seg_ptr(sizes).astype(np.int32)).to(dev)
    out = torch.full((len(sizes),), float("nan"), device=dev)
    with torch.cuda.device(dev):
        rc = L.oard_kabsch_rmsd(da.data_ptr(), 3, db.data_ptr(), 3, ptr.data_ptr(), len(sizes), flags, 0.0, out.data_ptr(), None, None,
                                torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _capi.OARD_OK
    return out.cpu().numpy()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind", mc.KINDS)
def test_parity(kind, flags):
    k = _mixed(kind, flags)
    ref = _reference(kind, flags)
    worst = 0.0
    for g, name in enumerate(mc.NAMES):
        assert k["status"][g] == (0 if name == "empty" else mc.STATUS[name]), (name, k["status"][g])
        r, rho, _ = ref[g]
        if r is None:
            assert np.isnan(k["rmsd"][g]) and np.isnan(k["rot"][g]).all(), name
            continue
        err, lim = abs(float(k["rmsd"][g]) - r), kc.gate(r, rho)
        print(f"  {kind} flags={flags} {name}: kernel {float(k['rmsd'][g]):.9g} reference {r:.9g} |diff| {err:.2e} gate {lim:.2e}")
        assert err <= lim, (kind, flags, name, float(k["rmsd"][g]), r, err, lim)
        worst = max(worst, err / lim if lim > 0 else 0.0)          # n = 1: r = rho = 0, and so is the kernel's number
    print(f"{kind} flags={flags}: worst |k - r| / gate = {worst:.3f}")


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind", mc.KINDS + mc.DEGENERATE)
def test_properties(kind, flags):
    c = _case(kind)
    k = _mixed(kind, flags)
    ref = _reference(kind, flags)
    p = kc.seg_ptr(c["sizes"])
    perm = k["perm"].astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(perm)))
    matched = c["b"][perm].copy()                                # b in a's row order, in the chirality the kernel kept
    for g, name in enumerate(mc.NAMES):
        s = slice(int(p[g]), int(p[g + 1]))
        assert k["status"][g] == (0 if name == "empty" else mc.STATUS[name]), name
        assert ((perm[s] >= p[g]) & (perm[s] < p[g + 1])).all(), name
        if name in mc.NO_REFERENCE:
            assert (perm[s] == np.arange(p[g], p[g + 1])).all(), name       # special segments: rows map to themselves
            assert np.isnan(k["aligned"][s]).all(), name
            continue
        assert (c["sp_b"][perm[s]] == c["sp_a"][s]).all(), name
        R = k["rot"][g].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6, name
        if np.linalg.det(R) < 0:
            assert flags == 1, name
            matched[s, 2] = -matched[s, 2]
        # `aligned` is that map applied to the matched rows, and its distance from a is the number returned
        sa, sb = c["a"][s].astype(np.float64), c["b"][perm[s]].astype(np.float64)
        want = (sb - sb.mean(0)) @ R.T + sa.mean(0)
        assert np.abs(k["aligned"][s] - want).max() <= 2.0 ** -22 * (np.abs(sa).max() + np.abs(sb - sb.mean(0)).max()), name
        back = np.sqrt(np.sum((k["aligned"][s].astype(np.float64) - sa) ** 2) / len(sa))
        assert abs(back - float(k["rmsd"][g])) <= 1e-6 * (np.abs(sa).max() + np.abs(sb - sb.mean(0)).max()), name
    again = _kabsch(c["a"], matched, c["sizes"], 0)
    for g, name in enumerate(mc.NAMES):
        if name in mc.NO_REFERENCE:
            continue
        _, rho, same = ref[g]
        got = float(k["rmsd"][g])
        assert abs(got - float(again[g])) <= kc.gate(got, rho), (kind, flags, name, got, float(again[g]))
        assert got <= same + kc.gate(same, rho), (kind, flags, name, got, same)      # two roundings of one number where the order given wins


def test_exact_limit_moves_segments_to_the_search():
    c = _case("rigid_noise")
    ref = _reference("rigid_noise", 1)
    base = _mixed("rigid_noise", 1)
    off = _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1, exact_limit=0)
    at = _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1, exact_limit=5040)
    for g, name in enumerate(mc.NAMES):
        if name in mc.NO_REFERENCE:
            assert off["status"][g] == base["status"][g], name
            continue
        assert off["status"][g] == 1, name
        assert at["status"][g] == (1 if name == "c7" else mc.STATUS[name]), name      # 5040 permutations are not below 5040
        a, b, sp, _ = mc.segment(c, g)
        r, rho = mc.search(a, b, sp, True)[0], ref[g][1]
        assert abs(float(off["rmsd"][g]) - r) <= kc.gate(r, rho), (name, float(off["rmsd"][g]), r)
        if mc.STATUS[name] == 0:
            assert float(off["rmsd"][g]) >= ref[g][0] - kc.gate(ref[g][0], rho), name       # never below the exact minimum
        if name != "c7":
            assert at["rmsd"][g].view(np.uint32) == base["rmsd"][g].view(np.uint32), name
    g7 = mc.NAMES.index("c7")
    assert at["rmsd"][g7].view(np.uint32) == off["rmsd"][g7].view(np.uint32)


def test_repeatable_and_independent_of_the_launch():
    c = _case("independent")
    one = _mixed("independent", 1)
    two = _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1)
    for key in one:
        assert np.array_equal(one[key], two[key], equal_nan=True), key
    p = kc.seg_ptr(c["sizes"])
    for name in ("c7", "mol23", "n65"):
        g = mc.NAMES.index(name)
        s = slice(int(p[g]), int(p[g + 1]))
        # alone, and behind another segment (row offsets, another block of the grid)
        for lead in ([], ["c52"]):
            gs = [mc.NAMES.index(x) for x in lead] + [g]
            rows = np.concatenate([np.arange(p[h], p[h + 1]) for h in gs])
            alone = _launch(c["a"][rows], c["b"][rows], c["sp_a"][rows], c["sp_b"][rows], [c["sizes"][h] for h in gs], 1)
            t = slice(len(rows) - c["sizes"][g], len(rows))
            assert alone["rmsd"][-1].view(np.uint32) == one["rmsd"][g].view(np.uint32), (name, lead)
            assert alone["status"][-1] == one["status"][g]
            assert np.array_equal(alone["rot"][-1], one["rot"][g]) and np.array_equal(alone["aligned"][t], one["aligned"][s])
            assert np.array_equal(alone["perm"][t] - t.start, one["perm"][s] - s.start)


def test_strides_null_outputs_and_null_species_b():
    c = _case("rigid_noise")
    dense = _mixed("rigid_noise", 1)
    wide = _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1, lda=9, ldb=6)
    for key in dense:
        assert np.array_equal(dense[key], wide[key], equal_nan=True), key
    only = _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1, lda=9, ldb=6, outputs=False)
    assert np.array_equal(only["rmsd"], dense["rmsd"], equal_nan=True)
    same = _launch(c["a"], c["b"], c["sp_a"], None, c["sizes"], 1)         # NULL: b's species are a's - the mismatch is gone
    gm = mc.NAMES.index("mismatch")
    others = [g for g in range(len(mc.NAMES)) if g != gm]
    assert np.array_equal(same["rmsd"][others], dense["rmsd"][others], equal_nan=True)
    assert same["status"][gm] == 0 and np.isfinite(same["rmsd"][gm])
    assert np.array_equal(same["perm"][:kc.seg_ptr(c["sizes"])[gm]], dense["perm"][:kc.seg_ptr(c["sizes"])[gm]])


def test_rows_of_b_in_any_order_with_their_own_species():
    """b's rows shuffled across species, species_b shuffled with them: the exact branch returns the same minimum, through a valid perm."""
    c = _case("rigid_noise")
    ref = _reference("rigid_noise", 1)
    rng = np.random.default_rng(11)
    p = kc.seg_ptr(c["sizes"])
    b, sb = c["b"].copy(), c["sp_b"].copy()
    for g in range(len(mc.NAMES)):
        idx = np.arange(p[g], p[g + 1])
        sh = rng.permutation(idx)
        b[idx], sb[idx] = c["b"][sh], c["sp_b"][sh]
    k = _launch(c["a"], b, c["sp_a"], sb, c["sizes"], 1)
    perm = k["perm"].astype(np.int64)
    for g, name in enumerate(mc.NAMES):
        assert k["status"][g] == (0 if name == "empty" else mc.STATUS[name]), name
        if name in mc.NO_REFERENCE:
            continue
        s = slice(int(p[g]), int(p[g + 1]))
        assert sorted(perm[s].tolist()) == list(range(p[g], p[g + 1])) and (sb[perm[s]] == c["sp_a"][s]).all(), name
        r, rho, _ = ref[g]
        if mc.STATUS[name] == 0:
            assert abs(float(k["rmsd"][g]) - r) <= kc.gate(r, rho), (name, float(k["rmsd"][g]), r)
        else:                                                    # the first start differs with the order: a bound, not the same run
            planted = mc.planted_rmsd(*[mc.segment(c, g)[i] for i in (0, 1, 3)], True)
            assert float(k["rmsd"][g]) <= planted + kc.gate(planted, rho), (name, float(k["rmsd"][g]), planted)


def test_special_segments():
    c = _case("independent")
    p = kc.seg_ptr(c["sizes"])
    clean = {cap: _launch(c["a"], c["b"], c["sp_a"], c["sp_b"], c["sizes"], 1, cap=cap) for cap in (0.0, 0.5)}
    ge, gm, gl = (mc.NAMES.index(x) for x in ("empty", "mismatch", "n257"))
    live = [g for g, name in enumerate(mc.NAMES) if name not in mc.NO_REFERENCE]
    assert np.isnan(clean[0.0]["rmsd"][[ge, gm, gl]]).all()
    assert np.isnan(clean[0.5]["rmsd"][ge]) and (clean[0.5]["rmsd"][[gm, gl]] == np.float32(0.5)).all()
    assert np.array_equal(clean[0.5]["rmsd"][live], np.minimum(clean[0.0]["rmsd"][live], np.float32(0.5)))
    assert (clean[0.0]["rmsd"][live] > 0.5).any() and (clean[0.0]["rmsd"][live] < 0.5).any()      # the cap both bites and does not
    g_nan, g_inf = mc.NAMES.index("mol23"), mc.NAMES.index("c52")
    pa, pb = c["a"].copy(), c["b"].copy()
    pa[p[g_nan] + 5, 1] = np.nan
    pb[p[g_inf] + 6, 2] = np.inf
    for cap in (0.0, 0.5):
        k = _launch(pa, pb, c["sp_a"], c["sp_b"], c["sizes"], 1, cap=cap)
        for g in (g_nan, g_inf):
            s = slice(int(p[g]), int(p[g + 1]))
            assert k["status"][g] == 4
            assert (np.isnan(k["rmsd"][g]) if cap == 0.0 else k["rmsd"][g] == np.float32(cap)), (cap, g)
            assert np.isnan(k["rot"][g]).all() and np.isnan(k["aligned"][s]).all() and (k["perm"][s] == np.arange(p[g], p[g + 1])).all()
        others = [g for g in range(len(mc.NAMES)) if g not in (g_nan, g_inf)]
        assert np.array_equal(k["rmsd"][others].view(np.uint32), clean[cap]["rmsd"][others].view(np.uint32)), "a poisoned segment changed another"
        assert np.array_equal(k["status"][others], clean[cap]["status"][others])


def test_argument_checks():
    _capi, L = _lib()
    dev = _dev()
    a = torch.zeros(4, 3, device=dev)
    sp = torch.zeros(4, dtype=torch.int32, device=dev)
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    out = torch.full((4,), float("nan"), device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    A, S, P, O = a.data_ptr(), sp.data_ptr(), ptr.data_ptr(), out.data_ptr()
    f = C.c_float(0.0)
    tail = (None, None, None, None, st)
    with torch.cuda.device(dev):
        for args in ((None, 3, A, 3, S, None, P, 1), (A, 3, None, 3, S, None, P, 1), (A, 3, A, 3, None, None, P, 1),
                     (A, 3, A, 3, S, None, None, 1), (A, 3, A, 3, S, None, P, -1), (A, 2, A, 3, S, None, P, 1), (A, 3, A, 2, S, None, P, 1)):
            assert L.oard_matched_rmsd(*args, 0, f, 10000, O, *tail) == _capi.OARD_EINVAL, args
        for limit in (-1, 10001):
            assert L.oard_matched_rmsd(A, 3, A, 3, S, None, P, 1, 0, f, limit, O, *tail) == _capi.OARD_EINVAL
        assert L.oard_matched_rmsd(A, 3, A, 3, S, None, P, 1, 0, f, 10000, None, *tail) == _capi.OARD_EINVAL
        assert L.oard_matched_rmsd(A, 3, A, 3, S, None, P, 0, 0, f, 10000, O, *tail) == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    assert bool(torch.isnan(out).all()), "n_segments = 0 wrote something"
