"""k_pairwise_kabsch / k_pairwise_matched / k_pairwise_diag through the C ABI alone (`oard_pairwise_rmsd`, include/oard.h).  One launch
holds groups of K = 0, 1, 2, 3, 5, 8 members of n = 1, 2, 3, 7, 23, 65 rows, two of the groups interleaved in storage, the species of
every member in its own row order.  The main oracle needs no tolerance: entry [i, j] has the 32 bits `oard_kabsch_rmsd` /
`oard_matched_rmsd` give for explicit copies of member i as a and member j as b, status included.  On top: the matrix form, the float64
references of tests/_kabsch_cases.py and tests/_match_cases.py under the project's gate |k - r| <= 2^-23 r + 1e-10 rho, the special
members, independence of the rest of the launch, the canaries, and member indices outside [0, S).

Measured on an MI355X (worst over all pairs, both modes and both flags): |k - r| = 0.401 of the gate."""
import functools
import math

import numpy as np
import pytest
import torch

import _kabsch_cases as kc
import _match_cases as mc
import _pairwise_cases as pc

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = -7
UNWRITTEN = -3.0
LABELS = (6, 1, 7, 8)
#        name    K  species counts
SPEC = [("k0", 0, (1,)), ("k1", 1, (1,)), ("k2", 2, (2,)), ("k3", 3, (2, 1)), ("k5", 5, (3, 2, 1, 1)), ("k8", 8, (7, 12, 2, 2)),
        ("k3n65", 3, (65,)), ("k5b", 5, (1, 1))]
INTERLEAVED = ("k5", "k5b")                                   # stored member by member in turn, candidate-major


def _dev():
    return torch.device("cuda:0")


def _lib():
    from oareactdiff_amd import _capi
    return _capi, _capi.lib()


@functools.lru_cache(maxsize=None)
def _mix(special=False):
    """-> dict(members: list over segments of (pos [n, 3] float32, species [n] int32), groups: list over groups of segment indices).
    `special`: four members are spoilt (one coordinate inf, one row fewer, one species label changed, 257 rows)."""
    rng = np.random.default_rng(11)
    made = {}
    for name, K, counts in SPEC:
        n = int(sum(counts))
        sp0 = np.repeat(np.array(LABELS[:len(counts)]), counts)
        base = 1.5 * rng.standard_normal((n, 3))
        for k in range(K):
            if k % 3 == 2:
                c = 1.5 * rng.standard_normal((n, 3))
            else:
                c = (base * (mc.MIRROR if k % 2 else 1.0)) @ kc.random_rotation(rng).T + 3.0 * rng.standard_normal(3) \
                    + 0.05 * rng.standard_normal((n, 3))
            perm = rng.permutation(n)
            made[(name, k)] = [c[perm].astype(np.float32), sp0[perm].astype(np.int32)]
    long_rows = 1.5 * rng.standard_normal((mc.SIZES[mc.NAMES.index("n257")], 3))
    if special:
        made[("k8", 2)][0][5, 1] = np.inf
        made[("k3", 1)] = [made[("k3", 1)][0][:-1], made[("k3", 1)][1][:-1]]
        made[("k5", 3)][1][0] = 99
        made[("k3n65", 1)] = [long_rows.astype(np.float32), np.full(len(long_rows), LABELS[0], np.int32)]
    order = []
    for name, K, _ in SPEC:
        if name == INTERLEAVED[1]:
            continue
        if name == INTERLEAVED[0]:
            order += [(nm, k) for k in range(K) for nm in INTERLEAVED]
        else:
            order += [(name, k) for k in range(K)]
    index = {key: s for s, key in enumerate(order)}
    return dict(members=[made[key] for key in order], groups=[[index[(name, k)] for k in range(K)] for name, K, _ in SPEC])


def _wide(x, ld, dev):
    w = torch.full((max(len(x), 1), ld), float("nan"), device=dev)
    w[:len(x), :3] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return w


def _pairwise(members, groups, mode, reflect, cap=0.0, exact_limit=10000, ldx=3):
    """-> (list of [K, K] float32 matrices, list of [K, K] int32 status) of one `oard_pairwise_rmsd` launch; canaries checked."""
    _capi, L = _lib()
    dev = _dev()
    x = np.concatenate([m[0] for m in members]) if members else np.zeros((0, 3), np.float32)
    sp = np.concatenate([m[1] for m in members]) if members else np.zeros(0, np.int32)
    S = len(members)
    seg = torch.from_numpy(kc.seg_ptr([len(m[0]) for m in members]).astype(np.int32)).to(dev)
    group_ptr, pair_ptr, mat_ptr = pc.tables([len(g) for g in groups])
    G, P, M, T = len(groups), int(pair_ptr[-1]), int(group_ptr[-1]), int(mat_ptr[-1])
    mem = torch.tensor([s for g in groups for s in g] + [0], dtype=torch.int32, device=dev)
    d_gp = torch.from_numpy(group_ptr.astype(np.int32)).to(dev)
    d_pp, d_mp = torch.from_numpy(pair_ptr).to(dev), torch.from_numpy(mat_ptr).to(dev)
    wx = _wide(x, ldx, dev)
    dsp = torch.from_numpy(np.concatenate([sp, np.zeros(1, np.int32)])).to(dev)
    out = torch.full((GUARD + T + GUARD,), float("nan"), device=dev)
    out[GUARD: GUARD + T] = UNWRITTEN
    st = torch.full((GUARD + T + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.oard_pairwise_rmsd(wx.data_ptr(), ldx, dsp.data_ptr(), seg.data_ptr(), S, mem.data_ptr(), d_gp.data_ptr(), d_pp.data_ptr(),
                                  d_mp.data_ptr(), G, P, M, (1 if reflect else 0) | (2 if mode else 0), cap, exact_limit,
                                  out[GUARD:].data_ptr(), st[GUARD:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    assert ldx == 3 or bool(torch.isnan(wx[:, 3:]).all())
    assert bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[GUARD + T:]).all()), "a canary around out was written"
    assert bool((st[:GUARD] == SENTINEL).all()) and bool((st[GUARD + T:] == SENTINEL).all()), "a canary around status was written"
    o, s = out[GUARD: GUARD + T].cpu().numpy(), st[GUARD: GUARD + T].cpu().numpy()
    assert not (o == UNWRITTEN).any() and not (s == SENTINEL).any(), "an entry of a matrix was not written"
    K = [len(g) for g in groups]
    return ([o[mat_ptr[g]: mat_ptr[g + 1]].reshape(K[g], K[g]) for g in range(G)],
            [s[mat_ptr[g]: mat_ptr[g + 1]].reshape(K[g], K[g]) for g in range(G)])


def _explicit(members, groups, mode, reflect, cap=0.0, exact_limit=10000):
    """The parent's way to the same numbers: explicit copies of member i as a and member j as b for every pair i < j of equal, non-zero
    row counts, one `oard_kabsch_rmsd` / `oard_matched_rmsd` call -> {(g, i, j): (rmsd float32, status)}."""
    _capi, L = _lib()
    dev = _dev()
    keys, A, B, SA, SB = [], [], [], [], []
    for g, grp in enumerate(groups):
        for i in range(len(grp)):
            for j in range(i + 1, len(grp)):
                a, b = members[grp[i]], members[grp[j]]
                if len(a[0]) == len(b[0]) > 0:
                    keys.append((g, i, j)), A.append(a[0]), B.append(b[0]), SA.append(a[1]), SB.append(b[1])
    n = len(keys)
    da, db = (torch.from_numpy(np.concatenate(t)).to(dev) for t in (A, B))
    dsa, dsb = (torch.from_numpy(np.concatenate(t)).to(dev) for t in (SA, SB))
    seg = torch.from_numpy(kc.seg_ptr([len(a) for a in A]).astype(np.int32)).to(dev)
    r = torch.full((n,), float("nan"), device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if mode:
            rc = L.oard_matched_rmsd(da.data_ptr(), 3, db.data_ptr(), 3, dsa.data_ptr(), dsb.data_ptr(), seg.data_ptr(), n, int(reflect), cap,
                                     exact_limit, r.data_ptr(), None, None, None, st.data_ptr(), stream)
        else:
            rc = L.oard_kabsch_rmsd(da.data_ptr(), 3, db.data_ptr(), 3, seg.data_ptr(), n, int(reflect), cap, r.data_ptr(), None, None, stream)
    assert rc == _capi.OARD_OK
    torch.cuda.synchronize(dev)
    r, st = r.cpu().numpy(), st.cpu().numpy()
    return {k: (r[t], int(st[t])) for t, k in enumerate(keys)}


def _bits(v):
    return np.asarray(v, np.float32).view(np.int32)


@functools.lru_cache(maxsize=None)
def _clean(mode, reflect):
    mix = _mix()
    return _pairwise(mix["members"], mix["groups"], mode, reflect)


@pytest.mark.parametrize("reflect", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_bits_of_the_existing_kernels_and_matrix_form(mode, reflect):
    mix = _mix()
    out, st = _clean(mode, reflect)
    ref = _explicit(mix["members"], mix["groups"], mode, reflect)
    assert len(ref) == sum(K * (K - 1) // 2 for _, K, _ in SPEC)
    for (g, i, j), (r, code) in ref.items():
        assert _bits(out[g][i, j]) == _bits(r), (SPEC[g][0], i, j, out[g][i, j], r)
        assert st[g][i, j] == code, (SPEC[g][0], i, j)
    for g, (name, K, counts) in enumerate(SPEC):
        assert out[g].shape == (K, K)
        assert (_bits(out[g]) == _bits(out[g].T)).all() and (st[g] == st[g].T).all(), name
        assert (_bits(np.diag(out[g])) == 0).all() and (np.diag(st[g]) == 0).all(), name          # +0.0
        if mode and K > 1:                                      # the table of SPEC: which branch a group takes
            want = 0 if math.prod(math.factorial(c) for c in counts) < 10000 else 1
            assert (st[g][~np.eye(K, dtype=bool)] == want).all(), name
    # the row stride is only an address: the same bits from a padded array
    wide, wide_st = _pairwise(mix["members"], mix["groups"], mode, reflect, ldx=10)
    for g in range(len(SPEC)):
        assert (_bits(wide[g]) == _bits(out[g])).all() and (wide_st[g] == st[g]).all()


def _aligned_species(a, b):
    """b's rows reordered so that they carry a's species row by row (the minimum over the matchings does not depend on b's order)."""
    oa, ob = np.argsort(a[1], kind="stable"), np.argsort(b[1], kind="stable")
    idx = np.empty(len(oa), np.int64)
    idx[oa] = ob
    return b[0][idx]


@pytest.mark.parametrize("reflect", [False, True])
def test_float64_references(reflect):
    """Same-order entries against the SVD fit, exact-branch entries against every permutation; both under `_kabsch_cases.gate`."""
    mix = _mix()
    same, _ = _clean(0, reflect)
    matched, st = _clean(1, reflect)
    worst = 0.0
    for g, (name, K, counts) in enumerate(SPEC):
        grp = mix["groups"][g]
        for i in range(K):
            for j in range(i + 1, K):
                a, b = mix["members"][grp[i]], mix["members"][grp[j]]
                r, rho = kc.svd_rmsd(a[0], b[0], reflect)
                worst = max(worst, abs(float(same[g][i, j]) - r) / kc.gate(r, rho))
                assert abs(float(same[g][i, j]) - r) <= kc.gate(r, rho), (name, i, j, same[g][i, j], r)
                if st[g][i, j] == 0:
                    r = mc.brute(a[0], _aligned_species(a, b), a[1], reflect)[0]
                    worst = max(worst, abs(float(matched[g][i, j]) - r) / kc.gate(r, rho))
                    assert abs(float(matched[g][i, j]) - r) <= kc.gate(r, rho), (name, i, j, matched[g][i, j], r)
    print("worst |k - r| / gate:", worst)


def _expected_code(a, b, mode):
    """The status of a special pair (None: an ordinary one) by the rule of csrc/oard_pairwise.h: empty, then 3, 4, 5, 2."""
    if len(a[0]) == 0 or len(b[0]) == 0:
        return 0
    if mode and (len(a[0]) > 256 or len(b[0]) > 256):
        return 3
    if not (np.isfinite(a[0]).all() and np.isfinite(b[0]).all()):
        return 4
    if len(a[0]) != len(b[0]):
        return 5
    if mode and sorted(a[1].tolist()) != sorted(b[1].tolist()):
        return 2
    return None


@pytest.mark.parametrize("cap", [0.5, 0.0])
@pytest.mark.parametrize("mode", [0, 1])
def test_special_members_poison_their_row_and_column(mode, cap):
    clean, clean_st = _clean(mode, True)
    mix = _mix(special=True)
    out, st = _pairwise(mix["members"], mix["groups"], mode, True, cap=cap)
    seen = set()
    for g, (name, K, _) in enumerate(SPEC):
        grp = mix["groups"][g]
        for i in range(K):
            for j in range(K):
                code = _expected_code(mix["members"][grp[i]], mix["members"][grp[j]], mode)
                if i == j and code in (2, 5):
                    code = None
                if code is None:                                # untouched by the spoilt members: the clean launch's bits (under the cap)
                    want = np.minimum(clean[g][i, j], np.float32(cap)) if cap > 0 else clean[g][i, j]
                    assert _bits(out[g][i, j]) == _bits(want) and st[g][i, j] == clean_st[g][i, j], (name, i, j)
                else:
                    seen.add(code)
                    assert st[g][i, j] == code, (name, i, j, st[g][i, j], code)
                    assert _bits(out[g][i, j]) == _bits(np.float32(cap)) if cap > 0 else np.isnan(out[g][i, j]), (name, i, j)
    assert seen == ({2, 3, 4, 5} if mode else {4, 5})
    # the whole row and column of the member with the inf, its diagonal entry included
    g = [s[0] for s in SPEC].index("k8")
    assert (st[g][2, :] == 4).all() and (st[g][:, 2] == 4).all()
    if mode:
        g = [s[0] for s in SPEC].index("k3n65")
        assert (st[g][1, :] == 3).all() and (st[g][:, 1] == 3).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_a_group_alone_gives_the_same_bits(mode):
    mix = _mix()
    out, st = _clean(mode, True)
    for g, (name, K, _) in enumerate(SPEC):
        members = [mix["members"][s] for s in mix["groups"][g]]
        alone, alone_st = _pairwise(members, [list(range(K))], mode, True)
        assert (_bits(alone[0]) == _bits(out[g])).all() and (alone_st[0] == st[g]).all(), name


@pytest.mark.parametrize("mode", [0, 1])
def test_member_indices_outside_the_segments_are_empty_members(mode):
    mix = _mix()
    clean, clean_st = _clean(mode, True)
    groups = [list(g) for g in mix["groups"]]
    S = len(mix["members"])
    names = [s[0] for s in SPEC]
    groups[names.index("k3")][1] = -1
    groups[names.index("k8")][4] = S
    groups[names.index("k1")][0] = S + 5
    out, st = _pairwise(mix["members"], groups, mode, True)
    for g, (name, K, _) in enumerate(SPEC):
        empty = np.array([not 0 <= s < S for s in groups[g]], bool)
        touched = empty[:, None] | empty[None, :]
        assert np.isnan(out[g][touched]).all() and (st[g][touched] == 0).all(), name
        assert (_bits(out[g][~touched]) == _bits(clean[g][~touched])).all() and (st[g][~touched] == clean_st[g][~touched]).all(), name
    assert sum(int(np.isnan(o).sum()) for o in out) == (2 * 3 - 1) + (2 * 8 - 1) + 1
