"""The float64 geometry block ALONE (csrc/oard_kernels.h: k_geom, k_edge_geo, k_active_list, k_rbf, k_fill_edges):
the kernels every call of every path runs first, launched by tests/geometry/harness.hip exactly as forward_impl launches them, on
hand-made tables, and compared output by output with a numpy restatement of the reference (model/leftnet.py:693-722, 747-771, 781-785,
812-834, 63-69), evaluated in float64 and in np.longdouble on the float32 positions the device sees.  The node frame is the exact
form b = -a / (n_s - 1) (b = 0 for a lone node).  The reference here stands on its own: it does not call the oracle.

Tables.  Groups are (sample, object) pairs, rows sample-major; the inner list holds every ordered pair of a group, sorted by target;
node_ref is the object-major permutation.  A bad index is a GPU fault, so `validate` checks every table on the CPU before every launch.
Every output buffer is NaN / sentinel filled and carries guard rows that must come back untouched.  The row strides are the kernels' own
(12, RP, WP), so the guard COLUMNS are the cells inside a row a kernel must leave alone: the first 3 H columns of an inner row of the
edge state (k_rbf), and the NaN-filled columns R..RP of the means and betas, which must not be read into a result.

Gates - all derived, none measured on the kernels.  u = 2^-53.
  integers: exact.  labels = node_ref of the centre the reference assigns; geo[:, 11] = mask; blk_cnt, rows, src, pre[0..A], n_act = numpy's
      compaction of the mask.
  pf64:  a = x - (sum of cnt members) / cnt: cnt - 1 additions and one division on the scale mean|x|, one subtraction on |a|:
      |got - ref_ld| <= u ((cnt + 1) mean|x| + |a|)  (K = cnt + 2 <= ng + 2 on max(mean|x|, |a|); one more than counted, for the second
      order).  cnt = 1: x / 1 and x - x are exact, the gate is 0.
  d64:   d = m sqrt(dx^2 + dy^2 + dz^2), dx = a_i - b_j: one subtraction, three products, two sums, one square root = at most
      1 + (1 + 2) / 2 + 1 < 4 roundings relative to d (K = 4), plus the float64 error of its inputs, |e(a_i) + e(b_j)|_2.
      The float64 numpy reference must meet both bounds against longdouble as well (asserted).
  float32 outputs: per entry |got - ref| <= 2^-23 |ref| + T + 2^-149 (one float32 rounding of a float64 value that may sit on a rounding
      boundary; the last term is the spacing of float32 below 2^-126).  T = the float64 side amplified by the entry's conditioning, with
      e(a) = |gate of pf64|_2 of the node, eps = 1e-6:
        pf32: the pf64 gate.     geo d: the d64 gate.
        x1 = k a / (|k a| + eps):  2 k e(a) / (|k a| + eps) + 6u        (normalising doubles an error; 6 roundings on |x1| <= 1)
        pp0 = a . x1:              e(a) + sqrt(3) |a| T(x1) + 4u |a|
        u = (a - b) / (|a - b| + eps):   m (2 (|e(a) + e(b)|_2 + u |a - b|) / (|a - b| + eps) + 6u)
        c = w / (|w| + eps), w = a x b:  m (2 (e(a) |b| + |a| e(b) + 4u |a||b|) / (|w| + eps) + 6u)  - the |a||b| / (|a x b| + eps) form:
              two products and a difference per component
        v = u x c:                 m (2 (T(u) + T(c)) + 4u)
        env = (cos(pi d / cutoff) + 1) / 2:   pi / (2 cutoff) gate(d64) + 8u
        rbf_k = rb(d) G m, G = exp(-beta q^2), q = exp(-d) - mu:  gate(d64) (pi / (2 cutoff) G + rb G 2 beta |q| exp(-d))
              + u (rb G (8 + 4 beta q^2 + 8 beta |q|) + 8 G)   (roundings of q and beta q^2 through exp; cos and exp a few ulps)
  padding: rbuf[:, R:RP] = 0; ew[:, 3H+R:WP] = 0 on inner rows; ew[:, :3H] of inner rows untouched by k_rbf; rows A..E of ew = c0row;
      nothing behind row E written.

Conditions, asserted from the reference alone before any comparison: no pair within 1e-9 (relative) of the cutoff, in raw or in
pos_frame distance, apart from the lattice's pairs at exactly the cutoff (exact integer arithmetic: no rounding can move them); float64
and longdouble give the same masks and labels; `chain` and `sizes` overwrite at least a third of their nodes' first labels.
An inner list of complete groups has an even length, so the launch that ends one short of a multiple of 256 rows is a PREFIX of the
`sizes` list (the kernels read act_src / act_tgt / A only); the one that ends on a multiple is the 257-atom group alone (257 x 256)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U53, U23, F32_TINY = 2.0 ** -53, 2.0 ** -23, 2.0 ** -149
EPS = 1e-6
MAX_GROUP = 1024                                        # OARD_MAX_GROUP (csrc/oard_layout.h)
GUARD, ISENT = 2, -7                                    # guard rows behind every output; the integer sentinel
DIMS = [(196, 96), (32, 8), (32, 32)]                   # the instantiated (H, R); (32, 8): RP = 16 > R
X_ROWS = 7                                              # inter-object rows of the edge state behind the inner ones (E = A + X_ROWS)


def pad16(n):
    return (n + 15) // 16 * 16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # as oareactdiff_amd/build.py finds it
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    so = str(tmp_path_factory.mktemp("geometry") / "libgeometry_block.so")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-result",
                        os.path.join(HERE, "geometry", "harness.hip"), "-o", so], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    L = C.CDLL(so)                                       # local symbol scope
    i, p, ll = C.c_int, C.c_void_p, C.c_longlong
    L.geometry_block.argtypes = [i, i, i, ll, ll] + [p] * 7 + [C.c_double] + [p] * 17 + [i, i, i, p]
    L.geometry_block.restype = i
    return L


# ---- tables --------------------------------------------------------------------------------------------------------------------------
class Tables:
    """layout[b][k] = atoms of object k in sample b.  Rows are sample-major, object-minor (group q = b * n_obj + k is contiguous)."""

    def __init__(self, layout):
        lay = np.asarray(layout, dtype=np.int64)
        self.B, self.n_obj = lay.shape
        self.n_groups = self.B * self.n_obj
        sizes = lay.reshape(-1)
        self.grp_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.sample_ptr = np.concatenate([[0], np.cumsum(lay.sum(1))]).astype(np.int32)
        self.N = int(sizes.sum())
        self.node_group = np.repeat(np.arange(self.n_groups), sizes).astype(np.int32)
        self.node_sample = (self.node_group // self.n_obj).astype(np.int32)
        # reference order: object-major, samples in order inside an object
        obj_start = np.concatenate([[0], np.cumsum(lay.sum(0))])
        before = np.cumsum(lay, axis=0) - lay                                  # atoms of object k in the samples in front of b
        self.node_ref = np.empty(self.N, dtype=np.int32)
        src, tgt = [], []
        for q in range(self.n_groups):
            g0, ng = int(self.grp_ptr[q]), int(sizes[q])
            b, k = divmod(q, self.n_obj)
            self.node_ref[g0:g0 + ng] = obj_start[k] + before[b, k] + np.arange(ng)
            if ng > 1:                                                          # every ordered pair, target-major
                t, s = np.repeat(np.arange(ng), ng), np.tile(np.arange(ng), ng)
                keep = t != s
                src.append(g0 + s[keep])
                tgt.append(g0 + t[keep])
        self.act_src = np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32)
        self.act_tgt = np.concatenate(tgt).astype(np.int32) if tgt else np.zeros(0, np.int32)
        self.A = int(self.act_src.size)

    @classmethod
    def of(cls, N, B, n_obj, grp_ptr, sample_ptr, node_sample, node_ref, act_src, act_tgt):
        """The same object from tables somebody else built."""
        t = cls.__new__(cls)
        t.N, t.B, t.n_obj, t.n_groups = N, B, n_obj, B * n_obj
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        t.grp_ptr, t.sample_ptr, t.node_sample, t.node_ref = i32(grp_ptr), i32(sample_ptr), i32(node_sample), i32(node_ref)
        t.act_src, t.act_tgt = i32(act_src), i32(act_tgt)
        t.A = int(t.act_src.size)
        t.node_group = np.repeat(np.arange(t.n_groups), np.diff(t.grp_ptr)).astype(np.int32)
        return t


def validate(t, A, pos):
    """Everything a kernel indexes with, checked on the CPU: a table that fails here is never launched."""
    assert t.N >= 1 and t.n_groups >= 1 and 0 <= A <= t.A
    assert pos.shape == (t.N, 3) and pos.dtype == np.float32 and np.isfinite(pos).all()
    assert t.grp_ptr.shape == (t.n_groups + 1,) and t.grp_ptr[0] == 0 and t.grp_ptr[-1] == t.N
    ng = np.diff(t.grp_ptr.astype(np.int64))
    assert (ng >= 0).all() and ng.max() <= MAX_GROUP
    assert t.sample_ptr.shape == (t.B + 1,) and t.sample_ptr[0] == 0 and t.sample_ptr[-1] == t.N
    assert (np.diff(t.sample_ptr.astype(np.int64)) >= 0).all()
    assert t.node_sample.shape == (t.N,) and t.node_sample.min() >= 0 and t.node_sample.max() < t.B
    assert (np.repeat(np.arange(t.B), np.diff(t.sample_ptr)) == t.node_sample).all()          # a node lies inside its sample's range
    assert (t.node_group // t.n_obj == t.node_sample).all()                                  # and a group inside one sample
    assert t.node_ref.shape == (t.N,) and (np.sort(t.node_ref) == np.arange(t.N)).all()      # a permutation
    for a in (t.act_src, t.act_tgt):
        assert a.shape == (t.A,) and (t.A == 0 or (a.min() >= 0 and a.max() < t.N))
    assert (t.node_group[t.act_src] == t.node_group[t.act_tgt]).all() and (t.act_src != t.act_tgt).all()
    assert (np.diff(t.act_tgt.astype(np.int64)) >= 0).all()                                  # target-sorted
    for a in (t.grp_ptr, t.sample_ptr, t.node_sample, t.node_ref, t.act_src, t.act_tgt):
        assert a.dtype == np.int32 and a.flags.c_contiguous


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def norm3(x):
    return np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


class Ref:
    """leftnet.py:747-761 (cutoff mask, one-hop labelling with overwrites, label-mean removal), 693-705 and 768-771 (edge frame, masked),
    785 (envelope), 812-834 with the exact node frame; in dtype `dt` on float32 positions."""

    def __init__(self, t, pos32, cutoff, dt):
        self.dt, self.cutoff = dt, cutoff
        pos = pos32.astype(dt)
        cut, eps, pi = dt(cutoff), dt(EPS), dt(np.pi)
        i, j = t.act_src.astype(np.int64), t.act_tgt.astype(np.int64)
        self.raw = norm3(pos[i] - pos[j])                                   # :747
        self.mask = self.raw < cut                                          # :749, strict
        # assemble_nodemask, :707-722: centres in row order; a centre labels its in-cutoff neighbours, overwriting earlier labels
        lab, first = np.full(t.N, -1, np.int64), np.full(t.N, -1, np.int64)
        pf, cnt, meanabs = np.zeros((t.N, 3), dt), np.ones(t.N, np.int64), np.zeros((t.N, 3))
        e0 = 0
        for q in range(t.n_groups):
            g0, g1 = int(t.grp_ptr[q]), int(t.grp_ptr[q + 1])
            ng = g1 - g0
            if ng == 0:
                continue
            adj = np.zeros((ng, ng), bool)
            ne = ng * (ng - 1)
            adj[i[e0:e0 + ne] - g0, j[e0:e0 + ne] - g0] = self.mask[e0:e0 + ne]
            e0 += ne
            gl, gf = lab[g0:g1], first[g0:g1]
            for c in range(ng):
                if gl[c] > -1:
                    continue
                con = adj[c].copy()
                con[c] = True
                gl[con] = c
                gf[con & (gf < 0)] = c
            for c in np.unique(gl):                                         # remove_mean_batch, :761
                mem = np.nonzero(gl == c)[0] + g0
                mean = pos[mem].sum(0) / dt(mem.size)
                pf[mem] = pos[mem] - mean
                cnt[mem] = mem.size
                meanabs[mem] = np.abs(pos32[mem].astype(np.float64)).sum(0) / mem.size
            lab[g0:g1] += g0
            first[g0:g1] += g0
        assert e0 == t.A
        self.centre, self.first = lab, first                                # row of the centre: final, and the first one assigned
        self.labels = t.node_ref[lab]
        self.pf, self.cnt, self.meanabs = pf, cnt, meanabs
        # node frame, :812-834 in its exact form: b = -a / (n_s - 1)
        ns = np.diff(t.sample_ptr.astype(np.int64))[t.node_sample]
        k = np.where(ns > 1, dt(1) + dt(1) / np.maximum(ns - 1, 1).astype(dt), dt(1))
        amb = pf * k[:, None]
        self.k, self.nr_node = k, norm3(amb) + eps
        self.x1 = amb / self.nr_node[:, None]
        self.pp0 = (pf * self.x1).sum(1)
        # scalarization, :693-705, masked :768-771
        a, b = pf[i], pf[j]
        m = self.mask.astype(dt)
        diff = a - b
        self.dist = norm3(diff)
        self.na, self.nb = norm3(a), norm3(b)
        w = cross3(a, b)
        self.nw = norm3(w)
        u = diff / (self.dist + eps)[:, None]
        c = w / (self.nw + eps)[:, None]
        v = cross3(u, c)
        self.d = self.dist * m
        self.env = (np.cos(self.d * pi / cut) + dt(1)) * dt(0.5)              # :785
        self.geo = np.concatenate([self.d[:, None], self.env[:, None], u * m[:, None], c * m[:, None], v * m[:, None]], 1)

    def rbf(self, means32, betas32):
        """:63-69, 781-782 -> [A, R]"""
        dt = self.dt
        d, mu, beta = self.d[:, None], means32.astype(dt)[None, :], betas32.astype(dt)[None, :]
        rb = (np.cos(d * dt(np.pi) / dt(self.cutoff)) + dt(1)) * dt(0.5) * (d < dt(self.cutoff))
        q = np.exp(-d) - mu
        return rb * np.exp(-beta * q * q) * self.mask.astype(dt)[:, None]


class Gates:
    """The tolerances of the module docstring, from the longdouble reference `r` (float64 arrays)."""

    def __init__(self, t, r):
        f = lambda x: np.asarray(x, dtype=np.float64)
        i, j = t.act_src.astype(np.int64), t.act_tgt.astype(np.int64)
        m, eps = f(r.mask), EPS
        self.pf = U53 * ((r.cnt[:, None] + 1) * r.meanabs + np.abs(f(r.pf))) * (r.cnt[:, None] > 1)
        ea = np.sqrt((self.pf ** 2).sum(1))
        na_node, k = norm3(f(r.pf)), f(r.k)
        self.x1 = (2 * k * ea / f(r.nr_node) + 6 * U53)[:, None]
        self.pp0 = ea + np.sqrt(3.0) * na_node * self.x1[:, 0] + 4 * U53 * na_node
        dist, na, nb, nw = f(r.dist), f(r.na), f(r.nb), f(r.nw)
        e_in = np.sqrt(((self.pf[i] + self.pf[j]) ** 2).sum(1))
        self.d = m * (4 * U53 * dist + e_in)
        tu = m * (2 * (e_in + U53 * dist) / (dist + eps) + 6 * U53)
        tc = m * (2 * (ea[i] * nb + na * ea[j] + 4 * U53 * na * nb) / (nw + eps) + 6 * U53)
        tv = m * (2 * (tu + tc) + 4 * U53)
        self.env = np.pi / (2 * r.cutoff) * self.d + 8 * U53
        self.geo = np.concatenate([self.d[:, None], self.env[:, None]] + [np.repeat(x[:, None], 3, 1) for x in (tu, tc, tv)], 1)
        ratio = m * na * nb / (nw + eps)                                    # conditioning of c; pairs parallel to rounding (a = -b) apart
        ratio = ratio[nw > 1e-9 * na * nb]
        self.cond_c = float(ratio.max()) if ratio.size else 0.0

    def rbf(self, r, means32, betas32):
        d, mu, beta = np.asarray(r.d, np.float64)[:, None], means32.astype(np.float64)[None, :], betas32.astype(np.float64)[None, :]
        rb = 0.5 * (np.cos(d * np.pi / r.cutoff) + 1.0) * (d < r.cutoff)
        q = np.exp(-d) - mu
        G = np.exp(-beta * q * q)
        return (self.d[:, None] * (np.pi / (2 * r.cutoff) * G + rb * G * 2 * beta * np.abs(q) * np.exp(-d))
                + U53 * (rb * G * (8 + 4 * beta * q * q + 8 * beta * np.abs(q)) + 8 * G)) * np.asarray(r.mask, np.float64)[:, None]


def rbf_params(R, cutoff):
    """The reference's initial values (leftnet.py:47-56), as float32"""
    start = np.exp(-cutoff)
    means = np.linspace(start, 1.0, R).astype(np.float32)
    betas = np.full(R, (2.0 / R * (1.0 - start)) ** -2, dtype=np.float32)
    return means, betas


def ratio64(got, ref, gate, what):
    """max |got - ref| / gate for a float64 output; an exact gate (0) admits exactly the reference"""
    assert np.isfinite(got).all(), f"{what}: not written, or not finite"
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    if err.size == 0:
        return 0.0
    assert (err[gate == 0] == 0).all(), f"{what}: an entry with an exact gate differs"
    return float((err[gate > 0] / gate[gate > 0]).max()) if (gate > 0).any() else 0.0


def ratio32(got, ref, T, what):
    """max over the entries of |got - ref| / (2^-23 |ref| + T + 2^-149)"""
    assert got.dtype == np.float32 and np.isfinite(got).all(), f"{what}: not written, or not finite"
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    return float((err / (U23 * np.abs(ref).astype(np.float64) + T + F32_TINY)).max())


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """Tables, float32 positions and both references of one case; made once per module and not changed."""

    def __init__(self, name, layout, pos, cutoff=10.0, exact_pairs=0, min_overwritten=0.0, tables=None):
        self.name, self.cutoff = name, float(cutoff)
        self.t = Tables(layout) if tables is None else tables
        self.pos = np.ascontiguousarray(pos, dtype=np.float32)
        validate(self.t, self.t.A, self.pos)
        self.r64, self.r = Ref(self.t, self.pos, self.cutoff, np.float64), Ref(self.t, self.pos, self.cutoff, LD)
        self.g = Gates(self.t, self.r)
        self._conditions(exact_pairs, min_overwritten)

    def _conditions(self, exact_pairs, min_overwritten):
        r, r64, g, cut = self.r, self.r64, self.g, self.cutoff
        assert (r.mask == r64.mask).all() and (r.labels == r64.labels).all() and (r.first == r64.first).all(), self.name
        near = np.abs(r.raw.astype(np.float64) - cut) <= 1e-9 * cut
        assert int(near.sum()) == exact_pairs and (r.raw[near] == cut).all() and (r64.raw[near] == cut).all() and not r.mask[near].any(), \
            (self.name, "pairs within 1e-9 of the cutoff that are not the declared exact ones")
        assert not (r.mask & (np.abs(r.dist.astype(np.float64) - cut) <= 1e-9 * cut)).any(), (self.name, "pos_frame distance at the cutoff")
        self.overwritten = float((r.centre != r.first).mean())
        assert self.overwritten >= min_overwritten, (self.name, self.overwritten)
        # the derivation of the float64 gates, checked on numpy's own float64 evaluation
        assert ratio64(r64.pf.astype(np.float64), r.pf, g.pf, "pf64 (numpy)") <= 1.0
        assert ratio64(r64.d.astype(np.float64), r.d, g.d, "d64 (numpy)") <= 1.0
        n_lab = len(np.unique(r.centre))
        print(f"{self.name}: N {self.t.N} A {self.t.A} inside {float(r.mask.mean()) if r.mask.size else 0.0:.3f} labels {n_lab} "
              f"overwritten {self.overwritten:.3f} max |a||b|/(|axb|+eps) {g.cond_c:.3g} max T(c) {float(g.geo[:, 5].max()) if r.mask.size else 0.0:.2e}")


def _lattice():
    y = np.nextafter(np.float32(8), np.float32(0))
    pos = np.array([[0, 0, 0], [6, 8, 0], [10, 0, 0], [6, y, 0], [3, 4, 0], [3, 4, 0],          # object 0: two pairs AT the cutoff, one just inside, two coincident
                    [1, 2, 2], [4, 6, 2],                                                       # object 1: two atoms, a = -b
                    [7, 7, 7]], dtype=np.float32)                                               # object 2: one atom
    c = Case("lattice", [(6, 2, 1)], pos, exact_pairs=4)
    r = c.r
    e = {(int(s), int(t)): k for k, (s, t) in enumerate(zip(c.t.act_src, c.t.act_tgt))}
    assert not r.mask[e[0, 1]] and not r.mask[e[0, 2]] and r.raw[e[0, 1]] == 10 and r.raw[e[0, 2]] == 10
    assert r.mask[e[0, 3]] and abs(float(r.raw[e[0, 3]]) - 9.99999962) < 1e-8
    assert r.mask[e[4, 5]] and r.d[e[4, 5]] == 0 and not r.geo[e[4, 5], 2:].any() and r.env[e[4, 5]] == 1
    assert (r.pf[6] == -r.pf[7]).all() and not r.geo[e[6, 7], 5:8].any()
    assert not r.pf[8].any() and not r.x1[8].any() and r.pp0[8] == 0
    assert r.centre.tolist() == [0, 1, 1, 1, 1, 1, 6, 6, 8] and r.first.tolist() == [0, 1, 1, 0, 0, 0, 6, 6, 8]
    return c


def _lone():
    layout = [(3, 2), (1, 0), (4, 3)]
    pos = np.random.default_rng(1).normal(size=(13, 3)) * 4
    c = Case("lone", layout, pos)
    assert c.r.k[5] == 1 and not c.r.pf[5].any() and not c.r.x1[5].any() and c.r.pp0[5] == 0
    return c


def _chain():
    g = np.random.default_rng(0)
    line = np.zeros((70, 3))
    line[:, 0] = 0.45 * 10.0 * np.arange(70)
    pos = np.concatenate([line + g.normal(scale=0.02, size=(70, 3)), g.normal(size=(5, 3)) * 4])
    c = Case("chain", [(70, 3, 2)], pos, min_overwritten=1 / 3)
    assert c.g.cond_c > 1e3, "pos_frame pairs are meant to be nearly (anti)parallel"
    return c


SIZES_LAYOUT = [(257, 1, 2), (63, 64, 65), (129, 0, 1)]


def _sizes_pos():
    return np.random.default_rng(3).normal(size=(sum(map(sum, SIZES_LAYOUT)), 3)) * 4


def _sizes():
    return Case("sizes", SIZES_LAYOUT, _sizes_pos(), min_overwritten=1 / 3)


def _g257():
    c = Case("g257", [(257, 1, 1)], _sizes_pos()[:259], min_overwritten=1 / 3)
    assert c.t.A == 257 * 256
    return c


def _limit():
    c = Case("limit", [(MAX_GROUP, 1, 1)], np.random.default_rng(4).normal(size=(MAX_GROUP + 2, 3)) * 4)
    assert c.t.A == 1047552
    return c


def _outside():
    c = Case("outside", SIZES_LAYOUT, _sizes_pos() * 60)
    assert not c.r.mask.any() and (c.r.centre == np.arange(c.t.N)).all() and not c.r.pf.any() and not c.r.geo[:, :1].any()
    return c


def _ones():
    c = Case("ones", [(1, 1, 1)] * 4 + [(1, 0, 1)], np.random.default_rng(5).normal(size=(14, 3)) * 4)
    assert c.t.A == 0
    return c


MAKERS = dict(lattice=_lattice, lone=_lone, chain=_chain, sizes=_sizes, g257=_g257, limit=_limit, outside=_outside, ones=_ones)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = MAKERS[name]()
        return cache[name]
    yield get
    cache.clear()


# ---- one launch ----------------------------------------------------------------------------------------------------------------------------
def launch(L, c, dims=None, A=None, training=False):
    """The block on case `c` (the first A inner rows; all of them by default) -> host copies of every output, after the write checks:
    guard rows untouched everywhere, and the edge state's regions (module docstring)."""
    t, dev = c.t, torch.device("cuda:0")
    A = t.A if A is None else A
    validate(t, A, c.pos)
    E, N = A + X_ROWS, t.N
    nblk = (A + 255) // 256
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tabs = [up(x if x.size else np.zeros(1, np.int32)) for x in (t.grp_ptr, t.node_sample, t.sample_ptr, t.node_ref, t.act_src[:A], t.act_tgt[:A])]
    pos = up(c.pos)
    nan = float("nan")
    full = lambda shape, v, dt=torch.float32: torch.full(shape, v, dtype=dt, device=dev)
    o = dict(pf64=full((N + GUARD, 3), nan, torch.float64), pf32=full((N + GUARD, 3), nan), x1=full((N + GUARD, 3), nan),
             pp0=full((N + GUARD,), nan), labels=full((N + GUARD,), ISENT, torch.int32), geo=full((A + GUARD, 12), nan),
             d64=full((A + GUARD,), nan, torch.float64), blk_cnt=full((nblk + GUARD,), ISENT, torch.int32),
             rows=full((A + GUARD,), ISENT, torch.int32), src=full((A + GUARD,), ISENT, torch.int32),
             pre=full((A + 1 + GUARD,), ISENT, torch.int32), n_act=full((1 + GUARD,), ISENT, torch.int32))
    flags = (1 if training else 0) | (0 if dims else 2)
    H, R = dims if dims else (0, 0)
    RP, WP = pad16(R), pad16(3 * H + R)
    if dims:
        means, betas = rbf_params(R, c.cutoff)
        mp, bp = np.full(RP, np.nan, np.float32), np.full(RP, np.nan, np.float32)       # columns R..RP of the parameters are never to be read
        mp[:R], bp[:R] = means, betas
        c0 = np.random.default_rng(7).normal(size=WP).astype(np.float32)
        par = [up(mp), up(bp), up(c0)]
        o.update(rbuf=full((A + GUARD, RP), nan), ew=full((E + 1 + GUARD, WP), nan))
        # sizes from the tables: the last cell each kernel can reach
        assert o["rbuf"].numel() >= A * RP and o["ew"].numel() >= (E + 1) * WP and WP % 4 == 0
    assert o["geo"].numel() >= A * 12 and o["pre"].numel() >= A + 1 and o["blk_cnt"].numel() >= nblk and A < 2 ** 31
    ptr = lambda x: x.data_ptr()
    args = [ptr(x) for x in tabs] + [ptr(pos), c.cutoff] + [ptr(o[k]) for k in ("pf64", "pf32", "x1", "pp0", "labels", "geo", "d64", "blk_cnt", "rows", "src", "pre", "n_act")]
    args += [ptr(x) for x in par] + [ptr(o["rbuf"]), ptr(o["ew"])] if dims else [None] * 5
    torch.cuda.synchronize(dev)
    rc = L.geometry_block(N, t.B, t.n_groups, A, E, *args, H, R, flags, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, (c.name, rc)
    out = {}
    if dims:
        ew = o.pop("ew")
        if A:
            assert bool(torch.isnan(ew[:A, :3 * H]).all()), f"{c.name}: k_rbf wrote into the first 3 H columns of an inner row"
        assert bool(torch.isnan(ew[E + 1:]).all()), f"{c.name}: the edge state was written behind row E"
        out["ew_rbf"], out["ew_rest"] = ew[:A, 3 * H:].cpu().numpy(), ew[A:E + 1].cpu().numpy()
        assert (out["ew_rest"] == c0[None, :]).all(), f"{c.name}: rows A..E of the edge state are not the constant row"
        out["c0"] = c0
    for k, v in o.items():
        out[k] = v.cpu().numpy()
    for k, n in (("pf64", N), ("pf32", N), ("x1", N), ("pp0", N), ("geo", A), ("d64", A)) + ((("rbuf", A),) if dims else ()):
        assert np.isnan(out[k][n:]).all(), f"{c.name}: {k} written behind its last row"
        out[k] = out[k][:n]
    assert (out["labels"][N:] == ISENT).all()
    out["labels"] = out["labels"][:N]
    out["A"], out["dims"] = A, dims
    return out


def check(c, out, training=False):
    """Every output of one launch against the longdouble reference; prints the worst ratio to its gate per output."""
    t, r, g, A, name = c.t, c.r, c.g, out["A"], c.name
    worst = {}
    # k_geom
    assert (out["labels"] == r.labels).all(), f"{name}: labels"
    worst["pf64"] = ratio64(out["pf64"], r.pf, g.pf, "pf64")
    worst["pf32"] = ratio32(out["pf32"], r.pf, g.pf, "pf32")
    worst["x1"] = ratio32(out["x1"], r.x1, g.x1, "x1")
    worst["pp0"] = ratio32(out["pp0"], r.pp0, g.pp0, "pp0")
    # k_edge_geo
    if A == 0:
        assert np.isnan(out["geo"]).all() and np.isnan(out["d64"]).all()
    mask = r.mask[:A]
    assert (out["geo"][:, 11] == mask.astype(np.float32)).all(), f"{name}: geo[:, 11] is not the mask"
    worst["d64"] = ratio64(out["d64"], r.d[:A], g.d[:A], "d64")
    for k, (lo, hi) in dict(d=(0, 1), env=(1, 2), u=(2, 5), c=(5, 8), v=(8, 11)).items():
        worst["geo." + k] = ratio32(out["geo"][:, lo:hi], r.geo[:A, lo:hi], g.geo[:A, lo:hi], "geo." + k)
    # k_active_list
    nblk = (A + 255) // 256
    if training or A == 0:
        for k in ("blk_cnt", "rows", "src", "pre", "n_act"):
            assert (out[k] == ISENT).all(), f"{name}: {k} written without an active list"
    else:
        cnt = np.add.reduceat(mask.astype(np.int64), np.arange(0, A, 256))
        act = np.nonzero(mask)[0]
        n_act = int(act.size)
        assert (out["blk_cnt"][:nblk] == cnt).all() and (out["blk_cnt"][nblk:] == ISENT).all(), f"{name}: blk_cnt"
        assert (out["rows"][:n_act] == act).all() and (out["rows"][n_act:] == ISENT).all(), f"{name}: rows"
        assert (out["src"][:n_act] == t.act_src[act]).all() and (out["src"][n_act:] == ISENT).all(), f"{name}: src"
        assert (out["pre"][:A + 1] == np.concatenate([[0], np.cumsum(mask)])).all() and (out["pre"][A + 1:] == ISENT).all(), f"{name}: pre"
        assert out["n_act"][0] == n_act and (out["n_act"][1:] == ISENT).all(), f"{name}: n_act"
    # k_rbf
    if out["dims"]:
        H, R = out["dims"]
        RP, WP = pad16(R), pad16(3 * H + R)
        means, betas = rbf_params(R, c.cutoff)
        ref, T = r.rbf(means, betas)[:A], g.rbf(r, means, betas)[:A]
        worst["rbuf"] = ratio32(out["rbuf"][:, :R], ref, T, "rbuf")
        worst["ew.rbf"] = ratio32(out["ew_rbf"][:, :R], ref, T, "ew.rbf")
        assert (out["rbuf"][:, R:] == 0).all(), f"{name}: rbuf padding"
        assert out["ew_rbf"].shape[1] == WP - 3 * H and (out["ew_rbf"][:, R:] == 0).all(), f"{name}: edge-state padding"
    tag = f"{name}{'' if A == t.A else '[:%d]' % A}{' training' if training else ''} {out['dims'] or ''}"
    print(f"{tag}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, bad)


# ---- 1. the kernels alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "h%d_r%d" % d)
def test_lattice_exact_cutoff_and_degenerate_frames(lib, cases, dims):
    """Integer coordinates: the strict < at distance == cutoff, one float32 ulp inside it, coincident atoms, a two-atom and a one-atom object."""
    c = cases("lattice")
    check(c, launch(lib, c, dims))


def test_lone_sample(lib, cases):
    """n_s = 1: k = 1, no division by n_s - 1; an empty group (ng = 0) beside it."""
    c = cases("lone")
    check(c, launch(lib, c, (32, 8)))


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "h%d_r%d" % d)
def test_chain_overwrites_and_parallel_frames(lib, cases, dims):
    """70 atoms on a line, 4.5 apart: a group above 64 atoms whose labels are mostly overwritten, and coord_cross of nearly (anti)parallel pairs."""
    c = cases("chain")
    check(c, launch(lib, c, dims))


def test_group_sizes_and_the_block_prefix(lib, cases):
    """Groups of 1, 2, 63, 64, 65, 129, 257 atoms: k_geom's 64-thread strides; 369 blocks: k_active_list's prefix beyond one stride."""
    c = cases("sizes")
    check(c, launch(lib, c, (32, 8)))


def test_launch_ends_one_row_short_of_a_block(lib, cases):
    """A = 94207 = 368 * 256 - 1: the last thread of the last block is the only one without a row."""
    c = cases("sizes")
    A = c.t.A // 256 * 256 - 1
    assert A % 256 == 255 and A > 256 * 256
    check(c, launch(lib, c, (32, 8), A=A))


def test_launch_ends_on_a_block(lib, cases):
    """The 257-atom group alone: A = 65792 = 257 blocks exactly; the last row is thread 255 of block 256, whose base is one full stride
    of 256 block counts (`sizes` and `limit` go beyond it)."""
    c = cases("g257")
    check(c, launch(lib, c, (32, 32)))


def test_limit_group(lib, cases):
    """OARD_MAX_GROUP atoms in one group: 16 strides of k_geom, 4092 blocks."""
    c = cases("limit")
    check(c, launch(lib, c, (32, 8)))


def test_everything_outside_the_cutoff(lib, cases):
    c = cases("outside")
    out = launch(lib, c, (32, 8))
    assert out["n_act"][0] == 0 and not out["pf64"].any() and not out["geo"][:, 11].any() and not out["rbuf"].any()
    check(c, out)


def test_one_atom_objects_only(lib, cases):
    """A = 0: k_geom alone; the edge state is the constant row throughout."""
    c = cases("ones")
    check(c, launch(lib, c, (32, 8)))


@pytest.mark.parametrize("name", ["lattice", "sizes"])
def test_training_form(lib, cases, name):
    """k_edge_geo without block counts, no active list: the same geometry, and none of the list's buffers touched."""
    c = cases(name)
    check(c, launch(lib, c, (32, 8), training=True), training=True)


# ---- 2. the product's own tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "cutoff"])
def test_taped_geometry_of_the_training_forward(name):
    """The training-mode forward through the C ABI on a ragged batch: the topology builder's tables equal the ones this file makes from
    the batch's sizes (target-sorted inner list, node_ref, groups), and the taped geo / rbf / pp0 / x1 - the INPUTS of every
    teacher-forced stage check - meet the float32 gates against the reference on the positions the device saw."""
    from _grad_cases import CNF, NODE_NFS, SyntheticGradCase
    from oareactdiff_amd import _capi, training
    from oareactdiff_amd.dynamics import EGNNDynamics
    c = SyntheticGradCase(name, references=False)
    dev = torch.device("cuda:0")
    dyn = EGNNDynamics(model_config=dict(c.cfg), fragment_names=["R", "TS", "P"], node_nfs=NODE_NFS, edge_nf=0, condition_nf=CNF, device=dev)
    sd = c.state_dict()
    dyn.load_state_dict(sd, strict=True)
    keep, orig = {}, training.DynamicsFunction.forward

    def spy(ctx, dyn_, run_forward, n_obj, *tensors):        # as _stage_checks.run keeps the step's state
        o = orig(ctx, dyn_, run_forward, n_obj, *tensors)
        keep["state"] = ctx.state
        return o
    training.DynamicsFunction.forward = staticmethod(spy)
    try:
        c.loss(dyn, torch.float32, dev)
    finally:
        training.DynamicsFunction.forward = orig
    st = keep["state"]
    tape, topo = st.tape, st.topo
    H, R = dyn._dims[0], dyn._dims[1]
    N, A, B = topo.N, topo.A, topo.B
    assert [N, topo.E, A] == list(c.spec.nea)
    mine = Tables(c.meta["sizes"])
    cpu = lambda x: x.cpu().numpy()
    assert (cpu(topo.node_group) == mine.node_group).all() and (cpu(topo.node_sample) == mine.node_sample).all()
    assert (cpu(topo.node_ref) == mine.node_ref).all()
    assert A == mine.A and (cpu(topo.inner_src) == mine.act_src).all() and (cpu(topo.inner_tgt) == mine.act_tgt).all()
    pos = torch.cat([x[:, :3] for x in st.xh]).float()[topo.node_ref]
    means = [v for k, v in sd.items() if k.endswith("radial_emb.means")][0].float().numpy()
    betas = [v for k, v in sd.items() if k.endswith("radial_emb.betas")][0].float().numpy()
    case = Case("taped " + name, None, cpu(pos), cutoff=c.spec.cutoff,
                tables=Tables.of(N, B, mine.n_obj, mine.grp_ptr, mine.sample_ptr, cpu(topo.node_sample), cpu(topo.node_ref), cpu(topo.inner_src), cpu(topo.inner_tgt)))
    r, g = case.r, case.g
    geo = cpu(tape.get(_capi.TAPE_GEO)[:A].float())
    rbf = cpu(tape.get(_capi.TAPE_RBF)[:A].float())
    pp0, x1 = cpu(tape.get(_capi.TAPE_PP0).float()), cpu(tape.get(_capi.TAPE_X1).float())
    assert geo.shape == (A, 12) and rbf.shape[0] == A and rbf.shape[1] >= R and x1.shape == (N, 3) and pp0.shape[0] == N
    assert (geo[:, 11] == r.mask.astype(np.float32)).all()
    worst = {"x1": ratio32(x1, r.x1, g.x1, "x1"), "pp0": ratio32(np.ascontiguousarray(pp0.reshape(N, -1)[:, 0]), r.pp0, g.pp0, "pp0")}
    assert not pp0.reshape(N, -1)[:, 1:3].any()
    for k, (lo, hi) in dict(d=(0, 1), env=(1, 2), u=(2, 5), c=(5, 8), v=(8, 11)).items():
        worst["geo." + k] = ratio32(np.ascontiguousarray(geo[:, lo:hi]), r.geo[:, lo:hi], g.geo[:, lo:hi], "geo." + k)
    worst["rbf"] = ratio32(np.ascontiguousarray(rbf[:, :R]), r.rbf(means, betas), g.rbf(r, means, betas), "rbf")
    assert not rbf[:, R:].any()
    print(f"taped {name}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (name, bad)
