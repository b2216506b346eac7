"""The dense layer of the general-edge-list path ALONE (csrc/oard_general.hip: k_general_gemm_f64<RT> behind HipExec::gemm):
float64 MFMA tiles, float4 operand reads with a clamped K tail, gathered row segments, an XCD-swizzled block index, output tiles dealt
unevenly over waves, and the bias / SiLU / row scale / residual epilogue - per layer shape and for both row shapes (RT = 1 below 65 536
rows, RT = 2 from there), against a numpy float64 evaluation of the same float32 operands.  tests/general_dense/harness.hip includes the
product's translation unit and exports one function that fills an og::Gemm as og::dense does; this file compiles it once.

Gates.  With pre = sum_seg X_seg[idx_seg] W_seg^T + bias and S = sum |x||w| + |bias| in float64, and ref = the epilogue applied to pre in
float64:
  act = 0 (derived):  |y - ref| <= 2^-24 (|pre| + |pre scale| + |ref|) + 4 Ktot 2^-53 S - one half-ulp per float32 rounding the epilogue
      performs (the cast of the sum; the row scale; the residual add - a term the layer does not have drops out), plus the float64 sum in any
      order on both sides.  Row scale and a residual mode are never combined (the product never does; the compiler may contract them).
      With a row scale the cast's half-ulp is itself multiplied by the scale, so that layer's first term is |pre| max(1, |scale|): the
      epilogue's own statements evaluated in exactly rounded float32 on the float64 pre (numpy, no kernel involved) reach 1.14 times the
      three-term form on H_to_H_rowscale wherever |scale| > 1 meets two roundings of the same sign.  The form used stays below
      2^-24 (|pre| + 2 |pre scale|), the formula with all of its terms kept.
  act = 1: og::silu_f is float32 with the device's expf; its distance from a float64 SiLU is MEASURED on the plain-thread executor (og::Gemm
      itself, matrix_pipe = 0 through the same harness - the formulation the CPU suite pins on the reference's goldens, with the same
      epilogue statement for statement): ACT1_THREADS = max |y_threads - ref| / (2^-24 max(|pre|, |ref|)) over every act = 1 case of this
      file.  The matrix kernel's gate is that + 2: its float64 sum may land on the neighbouring float32 before SiLU.
No gate here is measured on the matrix kernel."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H, R, W = 196, 96, 684                                  # production widths: hidden, num_radial, the edge state (3 H + R)
U24, U53 = 2.0 ** -24, 2.0 ** -53
ACT1_THREADS = 3.55                                     # measured 3.5402 (H_to_W_silu_accumulate@65553): profiles/general_dense.txt
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # as oareactdiff_amd/build.py finds it
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    so = str(tmp_path_factory.mktemp("general_dense") / "libgeneral_dense.so")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-result",
                        os.path.join(HERE, "general_dense", "harness.hip"), "-o", so], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    L = C.CDLL(so)                                       # local symbol scope: the unit re-defines the oard_graph_* entry points
    fp, ip, i, vp = C.c_void_p, C.c_void_p, C.c_int, C.c_void_p
    L.general_dense_gemm.argtypes = [C.c_longlong, i, i] + [fp, i, i, ip] * 3 + [fp, i, fp, fp, i, i, i, fp, i, fp, i, vp]
    L.general_dense_gemm.restype = i
    return L


class Layer:
    """One dense call.  segs: (K, ld, table) per segment - ld = None: K; table = None: rows of x are the layer's rows, else x has `table`
    rows and the layer gathers them through int32 indices."""

    def __init__(self, name, rows, nout, segs, bias=True, act=0, mode=0, rowscale=False, ldy=None, ldw=None, xoff=0):
        self.name, self.rows, self.nout, self.bias, self.act, self.mode, self.rowscale = name, rows, nout, bias, act, mode, rowscale
        self.segs = [(s, None, None) if isinstance(s, int) else tuple(s) for s in segs]
        self.segs = [(k, k if ld is None else ld, tab) for k, ld, tab in self.segs]
        self.ktot = sum(k for k, _, _ in self.segs)
        self.ldy = nout + 3 if ldy is None else ldy
        self.ldw = self.ktot if ldw is None else ldw
        self.xoff = xoff                                  # floats by which segment 0's pointer is moved off its 16-byte boundary
        assert not (rowscale and mode), "never combined: see the module docstring"

    def at(self, rows):
        c = Layer.__new__(Layer)
        c.__dict__.update(self.__dict__)
        c.rows, c.name = rows, f"{self.name}@{rows}"
        return c


class Data:
    """The operands of a Layer (float32, from a seeded CPU generator) and their float64 reference; made once per case and not changed."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
        rows = c.rows
        self.c, self.x, self.idx = c, [], []
        for k, ld, tab in c.segs:
            x = torch.full((rows if tab is None else tab, ld), float("nan"))        # columns K .. ld are never to be read
            x[:, :k] = torch.randn(x.shape[0], k, generator=g)
            self.x.append(x)
            if tab is None:
                self.idx.append(None)
            else:
                assert tab != rows
                idx = torch.randint(0, tab, (rows,), generator=g, dtype=torch.int32)
                idx[int(torch.randint(0, max(rows - 1, 1), (1,), generator=g))] = 0
                idx[-1] = tab - 1
                self.idx.append(idx)
        self.w = torch.full((c.nout, c.ldw), float("nan"))
        self.w[:, :c.ktot] = torch.randn(c.nout, c.ktot, generator=g) / c.ktot ** 0.5
        self.b = torch.randn(c.nout, generator=g) if c.bias else None
        self.resid = torch.randn(rows, c.nout + 1, generator=g) if c.mode == 2 else None           # ldr = nout + 1
        self.scale = torch.randn(rows, generator=g) if c.rowscale else None
        self.y0 = torch.randn(rows, c.nout, generator=g) if c.mode == 1 else None
        self._ref = None

    def prefix(self, rows):
        """The same operands, the first `rows` rows of the layer only."""
        d = Data.__new__(Data)
        d.__dict__.update(self.__dict__)
        d.c, d._ref = self.c.at(rows), None
        d.x = [x if tab is not None else x[:rows] for x, (_, _, tab) in zip(self.x, self.c.segs)]
        d.idx = [None if i is None else i[:rows] for i in self.idx]
        d.resid, d.scale, d.y0 = (None if v is None else v[:rows] for v in (self.resid, self.scale, self.y0))
        return d

    def ref(self):
        """-> (ref, act-0 tolerance, act-1 unit), float64 [rows, nout]"""
        if self._ref is None:
            c = self.c
            pre = np.zeros((c.rows, c.nout)) + (self.b.double().numpy() if c.bias else 0.0)
            S = np.zeros((c.rows, c.nout)) + (self.b.double().abs().numpy() if c.bias else 0.0)
            wd, koff = self.w.double().numpy(), 0
            for (k, _, _), x, idx in zip(c.segs, self.x, self.idx):
                X = (x if idx is None else x[idx.long()])[:, :k].double().numpy()
                Wk = wd[:, koff:koff + k]
                pre += X @ Wk.T
                S += np.abs(X) @ np.abs(Wk).T
                koff += k
            v = pre / (1.0 + np.exp(-pre)) if c.act else pre
            tol = U24 * np.abs(pre)
            if c.rowscale:
                sc = self.scale.double().numpy()[:, None]
                v = v * sc
                tol = U24 * (np.abs(pre) * np.maximum(1.0, np.abs(sc)) + np.abs(v))        # the cast's half-ulp goes through the multiply
            ref = v
            if c.mode == 1:
                ref = self.y0.double().numpy() + v
            elif c.mode == 2:
                ref = self.resid.double().numpy()[:, :c.nout] + v
            if c.mode:
                tol += U24 * np.abs(ref)
            tol += 4.0 * c.ktot * U53 * S
            self._ref = (ref, tol, U24 * np.maximum(np.abs(pre), np.abs(ref)))
        return self._ref


def run(L, d, matrix_pipe=1):
    """One launch -> Y[:rows, :nout] on the host, after the write checks: guard columns and guard rows untouched, and (modes 0 and 2) every
    cell in range overwritten with a finite value."""
    c, dev = d.c, torch.device("cuda:0")
    keep = []

    def up(t):
        t = t.to(dev)
        keep.append(t)
        return t
    segargs = []
    for s in range(3):
        if s < len(c.segs):
            k, ld, _ = c.segs[s]
            x = d.x[s]
            if s == 0 and c.xoff:
                flat = up(torch.cat([torch.zeros(c.xoff), x.reshape(-1)]))
                xptr = flat.data_ptr() + 4 * c.xoff
            else:
                xptr = up(x.contiguous()).data_ptr()
            segargs += [xptr, ld, k, None if d.idx[s] is None else up(d.idx[s].contiguous()).data_ptr()]
        else:
            segargs += [None, 0, 0, None]
    Y = torch.full((c.rows + 2, c.ldy), SENTINEL)
    Y[:c.rows, :c.nout] = d.y0 if c.mode == 1 else float("nan")
    Y = up(Y)
    ptr = lambda t: None if t is None else up(t.contiguous()).data_ptr()
    rc = L.general_dense_gemm(c.rows, c.nout, len(c.segs), *segargs, ptr(d.w), c.ldw, ptr(d.b), Y.data_ptr(), c.ldy, c.act, c.mode,
                              ptr(d.resid), c.nout + 1, ptr(d.scale), matrix_pipe, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, (c.name, rc)
    torch.cuda.synchronize(dev)
    Y = Y.cpu()
    assert bool((Y[c.rows:] == SENTINEL).all()) and bool((Y[:, c.nout:] == SENTINEL).all()), f"{c.name}: a write outside rows x nout"
    y = Y[:c.rows, :c.nout]
    assert bool(torch.isfinite(y).all()), f"{c.name}: a cell in range was not written (or is not finite)"
    return y


def excess(y, d):
    """max over the layer of |y - ref| in units of its gate: the derived tolerance (act = 0), 2^-24 max(|pre|, |ref|) (act = 1)"""
    ref, tol, unit = d.ref()
    err = np.abs(y.double().numpy() - ref)
    return float((err / (unit if d.c.act else tol)).max())


def check(L, c, d=None):
    d = Data(c) if d is None else d
    y = run(L, d)
    e = excess(y, d)
    assert d.c.act == 0
    print(f"{c.name}: |y - ref| / gate = {e:.3f}")
    assert e <= 1.0, (c.name, e)
    return y


# ---- 1. row, output and block tails, RT = 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 147])
def test_row_output_and_block_tails(lib, rows):
    """nout = 1, 2: one ragged tile; 17, 20: a second, ragged tile; 65: five tiles = 3 + 2 over two waves; 196: 4 + 3 + 3 + 3 and outputs
    196..207 of the 13th tile masked; 272: 17 tiles = 5 wave groups, a second column block in which three waves leave at once; 588: three
    column blocks.  rows = 147 = 10 row blocks: 10, 20 and 30 workgroups, no multiple of 8, through the XCD swizzle."""
    for nout in (1, 2, 16, 17, 20, 65, 196, 272, 588):
        check(lib, Layer(f"tails_r{rows}_o{nout}", rows, nout, [20]))


def test_seven_blocks_under_one_swizzle_round(lib):
    """7 workgroups in a grid padded to 8: per = 1, one block per XCD and one XCD without work."""
    check(lib, Layer("tails_r100_o20", 100, 20, [20]))


# ---- 2. K tails and the two-buffer step loop ----------------------------------------------------------------------------------------------
def test_k_tails_and_step_counts(lib):
    """One, two, three and more 16-k steps, odd and even counts, every K % 16 in {0, 4, 8, 12}."""
    for K in (4, 8, 12, 16, 20, 32, 36, 52, 96, 196):
        check(lib, Layer(f"k{K}", 17, 20, [K]))


@pytest.mark.parametrize("split", [(4, 36, 12), (20, 16)])
def test_k_split_over_segments(lib, split):
    """torch.cat([...], dim=1) of two and three segments of unequal length, each with its own K tail and weight column offset: plain,
    gathered (tables longer and shorter than the layer), one segment with ld > K (the padding is NaN), and W with ldw > Ktot."""
    name = "seg" + "_".join(map(str, split))
    check(lib, Layer(name, 17, 20, list(split)))
    check(lib, Layer(name + "_gather", 17, 20, [(k, None, (29, 5, 23)[i]) for i, k in enumerate(split)]))
    check(lib, Layer(name + "_mixed", 17, 20, [(k, None, 9 if i == 1 else None) for i, k in enumerate(split)]))
    check(lib, Layer(name + "_ld", 17, 20, [(k, k + 8 if i == 0 else None, None) for i, k in enumerate(split)], ldw=sum(split) + 4))


# ---- 3. every dense layer the network runs on the matrix pipe, production widths -----------------------------------------------------------
ROWS = 147
GCL_EDGE = Layer("gcl_edge_2H+W_to_H_silu", ROWS, H, [(H, None, 50), (H, None, 50), W], act=1)
H_TO_W = Layer("H_to_W_silu_accumulate", ROWS, W, [H], act=1, mode=1)
PRODUCTION = [
    Layer("R_to_H_silu", ROWS, H, [R], act=1),
    Layer("H_to_H_rowscale", ROWS, H, [H], rowscale=True),
    Layer("H_to_H", ROWS, H, [H]),
    Layer("H_to_H_silu", ROWS, H, [H], act=1),
    GCL_EDGE,
    Layer("H_to_1_silu", ROWS, 1, [H], act=1, ldy=1),
    Layer("2H_to_H_silu", ROWS, H, [H, H], act=1),
    Layer("H_to_H_residual", ROWS, H, [H], mode=2),
    H_TO_W,
    Layer("H_to_3H", ROWS, 3 * H, [H], bias=False),
    Layer("R_to_3H", ROWS, 3 * H, [R], bias=False),
    Layer("W_to_3H_silu", ROWS, 3 * H, [W], act=1),
    Layer("3H_to_3H", ROWS, 3 * H, [3 * H]),
    Layer("H_to_2H_three_rows_per_node", 3 * ROWS, 2 * H, [H], bias=False),
    Layer("H_to_2", ROWS, 2, [H], ldy=2),
    Layer("H_to_9", ROWS, 9, [H], ldy=9),
]
BIG = 65553                                             # RT = 2; 65553 % 32 = 17: the last workgroup's second row tile holds one row
RT2_PRODUCTION = [GCL_EDGE.at(BIG), H_TO_W.at(BIG)]
ACT1_CASES = [c for c in PRODUCTION if c.act] + RT2_PRODUCTION


@pytest.fixture(scope="module")
def data():
    """Operands and float64 references shared by the tests of the production layers (made on first use, never changed)."""
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = Data(c)
        return cache[c.name]
    yield get
    cache.clear()


def _check_any(L, d, what="matrix pipe"):
    y = run(L, d)
    e = excess(y, d)
    if d.c.act:
        print(f"{d.c.name}: {what} |y - ref| / (2^-24 max(|pre|, |ref|)) = {e:.3f}   (gate {ACT1_THREADS} + 2)")
        assert e <= ACT1_THREADS + 2.0, (d.c.name, e)
    else:
        print(f"{d.c.name}: {what} |y - ref| / gate = {e:.3f}")
        assert e <= 1.0, (d.c.name, e)
    return y


@pytest.mark.parametrize("c", PRODUCTION, ids=lambda c: c.name)
def test_production_layers(lib, data, c):
    """One case per distinct dense(...) call of og::forward that runs on the matrix pipe, with its own segments and epilogue, on 147 rows
    (10 row blocks, the last with 3 rows)."""
    _check_any(lib, data(c))


def test_silu_layers_on_plain_threads_stay_under_the_measured_constant(lib, data):
    """Where ACT1_THREADS comes from, and that it still holds: og::Gemm on plain threads against the float64 SiLU, every act = 1 case."""
    worst = 0.0
    for c in ACT1_CASES:
        d = data(c)
        e = excess(run(lib, d, matrix_pipe=0), d)
        print(f"{c.name}: plain threads |y - ref| / (2^-24 max(|pre|, |ref|)) = {e:.4f}")
        worst = max(worst, e)
    print(f"ACT1_THREADS measured: {worst:.4f}")
    assert worst <= ACT1_THREADS


# ---- 4. layers that fall back to plain threads ------------------------------------------------------------------------------------------------
def test_layers_the_matrix_kernel_cannot_read_fall_back_to_plain_threads(lib):
    """K % 4 != 0 (the 3-column frame input, in_hidden + 1 = 9, H / 2 = 98), rows that are not 16-byte multiples, an operand off its 16-byte
    boundary: float4 reads are impossible, HipExec::gemm runs og::Gemm on plain threads.  Right within the derived gate, and - the
    fallback IS that executor - bit for bit what matrix_pipe = 0 gives."""
    cases = [Layer(f"fallback_k{K}", 17, 20, [K]) for K in (3, 6, 9, 98)]
    cases += [Layer("fallback_ld10", 17, 20, [(8, 10, None)]), Layer("fallback_seg1_k6", 17, 20, [16, 6]),
              Layer("fallback_xoff1", 17, 20, [16], xoff=1), Layer("fallback_ldw", 17, 20, [16], ldw=18)]
    for c in cases:
        d = Data(c)
        y = check(lib, c, d)
        assert torch.equal(y, run(lib, d, matrix_pipe=0)), c.name


# ---- 5. RT = 2 ----------------------------------------------------------------------------------------------------------------------------------
RT2_SMALL = [Layer("rt2_o20_k20", 65567, 20, [20]), Layer("rt2_o17_k36", 65567, 17, [36])]


@pytest.mark.parametrize("c", RT2_SMALL, ids=lambda c: c.name)
def test_two_row_tiles_per_wave(lib, c):
    """rows >= 65536: a wave owns 32 rows.  65536: every second tile full; 65537: a last workgroup with one row and an EMPTY second tile;
    65552: a first tile ending on the boundary, second empty; 65553: one row in the second tile; 65567: 15.  The operands of the shorter
    calls are the first rows of the longest one's."""
    whole = Data(c)
    for rows in (65536, 65537, 65552, 65553, 65567):
        d = whole.prefix(rows)
        check(lib, d.c, d)


@pytest.mark.parametrize("c", RT2_PRODUCTION, ids=lambda c: c.name)
def test_two_row_tiles_per_wave_production_widths(lib, data, c):
    """The two widest edge-level layers as the network runs them from 65 536 edges on: the GCL edge layer (two gathered segments and the
    684-wide edge state, 4 + 3 + 3 + 3 tiles) and H -> W accumulating into the edge state (43 tiles, three column blocks)."""
    _check_any(lib, data(c))


@pytest.mark.parametrize("c", RT2_SMALL + [GCL_EDGE], ids=lambda c: c.name)
def test_row_shape_does_not_change_a_single_bit(lib, data, c):
    """Every (row, output) accumulator receives the same MFMA sequence with the same operands whatever RT is: rows [0, 65535) of a
    65553-row call (RT = 2) equal those rows of a 65535-row call (RT = 1) on the same operands."""
    d = data(c.at(BIG))
    two, one = run(lib, d), run(lib, d.prefix(65535))
    assert one.shape[0] == 65535 and torch.equal(two[:65535], one)
