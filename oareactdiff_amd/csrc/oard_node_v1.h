// oard_node_v1.h — per-layer node stages, second generation.
//
// A workgroup of WAVES wavefronts owns 16 nodes (one MFMA column block).  Activations of those 16 nodes
// live in LDS as "vectors": block b (16 features x 16 nodes) = 1 KiB stored lane-linear, exactly the
// register block layout of oard_engine.h, so a B operand is one conflict-free ds_read_b128 and an output
// tile is one ds_write_b128.  The output tiles of every dense layer are dealt round-robin to the waves
// (tile t -> wave t % WAVES), the layers are separated by __syncthreads(), and the weights (A operand)
// come straight from L2 — every workgroup reads the same chunks, so they stay L2-resident.
// 276 workgroups x 8 waves at N = 4416 instead of 276 single waves.
#pragma once
#include "oard_kernels.h"

OARD_DEV f4 lds_blk(const float* v, int b, int lane) { return *reinterpret_cast<const f4*>(v + b * 256 + lane * 4); }
OARD_DEV void lds_st(float* v, int t, int lane, f4 x) { *reinterpret_cast<f4*>(v + t * 256 + lane * 4) = x; }

// one output tile from an LDS-resident input vector; even / odd K blocks on two accumulators.
// The weight chunks come straight from L2 (latency ~1 us): they are requested a whole group (<= 13 chunks,
// 52 VGPRs) at a time BEFORE the first MFMA of the group - left to itself the compiler keeps only two
// loads in flight and the tile costs one L2 round trip per chunk pair (measured: 5-6 us per tile instead of ~2).
#ifndef OARD_NODE_PF
#define OARD_NODE_PF 13
#endif
template <int KB>
OARD_DEV f4 dense_tile_lds(const float* __restrict__ wp, int t, const float* in, int lane, f4 init) {
    const float* base = wp + ((size_t)t * KB * 64 + lane) * 4;
    f4 c0 = init, c1 = f4zero();
    constexpr int G = OARD_NODE_PF;
#pragma unroll
    for (int b0 = 0; b0 < KB; b0 += G) {
        f4 a[G];
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (b0 + i < KB) a[i] = ld_f4(base + (size_t)(b0 + i) * 256);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (b0 + i < KB) {
                const f4 x = lds_blk(in, b0 + i, lane);
                if (i & 1) c1 = mma_chunk(a[i], x, c1);
                else c0 = mma_chunk(a[i], x, c0);
            }
    }
    return c0 + c1;
}

// A sequence of N output tiles, software-pipelined: the weight chunks of step s+1 (a step = up to 13 chunks of
// one tile) are requested before the MFMAs of step s are issued, so the L2 round trip of every step but the
// first hides behind the previous step's MFMAs.  job[j].w = first chunk of the tile (lane offset included by
// the callee), job[j].in = LDS input vector; acc[j] carries the initial value in and the result out.
struct TileJob {
    const float* w;
    const float* in;
};
template <int KB>
OARD_DEV TileJob tile_job(const float* __restrict__ wp, int t, const float* in) {
    return TileJob{wp + (size_t)t * KB * 256, in};
}
#ifndef OARD_NODE_SEQ_G
#define OARD_NODE_SEQ_G 7       // chunks per pipeline step
#endif
// k_node_pre_v1 / k_gcl_node_v1 have the registers for longer steps (84 / 94 of 128), but steps of 7 / 10 / 13 chunks measure the same
// (node stages 2.46 / 2.465 / 2.478 ms, profiles/round5_notes.txt section 3), and the step length fixes which chunks land in dense_seq's
// even / odd accumulators: 7 keeps the summation order the parity margins were measured with (config 1 under the default launch shapes:
// worst of 51 calls 9.05e-6 with 7, 1.03e-5 with 10, tolerance 1e-5)
#ifndef OARD_NODE_PRE_G
#define OARD_NODE_PRE_G 7
#endif
#ifndef OARD_GCL_NODE_G
#define OARD_GCL_NODE_G 7
#endif
// R = ring depth: the chunks of steps s+1 .. s+R-1 are in flight while step s issues its MFMAs ((R-1) x G x 4 VGPRs in flight,
// R x G x 4 held).  R = 2 is the node kernels' shape (register budget of 13-wave workgroups); the latency edge kernels use R = 4:
// with 7 chunks per step one step's MFMAs take ~0.4 us and an L2 round trip ~1.5 us, so three steps have to be in flight.
template <int KB, int N, int G = OARD_NODE_SEQ_G, int R = 2>
OARD_DEV void dense_seq(const TileJob (&job)[N], int lane, f4 (&acc)[N]) {
    constexpr int NG = (KB + G - 1) / G, S = N * NG;
    f4 a[R][G];
    f4 c1 = f4zero();
    auto fetch = [&](int st) {                                // st is a compile-time constant after unrolling
        const int j1 = st / NG, q1 = st % NG;
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (q1 * G + i < KB) a[st % R][i] = ld_f4(job[j1].w + (size_t)(q1 * G + i) * 256 + lane * 4);
    };
#pragma unroll
    for (int st = 0; st < R - 1; ++st)
        if (st < S) fetch(st);
#pragma unroll
    for (int st = 0; st < S; ++st) {
        const int j = st / NG, q = st % NG;
        if (st + R - 1 < S) fetch(st + R - 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (q * G + i < KB) {
                const f4 x = lds_blk(job[j].in, q * G + i, lane);
                if (i & 1) c1 = mma_chunk(a[st % R][i], x, c1);
                else acc[j] = mma_chunk(a[st % R][i], x, acc[j]);
            }
        if (q == NG - 1) { acc[j] += c1; c1 = f4zero(); }
    }
}
// The same pipeline for tiles whose weights are applied to THREE input vectors (the x, y, z components of `vec` under vec_proj /
// vec1_proj): job[j].in is the first input, the others follow at STRIDE floats; acc[3 j + k] belongs to input k.  Every weight
// chunk is fetched ONCE and feeds 3 x 4 MFMAs - as separate jobs the three components re-fetched the same chunks, and these stages
// are bound by the L2 round trips of their weight fetches, not by their MFMAs (round 5: 78 -> 26 chunk fetches per wave in
// k_equi_node_v1's vec_proj).
// The three B operands of a chunk are read by ONE volatile asm statement: written as plain LDS loads, hipcc moves the 3 x G reads of a
// step - and, where two jobs share their inputs, the second job's as well - to the top of the block and spills them (660 bytes per lane in
// k_equi_node_v1 at its 128-register cap; sched_barrier does not stop it, the motion happens before instruction scheduling).
template <int STRIDE>
OARD_DEV void lds_blk3(const float* in, int b, int lane, f4& x0, f4& x1, f4& x2) {
    const unsigned addr = (unsigned)(size_t)(in + b * 256 + lane * 4);          // LDS byte address = low half of the generic pointer
    static_assert(2 * STRIDE * 4 < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:%4\n\tds_read_b128 %2, %3 offset:%5\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(x0), "=&v"(x1), "=&v"(x2) : "v"(addr), "n"(STRIDE * 4), "n"(2 * STRIDE * 4) : "memory");
}
// ... and the MFMAs are volatile asm statements as well (accumulator in place): as builtins hipcc regroups the three chains of a chunk by
// accumulator - all chunks of x first, y and z operands parked in scratch meanwhile.  Volatile asm keeps program order.
// (The hazard recogniser does not know these statements are MFMAs: the leading s_nop covers "VALU writes a VGPR -> XDL reads it as SrcC"
// - hipcc zero-initialises an accumulator with v_mov right in front of its first MFMA; found as a 1e-3 error of dpos at H = 32.)
OARD_DEV void mma_chunk_pinned(f4 a, f4 b, f4& acc) {
    asm volatile("s_nop 1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %1, %5, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %2, %6, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %3, %7, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %4, %8, %0"
                 : "+v"(acc) : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w));
}
// The LAST chunk of a group of three chains: the z chain's four MFMAs, then - INSIDE the string, where neither the scheduler nor the
// register allocator can put anything - the wait states that an XDL result needs before anything but an accumulating MFMA may touch it
// (hipcc's hazard recogniser does not look inside asm statements, so nothing else would insert them).  The x and y accumulators are "+v"
// operands of this statement too: it is ordered behind their last MFMAs by data dependence, and every later reader of any of the three
// - VALU, a store, a spill - is ordered behind IT, hence behind the wait states.  (Round 5 had the s_nops in a separate statement that
// named no accumulator: hipcc was free to schedule a dependent add, copy or spill store in front of it.)
OARD_DEV void mma_chunk_pinned_last(f4 a, f4 b, f4& acc, f4& other0, f4& other1) {
    asm volatile("s_nop 1\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %3, %7, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %4, %8, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %5, %9, %0\n\t"
                 "v_mfma_f32_16x16x4_f32 %0, %6, %10, %0\n\t"
                 "s_nop 7\n\ts_nop 7\n\ts_nop 3"
                 : "+v"(acc), "+v"(other0), "+v"(other1)
                 : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w));
}
constexpr int last_chunk_at(int kb, int g, int parity) {         // last chunk of a job whose position inside its pipeline step has this parity
    int r = -1;
    for (int ch = 0; ch < kb; ++ch)
        if (((ch % g) & 1) == parity) r = ch;
    return r;
}
// SPLIT: even / odd chunks of a pipeline step on two accumulators per input, added at the end of the tile - dense_seq's summation order
// (bit-identical to the three separate jobs this replaced); used where the registers allow it, the single chain elsewhere.
template <int KB, int N, int STRIDE, int G = OARD_NODE_SEQ_G, bool SPLIT = false, int R = 2>
OARD_DEV void dense_seq_xyz(const TileJob (&job)[N], int lane, f4 (&acc)[N * 3]) {
    constexpr int NG = (KB + G - 1) / G, S = N * NG;
    f4 a[R][G];
    f4 c1[SPLIT ? 3 : 1];
#pragma unroll
    for (int k = 0; k < (SPLIT ? 3 : 1); ++k) c1[k] = f4zero();
    auto fetch = [&](int st) {
        const int j1 = st / NG, q1 = st % NG;
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (q1 * G + i < KB) a[st % R][i] = ld_f4(job[j1].w + (size_t)(q1 * G + i) * 256 + lane * 4);
    };
#pragma unroll
    for (int st = 0; st < R - 1; ++st)
        if (st < S) fetch(st);
    // The chunk that ends a job's chains carries the wait states (mma_chunk_pinned_last).  With SPLIT a job has two groups of chains, on
    // acc (even positions of a pipeline step) and on c1 (odd positions): each group's last chunk is marked, so both are settled when
    // `acc += c1` reads them.
    constexpr int LAST_EVEN = SPLIT ? last_chunk_at(KB, G, 0) : KB - 1;
    constexpr int LAST_ODD = SPLIT ? last_chunk_at(KB, G, 1) : -1;
#pragma unroll
    for (int st = 0; st < S; ++st) {
        const int j = st / NG, q = st % NG;
        if (st + R - 1 < S) fetch(st + R - 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (q * G + i < KB) {
                const int ch = q * G + i;
                const bool last = ch == LAST_EVEN || ch == LAST_ODD;
                f4 x0, x1, x2;
                lds_blk3<STRIDE>(job[j].in, ch, lane, x0, x1, x2);
                if (SPLIT && (i & 1)) {
                    mma_chunk_pinned(a[st % R][i], x0, c1[0]);
                    mma_chunk_pinned(a[st % R][i], x1, c1[SPLIT ? 1 : 0]);
                    if (last) mma_chunk_pinned_last(a[st % R][i], x2, c1[SPLIT ? 2 : 0], c1[0], c1[SPLIT ? 1 : 0]);
                    else mma_chunk_pinned(a[st % R][i], x2, c1[SPLIT ? 2 : 0]);
                } else {
                    mma_chunk_pinned(a[st % R][i], x0, acc[3 * j + 0]);
                    mma_chunk_pinned(a[st % R][i], x1, acc[3 * j + 1]);
                    if (last) mma_chunk_pinned_last(a[st % R][i], x2, acc[3 * j + 2], acc[3 * j + 0], acc[3 * j + 1]);
                    else mma_chunk_pinned(a[st % R][i], x2, acc[3 * j + 2]);
                }
            }
        if (SPLIT && q == NG - 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { acc[3 * j + k] += c1[k]; c1[k] = f4zero(); }
        }
    }
}
// LayerNorm statistics of an LDS vector (every wave computes them redundantly)
template <int HT, int H>
OARD_DEV void ln_stats_lds(const float* v, int lane, float& mean, float& rstd) {
    const int g = lane >> 4;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        const f4 x = lds_blk(v, t, lane);
        const int f0 = 16 * t + 4 * g;
        s += (f0 + 0 < H ? x.x : 0.f) + (f0 + 1 < H ? x.y : 0.f) + (f0 + 2 < H ? x.z : 0.f) + (f0 + 3 < H ? x.w : 0.f);
    }
    mean = col_reduce(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < HT; ++t) {
        const f4 x = lds_blk(v, t, lane);
        const int f0 = 16 * t + 4 * g;
        const float dx = x.x - mean, dy = x.y - mean, dz = x.z - mean, dw = x.w - mean;
        q += (f0 + 0 < H ? dx * dx : 0.f) + (f0 + 1 < H ? dy * dy : 0.f) + (f0 + 2 < H ? dz * dz : 0.f) +
             (f0 + 3 < H ? dw * dw : 0.f);
    }
    rstd = 1.0f / sqrtf(col_reduce(q) * (1.0f / H) + 1e-5f);
}
template <int H>
OARD_DEV f4 ln_apply(f4 x, float mean, float rstd, const float* gamma, const float* beta, int t, int lane) {
    const int f0 = 16 * t + 4 * (lane >> 4);
    f4 y = (x - mean) * rstd * ld_vec(gamma, t, lane) + ld_vec(beta, t, lane);
    y.x = f0 + 0 < H ? y.x : 0.f; y.y = f0 + 1 < H ? y.y : 0.f; y.z = f0 + 2 < H ? y.z : 0.f; y.w = f0 + 3 < H ? y.w : 0.f;
    return y;
}

struct NodeBlk {
    int lane, wave, g, n;
    bool valid;
};
// npb = real nodes per workgroup (<= 16; TopoDev::npb, chosen by the host): fewer than 16 leaves MFMA columns
// empty but multiplies the number of workgroups, which is what these latency-bound stages need on small
// batches (at B = 1 sixteen nodes per workgroup would put the whole layer on 5 CUs)
OARD_DEV NodeBlk node_blk(int N, int npb) {
    NodeBlk b;
    b.lane = threadIdx.x & 63; b.wave = threadIdx.x >> 6; b.g = b.lane >> 4;
    const int c = blockIdx.x * npb + (b.lane & 15);
    b.valid = (b.lane & 15) < npb && c < N;
    b.n = b.valid ? c : N - 1;
    return b;
}

// Small batches (npb <= 4 real nodes per workgroup): the 16 MFMA columns of a wave are mostly padding, and a gather that walks a
// node's rows two or eight at a time is a chain of dependent L2 / HBM round trips (B = 1: eleven steps of ~1.8 us in
// k_equi_node_v1).  There the 16 columns are dealt to the ROWS instead: node i of the workgroup owns the L = 16 >> ceil(log2 npb)
// lanes e = i L .. i L + L - 1 of every 16-lane group, lane slot e % L takes rows slot, slot + L, ... of its node, a butterfly
// adds the L partial sums and column i fetches the total from lane i L.  22 rows then take one or two steps instead of eleven.
struct RowLanes {
    int L, npb, node, slot; // lanes per node, nodes per workgroup, node (column) this lane works for, its slot among the node's lanes
    bool live;              // this lane's node exists
};
OARD_DEV RowLanes row_lanes(int N, int npb, int lane) {
    RowLanes r;
    r.L = npb == 1 ? 16 : (npb == 2 ? 8 : 4); r.npb = npb;
    const int e = lane & 15;
    r.node = e / r.L; r.slot = e % r.L;
    r.live = r.node < npb && blockIdx.x * npb + r.node < N;
    return r;
}
OARD_DEV float rows_total(float x, const RowLanes& r, int lane) {          // sum over the node's lanes, delivered to column `node`
    for (int d = 1; d < r.L; d <<= 1) x += __shfl_xor(x, d, 64);
    const int e = lane & 15;
    return __shfl(x, (lane & 48) | ((e < r.npb ? e : 0) * r.L), 64);        // column e < npb reads lane e L of its 16-lane group
}
OARD_DEV f4 rows_total4(f4 v, const RowLanes& r, int lane) {
    return (f4){rows_total(v.x, r, lane), rows_total(v.y, r, lane), rows_total(v.z, r, lane), rows_total(v.w, r, lane)};
}

// =====================================================================================================
// s += pos_expansion(pos_prjt);  xh = LN_gcl(s);  P = W1a xh + b1;  Q = W1b xh      (see k_node_pre)
// =====================================================================================================
template <class D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_node_pre_v1(TopoDev tp, const float* __restrict__ wb, PackOff po,
                                                            LayerOff lo, const float* __restrict__ s,
                                                            const float* __restrict__ pp0, float* __restrict__ xh,
                                                            float* __restrict__ P, float* __restrict__ Q) {
    __shared__ __attribute__((aligned(16))) float sm[(D::PB + 2 * D::HT) * 256];
    float* hid = sm;                      // [PB]
    float* sv = sm + D::PB * 256;         // [HT]
    float* xv = sv + D::HT * 256;         // [HT]
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    const float pp = pp0[nb.n];
    for (int b = nb.wave; b < D::PB; b += WAVES) {
        const int k0 = 16 * b + 4 * nb.g;
        const float* w = wb + po.pe0;
        f4 h;
        h.x = k0 + 0 < D::H2 ? silu1(w[(k0 + 0) * 3] * pp) : 0.f;
        h.y = k0 + 1 < D::H2 ? silu1(w[(k0 + 1) * 3] * pp) : 0.f;
        h.z = k0 + 2 < D::H2 ? silu1(w[(k0 + 2) * 3] * pp) : 0.f;
        h.w = k0 + 3 < D::H2 ? silu1(w[(k0 + 3) * 3] * pp) : 0.f;
        lds_st(hid, b, nb.lane, h);
    }
    __syncthreads();
    constexpr int TPW = (D::HT + WAVES - 1) / WAVES, TPW2 = (2 * D::HT + WAVES - 1) / WAVES;
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = min(nb.wave + i * WAVES, D::HT - 1);
            job[i] = tile_job<D::PB>(wb + po.pe1, t, hid);
            acc[i] = f4zero();
        }
        dense_seq<D::PB, TPW, OARD_NODE_PRE_G>(job, nb.lane, acc);
        // s + pos_expansion(.): the product is summed on its own and added to s ONCE, as `s = s + mlp(pos_prjt)` does (leftnet.py:840-841).
        // Rounds 1-5 started the chain AT s: ~100 small terms, each rounded at the magnitude of s - the one stage of the forward whose
        // error sat above plain torch float32's (tools/stage_error.py: 4.5e-7 against 1.6e-7 per layer; it is what made the node state's
        // error grow to 1.3e-6 over the six layers and config 1's worst call read 5e-6 ... 9e-6)
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < D::HT)
                lds_st(sv, nb.wave + i * WAVES, nb.lane, ld_blk(s, nb.n, D::HP, nb.wave + i * WAVES, nb.lane) + acc[i]);
    }
    __syncthreads();
    float mean, rstd;
    ln_stats_lds<D::HT, D::H>(sv, nb.lane, mean, rstd);
    for (int t = nb.wave; t < D::HT; t += WAVES) {
        const f4 y = ln_apply<D::H>(lds_blk(sv, t, nb.lane), mean, rstd, wb + lo.ln_g_w, wb + lo.ln_g_b, t, nb.lane);
        lds_st(xv, t, nb.lane, y);
        if (nb.valid) st_blk(xh, nb.n, D::HP, t, nb.lane, y);
    }
    __syncthreads();
    {
        TileJob job[TPW2];
        f4 acc[TPW2];
#pragma unroll
        for (int i = 0; i < TPW2; ++i) {
            const int t = min(nb.wave + i * WAVES, 2 * D::HT - 1);
            job[i] = t < D::HT ? tile_job<D::HT>(wb + lo.W1a, t, xv) : tile_job<D::HT>(wb + lo.W1b, t - D::HT, xv);
            acc[i] = t < D::HT ? ld_vec(wb + lo.b1, t, nb.lane) : f4zero();
        }
        dense_seq<D::HT, TPW2, OARD_NODE_PRE_G>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW2; ++i) {
            const int t = nb.wave + i * WAVES;
            if (t < 2 * D::HT && nb.valid) {
                if (t < D::HT) st_blk(P, nb.n, D::HP, t, nb.lane, acc[i]);
                else st_blk(Q, nb.n, D::HP, t - D::HT, nb.lane, acc[i]);
            }
        }
    }
}

// =====================================================================================================
// agg = mean_e m_e;  s = xh + node_mlp([xh, agg]);  xq = x_proj(LN_msg(s))           (see k_gcl_node)
// =====================================================================================================
// ROWS: the small-batch gather (row_lanes, <= 4 nodes per workgroup) - its own instantiation, chosen at launch
// MSUM (large batches only): `mbuf` is msum, the per-node partial sums the MSUM edge kernels left (oard_edge_v1.h, st_msum) - one at the
//   first column of each of the node's two column ranges (TopoDev::node_cols) and one at every multiple of 16 strictly inside a range,
//   where a wave tile cut the node's segment.  They are added in ascending column order, inner range first: ~6 rows per node instead of
//   one per edge.  Its own instantiation, the others stay what they are.
template <class D, int WAVES, bool ROWS = false, bool MSUM = false>
__global__ __launch_bounds__(WAVES * 64) void k_gcl_node_v1(TopoDev tp, const float* __restrict__ wb, LayerOff lo,
                                                            const float* __restrict__ xh, const float* __restrict__ mbuf,
                                                            float* __restrict__ s, float* __restrict__ xq,
                                                            float* __restrict__ agg_out /* training tape, or NULL */) {
    static_assert(!(MSUM && ROWS), "the partial sums exist for the large-batch gather only");
    __shared__ __attribute__((aligned(16))) float sm[4 * D::HT * 256];
    float* in = sm;                        // [2 HT]: xh | agg      (later: xln | hq)
    float* hm = sm + 2 * D::HT * 256;      // [HT]
    float* sv = sm + 3 * D::HT * 256;      // [HT]
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    const int smp = tp.node_sample[nb.n];
    const int deg = nb.valid ? tp.sample_ptr[smp + 1] - tp.sample_ptr[smp] - 1 : 0;
    const size_t e0 = (size_t)tp.edge_ptr[nb.n];
    const int mx = wave_max(deg);
    const float inv = 1.0f / (float)max(deg, 1);
    // MSUM: partial k of the node = column pc(k); n_in of them in the inner range, cnt in all
    int in_lo = 0, x_lo = 0, n_in = 0, cnt = 0;
    if (MSUM) {
        const int* nc = tp.node_cols + 4 * (size_t)nb.n;
        const int in_hi = nc[1], x_hi = nc[3];
        in_lo = nc[0]; x_lo = nc[2];
        n_in = (nb.valid && in_hi > in_lo) ? 1 + ((in_hi - 1) >> 4) - (in_lo >> 4) : 0;
        cnt = n_in + ((nb.valid && x_hi > x_lo) ? 1 + ((x_hi - 1) >> 4) - (x_lo >> 4) : 0);
    }
    auto pc = [&](int k) -> size_t {
        const int lo = k < n_in ? in_lo : x_lo, j = k < n_in ? k : k - n_in;
        return (size_t)(j == 0 ? lo : ((lo >> 4) + j) << 4);
    };
    const int mxp = MSUM ? wave_max(cnt) : 0;
    for (int t = nb.wave; t < D::HT; t += WAVES) {
        lds_st(in, t, nb.lane, ld_blk(xh, nb.n, D::HP, t, nb.lane));
        f4 a0 = f4zero(), a1 = f4zero();
        if (ROWS) {                                             // small batches: the wave's columns walk the rows (row_lanes)
            const RowLanes rl = row_lanes(tp.N, tp.npb, nb.lane);
            const int nn = min(blockIdx.x * tp.npb + rl.node, tp.N - 1);
            const int smp2 = tp.node_sample[nn];
            const int deg2 = rl.live ? tp.sample_ptr[smp2 + 1] - tp.sample_ptr[smp2] - 1 : 0;
            const size_t e2 = (size_t)tp.edge_ptr[nn];
            const int mx2 = wave_max(deg2), last2 = max(deg2 - 1, 0);
            for (int k = 0; k < mx2; k += 2 * rl.L) {
                const int k0 = k + rl.slot, k1 = k0 + rl.L;
                const f4 r0 = ld_blk(mbuf, e2 + min(k0, last2), D::HP, t, nb.lane), r1 = ld_blk(mbuf, e2 + min(k1, last2), D::HP, t, nb.lane);
                if (k0 < deg2) a0 += r0;
                if (k1 < deg2) a1 += r1;
            }
            a0 = rows_total4(a0 + a1, rl, nb.lane);
            a1 = f4zero();
        }
        // 8 message rows in flight per step (branch-free: out-of-range slots re-read the last row with weight 0)
        const int last = max(deg - 1, 0);
        for (int k = 0; MSUM && k < mxp; k += 8) {            // 8 partial rows in flight (slots past the end re-read the last one with weight 0)
            f4 r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = ld_blk(mbuf, pc(min(k + i, max(cnt - 1, 0))), D::HP, t, nb.lane);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f4 v = k + i < cnt ? r[i] : f4zero();
                if (i & 1) a1 += v; else a0 += v;
            }
        }
        for (int k = 0; !ROWS && !MSUM && k < mx; k += 8) {
            f4 r[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = ld_blk(mbuf, e0 + min(k + i, last), D::HP, t, nb.lane);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f4 v = k + i < deg ? r[i] : f4zero();
                if (i & 1) a1 += v; else a0 += v;
            }
        }
        lds_st(in, D::HT + t, nb.lane, (a0 + a1) * inv);
        if (agg_out != nullptr && nb.valid) st_blk(agg_out, nb.n, D::HP, t, nb.lane, (a0 + a1) * inv);
    }
    __syncthreads();
    constexpr int TPW = (D::HT + WAVES - 1) / WAVES, TPW3 = (3 * D::HT + WAVES - 1) / WAVES;
    int tw[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) tw[i] = min(nb.wave + i * WAVES, D::HT - 1);
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) { job[i] = tile_job<2 * D::HT>(wb + lo.nm0, tw[i], in); acc[i] = ld_vec(wb + lo.nm0b, tw[i], nb.lane); }
        dense_seq<2 * D::HT, TPW, OARD_GCL_NODE_G>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < D::HT) lds_st(hm, tw[i], nb.lane, silu4(acc[i]));
    }
    __syncthreads();
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) { job[i] = tile_job<D::HT>(wb + lo.nm1, tw[i], hm); acc[i] = ld_vec(wb + lo.nm1b, tw[i], nb.lane); }
        dense_seq<D::HT, TPW, OARD_GCL_NODE_G>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < D::HT) {
                const f4 v = lds_blk(in, tw[i], nb.lane) + acc[i];
                lds_st(sv, tw[i], nb.lane, v);
                if (nb.valid) st_blk(s, nb.n, D::HP, tw[i], nb.lane, v);
            }
    }
    __syncthreads();
    float mean, rstd;
    ln_stats_lds<D::HT, D::H>(sv, nb.lane, mean, rstd);
    float* xln = in;                       // safe: `in` is no longer read after the barrier above
    float* hq = in + D::HT * 256;
    for (int t = nb.wave; t < D::HT; t += WAVES)
        lds_st(xln, t, nb.lane, ln_apply<D::H>(lds_blk(sv, t, nb.lane), mean, rstd, wb + lo.ln_q_w, wb + lo.ln_q_b, t, nb.lane));
    __syncthreads();
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) { job[i] = tile_job<D::HT>(wb + lo.xp0, tw[i], xln); acc[i] = f4zero(); }
        dense_seq<D::HT, TPW, OARD_GCL_NODE_G>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < D::HT) lds_st(hq, tw[i], nb.lane, silu4(acc[i]));
    }
    __syncthreads();
    {
        TileJob job[TPW3];
        f4 acc[TPW3];
#pragma unroll
        for (int i = 0; i < TPW3; ++i) {
            job[i] = tile_job<D::HT>(wb + lo.xp2, min(nb.wave + i * WAVES, 3 * D::HT - 1), hq);
            acc[i] = f4zero();
        }
        dense_seq<D::HT, TPW3, OARD_GCL_NODE_G>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW3; ++i)
            if (nb.wave + i * WAVES < 3 * D::HT && nb.valid) st_blk(xq, nb.n, 3 * D::HP, nb.wave + i * WAVES, nb.lane, acc[i]);
    }
}

// EquiUpdate's frame-scalar MLP (Linear(3,48) SiLU Linear(48,8) SiLU Linear(8,1) on (x, 0, 0), see lin3u) for the
// four features of a lane at once, first two layers from an LDS copy laid out per hidden unit k as
// [w2[0..7][k], w0[k][0], b0[k], -, -] (12 floats): three broadcast LDS reads per k instead of ten dependent
// scalar loads per k and per value
OARD_DEV void lin3u_stage(const float* __restrict__ p, float* l3s, int tid, int nthreads) {
    for (int i = tid; i < 48 * 12; i += nthreads) {
        const int k = i / 12, j = i % 12;
        l3s[i] = j < 8 ? p[192 + j * 48 + k] : (j == 8 ? p[3 * k] : (j == 9 ? p[144 + k] : 0.f));
    }
}
OARD_DEV f4 lin3u4(const float* l3s, const float* __restrict__ p, f4 x) {
    const float* b2 = p + 576;
    const float* w4 = p + 584;
    f4 h2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h2[j] = (f4){b2[j], b2[j], b2[j], b2[j]};
#pragma unroll 4
    for (int k = 0; k < 48; ++k) {
        const f4 wa = *reinterpret_cast<const f4*>(l3s + 12 * k), wc = *reinterpret_cast<const f4*>(l3s + 12 * k + 4);
        const float w0 = l3s[12 * k + 8], b0 = l3s[12 * k + 9];
        const f4 h = silu4(x * w0 + b0);
        h2[0] += h * wa.x; h2[1] += h * wa.y; h2[2] += h * wa.z; h2[3] += h * wa.w;
        h2[4] += h * wc.x; h2[5] += h * wc.y; h2[6] += h * wc.z; h2[7] += h * wc.w;
    }
    const float b4 = p[592];
    f4 o = (f4){b4, b4, b4, b4};
#pragma unroll
    for (int j = 0; j < 8; ++j) o += silu4(h2[j]) * w4[j];
    return o;
}

// the same MLP for one value per lane (small batches: with <= 4 real nodes per workgroup a 16 x 16 tile holds at
// most 64 real values, one per lane, instead of four per lane of which most belong to padding columns)
OARD_DEV float lin3u1(const float* l3s, const float* __restrict__ p, float x) {
    const float* b2 = p + 576;
    const float* w4 = p + 584;
    float h2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h2[j] = b2[j];
#pragma unroll 4
    for (int k = 0; k < 48; ++k) {
        const f4 wa = *reinterpret_cast<const f4*>(l3s + 12 * k), wc = *reinterpret_cast<const f4*>(l3s + 12 * k + 4);
        const float h = silu1(x * l3s[12 * k + 8] + l3s[12 * k + 9]);
        h2[0] += h * wa.x; h2[1] += h * wa.y; h2[2] += h * wa.z; h2[3] += h * wa.w;
        h2[4] += h * wc.x; h2[5] += h * wc.y; h2[6] += h * wc.z; h2[7] += h * wc.w;
    }
    float o = p[592];
#pragma unroll
    for (int j = 0; j < 8; ++j) o += silu1(h2[j]) * w4[j];
    return o;
}

// =====================================================================================================
// EquiMessage node side + EquiUpdate, fused (see k_equi_agg_v1 / k_equi_upd):
//   messages from q, aggregation, s = (s + dx)/sqrt2, vec += dvec, vec_proj, frame scalar MLP,
//   xvec_proj, s += (a + b + vdot)/sqrt2, vec += c * vec2.        vec_in != vec_out.
// =====================================================================================================
// XC: reflect_equiv = False - the message carries x (x) coord_cross as well (leftnet.py:268-272); its own instantiation, so
// that the production kernel's register budget is untouched
// D = Layer0<Dims<...>> (large-batch gather only): layer 0 of an inference forward.  The vector state entering it is exactly zero, so
// vec[src] * a2 adds nothing and the edge kernel has not written the middle third of q (k_equi_edge_v1, skip_mid): neither that third of
// q and of xq[src] nor vec_in[src] is loaded.  A zero takes their place in the unchanged expressions, so the sums are the same bit for
// bit (up to the sign of an exact zero) however the compiler contracts the products.  Its own instantiation, selected through the
// dimensions type: the instantiations of the other layers keep their names and their register budget (36 bytes of scratch at the
// 128-register cap; a run-time flag costs 8 more, and loads from scratch inside the gather loop).
template <class D> struct Layer0 : D {};
template <class D> struct is_layer0 { static constexpr bool value = false; };
template <class D> struct is_layer0<Layer0<D> > { static constexpr bool value = true; };
template <class D, int WAVES, bool ROWS = false, bool XC = false>
__global__ __launch_bounds__(WAVES * 64) void k_equi_node_v1(TopoDev tp, const float* __restrict__ wb, LayerOff lo,
                                                             const float* __restrict__ qbuf, const float* __restrict__ xq,
                                                             const float* __restrict__ geo, const float* __restrict__ x1,
                                                             const float* s, float* s_out, const float* __restrict__ vec_in,
                                                             float* __restrict__ vec_out,
                                                             float* __restrict__ sa_out, float* __restrict__ va_out /* training tape: state after the aggregation, or NULL */,
                                                             ActList al /* inner rows inside the cutoff: the gather walks this list (NULL: every row) */) {
    constexpr bool L0 = is_layer0<D>::value;
    static_assert(!(L0 && ROWS), "the layer-0 form exists for the large-batch gather only");
    // s: scalar state entering the stage (s_mid), s_out: the state leaving it - the same buffer in inference (every element is read and
    // later written by the same lane), the tape slots s_mid[l] / s_in[l + 1] in training
    constexpr int HT = D::HT;
    constexpr int TPW = (HT + WAVES - 1) / WAVES;            // tiles owned per wave (upper bound)
    __shared__ __attribute__((aligned(16))) float sm[6 * HT * 256 + 48 * 12 + L3T_FLOATS];
    float* l3s = sm + 6 * HT * 256;        // frame-scalar MLP weights (lin3u_stage)
    float* l3t = l3s + 48 * 12;            // ... and its table (round 5: L3T_* in oard_layout.h; staged only when its flag is set)
#ifdef OARD_NO_L3T                        // A/B build: always the MLP itself
    const bool l3t_ok = false;
#else
    const bool l3t_ok = tp.npb > 4 && (wb + lo.l3t)[2 * (L3T_N + 1)] > 0.5f;          // uniform
#endif
    if (l3t_ok)
        for (int i = threadIdx.x; i < 2 * (L3T_N + 1) / 4; i += WAVES * 64)
            reinterpret_cast<f4*>(l3t)[i] = ld_f4(wb + lo.l3t + 4 * i);
    if (l3t_ok && threadIdx.x < 2) l3t[2 * (L3T_N + 1) - 2 + threadIdx.x] = (wb + lo.l3t)[2 * (L3T_N + 1) - 2 + threadIdx.x];
#ifdef OARD_TIMELINE
    const bool tl_on_ = blockIdx.x == gridDim.x / 2 && (threadIdx.x & 63) == 0; int tl_n_ = 0;
#endif
    TL(1);
    lin3u_stage(wb + lo.l3u, l3s, threadIdx.x, WAVES * 64);        // visible after the first barrier below
    float* vx = sm;                        // [3][HT] updated vec
    float* in = sm + 3 * HT * 256;         // [2 HT]: s_mid | scal
    float* hx = sm + 5 * HT * 256;         // [HT]
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    // list entries [a0, a0 + cnt) belong to node n: with an ActList the entries are (row, source) pairs of the edges inside the cutoff, in
    // row order; without, entry k IS row k
    // (while nothing is masked - n_act == A, the usual case - the list is the identity: one uniform test, and the gather keeps the
    // direct addressing it had before the list existed; the extra level of indexing cost 2 % of the node stages)
    const int n = nb.n;
    const bool listed = al.pre != nullptr && (long long)__builtin_amdgcn_readfirstlane(*al.n) != tp.A;
    const int a0 = listed ? al.pre[tp.act_ptr[n]] : tp.act_ptr[n];
    const int cnt = nb.valid ? (listed ? al.pre[tp.act_ptr[n + 1]] : tp.act_ptr[n + 1]) - a0 : 0;
    const int mx = wave_max(cnt);
    auto row_of = [&](int k) -> int { return listed ? al.rows[k] : k; };
    auto src_of = [&](int k) -> int { return listed ? al.src[k] : tp.act_src[k]; };
    const float inv_sqrt2 = 0.70710678118654752f, inv_sqrt3 = 0.57735026918962576f,
                inv_sqrt_h = 1.0f / sqrtf((float)D::H);

    // 1. messages + aggregation for the tiles this wave owns
    for (int t = nb.wave; t < HT; t += WAVES) {
        f4 dx = f4zero(), v0 = f4zero(), v1 = f4zero(), v2 = f4zero();
        const f4 xn0 = ld_blk(xq, n, 3 * D::HP, t, nb.lane), xn1 = ld_blk(xq, n, 3 * D::HP, HT + t, nb.lane),
                 xn2 = ld_blk(xq, n, 3 * D::HP, 2 * HT + t, nb.lane);
        const int a_hi = (int)max(tp.A - 1, 0LL);
        if (ROWS) {                                             // small batches: the wave's columns walk the edges (row_lanes)
            const RowLanes rl = row_lanes(tp.N, tp.npb, nb.lane);
            const int nn = min(blockIdx.x * tp.npb + rl.node, tp.N - 1);
            const int b0 = listed ? al.pre[tp.act_ptr[nn]] : tp.act_ptr[nn];
            const int cnt2 = rl.live ? (listed ? al.pre[tp.act_ptr[nn + 1]] : tp.act_ptr[nn + 1]) - b0 : 0;
            const int mx2 = wave_max(cnt2);
            const f4 zn0 = ld_blk(xq, nn, 3 * D::HP, t, nb.lane), zn1 = ld_blk(xq, nn, 3 * D::HP, HT + t, nb.lane),
                     zn2 = ld_blk(xq, nn, 3 * D::HP, 2 * HT + t, nb.lane);
            for (int k = 0; k < mx2; k += rl.L) {
                const int kk = k + rl.slot;
                const int ke = min(b0 + min(kk, max(cnt2 - 1, 0)), a_hi);      // list entry (clamped: discarded when kk >= cnt2)
                const size_t a = cnt2 > 0 ? (size_t)row_of(ke) : 0;
                const int m = cnt2 > 0 ? src_of(ke) : 0;
                const float* gp = geo + a * GEO_STRIDE;
                const float gx = gp[2], gy = gp[3], gz = gp[4];
                const float cx = XC ? gp[5] : 0.f, cy = XC ? gp[6] : 0.f, cz = XC ? gp[7] : 0.f;
                const f4 q0 = ld_blk(qbuf, a, 3 * D::HP, t, nb.lane), q1 = ld_blk(qbuf, a, 3 * D::HP, HT + t, nb.lane),
                         q2 = ld_blk(qbuf, a, 3 * D::HP, 2 * HT + t, nb.lane);
                const f4 y0 = ld_blk(xq, m, 3 * D::HP, t, nb.lane), y1 = ld_blk(xq, m, 3 * D::HP, HT + t, nb.lane),
                         y2 = ld_blk(xq, m, 3 * D::HP, 2 * HT + t, nb.lane);
                const f4 w0 = ld_blk(vec_in, (size_t)m * 3 + 0, D::HP, t, nb.lane), w1 = ld_blk(vec_in, (size_t)m * 3 + 1, D::HP, t, nb.lane),
                         w2 = ld_blk(vec_in, (size_t)m * 3 + 2, D::HP, t, nb.lane);
                if (kk < cnt2) {
                    const f4 xm = (y0 + zn0) * q0;
                    dx += xm;
                    const f4 a2 = (y1 + zn1) * q1 * inv_sqrt3;
                    const f4 a3 = (y2 + zn2) * q2;
                    v0 += (XC ? w0 * a2 + a3 * gx + xm * cx : w0 * a2 + a3 * gx) * inv_sqrt_h;
                    v1 += (XC ? w1 * a2 + a3 * gy + xm * cy : w1 * a2 + a3 * gy) * inv_sqrt_h;
                    v2 += (XC ? w2 * a2 + a3 * gz + xm * cz : w2 * a2 + a3 * gz) * inv_sqrt_h;
                }
            }
            dx = rows_total4(dx, rl, nb.lane); v0 = rows_total4(v0, rl, nb.lane);
            v1 = rows_total4(v1, rl, nb.lane); v2 = rows_total4(v2, rl, nb.lane);
        }
        // two edges in flight per step, branch-free (out-of-range slots re-read a valid edge and are discarded)
        int mnext[2], rnext[2];                  // (source, row) of the next step's two edges; a node without edges reads nothing
        auto entry = [&](int kk, int& m, int& r) {
            const int ke = min(a0 + min(kk, max(cnt - 1, 0)), a_hi);
            m = cnt > 0 ? src_of(ke) : 0;
            r = cnt > 0 ? row_of(ke) : 0;
        };
#pragma unroll
        for (int i = 0; i < 2; ++i) entry(i, mnext[i], rnext[i]);
        float zero1 = 0.f;
        if (L0) asm volatile("" : "+v"(zero1));          // opaque to the optimiser: the expressions keep their shape
        const f4 zero4 = {zero1, zero1, zero1, zero1};
        for (int k = 0; !ROWS && k < mx; k += 2) {
            f4 q0[2], q1[2], q2[2], y0[2], y1[2], y2[2], w0[2], w1[2], w2[2];
            float gx[2], gy[2], gz[2], cx[2], cy[2], cz[2];
            const int mc[2] = {mnext[0], mnext[1]}, rc[2] = {rnext[0], rnext[1]};
#pragma unroll
            for (int i = 0; i < 2; ++i)          // entries of the NEXT step: their latency hides behind this step's gathers
                entry(k + 2 + i, mnext[i], rnext[i]);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const size_t a = (size_t)rc[i];
                const int m = mc[i];
                const float* g = geo + a * GEO_STRIDE;
                gx[i] = g[2]; gy[i] = g[3]; gz[i] = g[4];
                cx[i] = XC ? g[5] : 0.f; cy[i] = XC ? g[6] : 0.f; cz[i] = XC ? g[7] : 0.f;
                q0[i] = ld_blk(qbuf, a, 3 * D::HP, t, nb.lane); q1[i] = L0 ? zero4 : ld_blk(qbuf, a, 3 * D::HP, HT + t, nb.lane);
                q2[i] = ld_blk(qbuf, a, 3 * D::HP, 2 * HT + t, nb.lane);
                y0[i] = ld_blk(xq, m, 3 * D::HP, t, nb.lane); y1[i] = L0 ? zero4 : ld_blk(xq, m, 3 * D::HP, HT + t, nb.lane);
                y2[i] = ld_blk(xq, m, 3 * D::HP, 2 * HT + t, nb.lane);
                w0[i] = L0 ? zero4 : ld_blk(vec_in, (size_t)m * 3 + 0, D::HP, t, nb.lane);
                w1[i] = L0 ? zero4 : ld_blk(vec_in, (size_t)m * 3 + 1, D::HP, t, nb.lane);
                w2[i] = L0 ? zero4 : ld_blk(vec_in, (size_t)m * 3 + 2, D::HP, t, nb.lane);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (k + i < cnt) {
                    const f4 xm = (y0[i] + xn0) * q0[i];
                    dx += xm;
                    const f4 a2 = (y1[i] + xn1) * q1[i] * inv_sqrt3;
                    const f4 a3 = (y2[i] + xn2) * q2[i];
                    v0 += (XC ? w0[i] * a2 + a3 * gx[i] + xm * cx[i] : w0[i] * a2 + a3 * gx[i]) * inv_sqrt_h;
                    v1 += (XC ? w1[i] * a2 + a3 * gy[i] + xm * cy[i] : w1[i] * a2 + a3 * gy[i]) * inv_sqrt_h;
                    v2 += (XC ? w2[i] * a2 + a3 * gz[i] + xm * cz[i] : w2[i] * a2 + a3 * gz[i]) * inv_sqrt_h;
                }
        }
        const f4 sa = (ld_blk(s, n, D::HP, t, nb.lane) + dx) * inv_sqrt2;
        v0 += ld_blk(vec_in, (size_t)n * 3 + 0, D::HP, t, nb.lane);
        v1 += ld_blk(vec_in, (size_t)n * 3 + 1, D::HP, t, nb.lane);
        v2 += ld_blk(vec_in, (size_t)n * 3 + 2, D::HP, t, nb.lane);
        lds_st(in, t, nb.lane, sa);
        lds_st(vx + 0 * HT * 256, t, nb.lane, v0);
        lds_st(vx + 1 * HT * 256, t, nb.lane, v1);
        lds_st(vx + 2 * HT * 256, t, nb.lane, v2);
        if (sa_out != nullptr && nb.valid) {
            st_blk(sa_out, n, D::HP, t, nb.lane, sa);
            st_blk(va_out, (size_t)n * 3 + 0, D::HP, t, nb.lane, v0);
            st_blk(va_out, (size_t)n * 3 + 1, D::HP, t, nb.lane, v1);
            st_blk(va_out, (size_t)n * 3 + 2, D::HP, t, nb.lane, v2);
        }
    }
    TL(2);
    __syncthreads();
    TL(3);

    // 2. vec_proj for owned tile pairs (t, HT + t), frame scalar, vdot; keep vec2 / vdot in registers
    const float fx = x1[n * 3], fy = x1[n * 3 + 1], fz = x1[n * 3 + 2];
    const float* l3 = wb + lo.l3u;
    f4 v2k[TPW][3], vdk[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = nb.wave + i * WAVES;
        if (t < HT) {                                    // wave-uniform
            TileJob job[2] = {tile_job<HT>(wb + lo.vp, t, vx), tile_job<HT>(wb + lo.vp, HT + t, vx)};   // each chunk feeds x, y and z
            f4 acc[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] = f4zero();
            dense_seq_xyz<HT, 2, HT * 256, (ROWS ? 5 : OARD_NODE_SEQ_G), ROWS>(job, nb.lane, acc);    // (the small-batch instantiation has the registers for dense_seq's order)   // 5: no scratch in the small-batch instantiation
            const f4 v1[3] = {acc[0], acc[1], acc[2]}, v2[3] = {acc[3], acc[4], acc[5]};
#pragma unroll
            for (int x = 0; x < 3; ++x) v2k[i][x] = v2[x];
            const f4 sc = v1[0] * fx + v1[1] * fy + v1[2] * fz;
            vdk[i] = (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) * inv_sqrt_h;
            f4 sca;
            const int f0 = 16 * t + 4 * nb.g;
            if (tp.npb <= 4) {
                // one value per lane: lane -> (feature lane >> 2, column lane & 3) of this tile, through the LDS block
                float* blk = in + (HT + t) * 256;
                lds_st(in, HT + t, nb.lane, sc);
                __builtin_amdgcn_wave_barrier();        // same-wave LDS traffic: the queue is in order, keep the compiler in order too
                const int f = nb.lane >> 2, c = nb.lane & 3;
                float* cell = blk + (16 * (f >> 2) + c) * 4 + (f & 3);
                const float y = (c < tp.npb && 16 * t + f < D::H) ? lin3u1(l3s, l3, *cell) : 0.f;
                *cell = y;                  // columns 4..15 of the block are padding and keep the raw projection
            } else {
                // table where every argument of the wave lies inside it (|x| < L3T_X), the MLP itself otherwise
                const bool in_tab = fabsf(sc.x) < L3T_X && fabsf(sc.y) < L3T_X && fabsf(sc.z) < L3T_X && fabsf(sc.w) < L3T_X;
                if (l3t_ok && !__any(!in_tab))
                    sca = (f4){lin3u_table_eval(l3t, sc.x), lin3u_table_eval(l3t, sc.y), lin3u_table_eval(l3t, sc.z), lin3u_table_eval(l3t, sc.w)};
                else
                    sca = lin3u4(l3s, l3, sc);
                sca.x = f0 + 0 < D::H ? sca.x : 0.f; sca.y = f0 + 1 < D::H ? sca.y : 0.f;
                sca.z = f0 + 2 < D::H ? sca.z : 0.f; sca.w = f0 + 3 < D::H ? sca.w : 0.f;
                lds_st(in, HT + t, nb.lane, sca);
            }
        }
    }
    TL(4);
    __syncthreads();
    TL(5);

    // 3. xvec_proj hidden
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) { job[i] = tile_job<2 * HT>(wb + lo.xv0, min(nb.wave + i * WAVES, HT - 1), in); acc[i] = f4zero(); }
        dense_seq<2 * HT, TPW>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < HT) lds_st(hx, nb.wave + i * WAVES, nb.lane, silu4(acc[i]));
    }
    TL(6);
    __syncthreads();
    TL(7);

    // 4. outputs for owned tiles
    {
        TileJob job[3 * TPW];
        f4 acc[3 * TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = min(nb.wave + i * WAVES, HT - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) { job[3 * i + k] = tile_job<HT>(wb + lo.xv2, k * HT + t, hx); acc[3 * i + k] = f4zero(); }
        }
        dense_seq<HT, 3 * TPW>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = nb.wave + i * WAVES;
            if (t < HT && nb.valid) {
                const f4 a = acc[3 * i], b = acc[3 * i + 1], c = acc[3 * i + 2];
                st_blk(s_out, n, D::HP, t, nb.lane, lds_blk(in, t, nb.lane) + (a + b + vdk[i]) * inv_sqrt2);
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    st_blk(vec_out, (size_t)n * 3 + x, D::HP, t, nb.lane,
                           lds_blk(vx + x * HT * 256, t, nb.lane) + c * v2k[i][x]);
            }
        }
    }
    TL(0);
    TL_END();
}

// =====================================================================================================
// init / output node stages in the same shape (WAVES waves share tp.npb nodes, one hidden tile per wave)
// =====================================================================================================
// NeighborEmb aggregation + s2v.lin1 (see k_neighbor):  s = z_emb + sum_m f(m->n) * nb[m];  s1 = SiLU(LN0(Linear(s)))
template <class D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_neighbor_v1(TopoDev tp, const float* __restrict__ wb, PackOff po,
                                                            const float* __restrict__ zemb, const float* __restrict__ nbe,
                                                            const float* __restrict__ ew, float* __restrict__ s,
                                                            float* __restrict__ s1) {
    constexpr int HT = D::HT, TPW = (HT + WAVES - 1) / WAVES;
    __shared__ __attribute__((aligned(16))) float sm[2 * HT * 256];
    float* sv = sm;
    float* yv = sm + HT * 256;
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    const int n = nb.n, smp = tp.node_sample[n], s0 = tp.sample_ptr[smp];
    const int ns = nb.valid ? tp.sample_ptr[smp + 1] - s0 : 0;
    const int mx = wave_max(ns);
    const int self = n - s0;
    const float* c0f = wb + po.c0row + 2 * D::H;
    for (int t = nb.wave; t < HT; t += WAVES) {
        // the neighbour sum on its own, z_emb added ONCE at the end, as `s = z_emb + scatter(...)` does (leftnet.py:81-89, 789): a chain that
        // starts at z_emb (|.| up to 13) rounds each of the ~60 small terms at that magnitude (round 6, tools/config1_locate.py: s0 sat at
        // 5e-7 ... 1.1e-6 of its largest entry, plain torch float32 at 2.5e-7)
        f4 acc = f4zero();
        const bool fok = 16 * t + 4 * nb.g < D::H;                 // the f section is H wide, not HP
        const int fo = 16 * t + 4 * nb.g;
        // four neighbours in flight per step; slot k of the sample is node s0 + k, the own slot is skipped
        for (int k = 0; k < mx; k += 4) {
            int r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = min(k + i, max(ns - 1, 0)), m = s0 + kk;
                r[i] = kk == self ? -1 : tp.edge_row[tp.edge_ptr[m] + self - (self > kk ? 1 : 0)];
            }
            f4 f[4], x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = min(k + i, max(ns - 1, 0));
                const float* frow = (r[i] >= 0 && r[i] < tp.A) ? ew + (size_t)r[i] * D::WP + 2 * D::H : c0f;
                f[i] = fok ? ld_f4(frow + fo) : f4zero();
                x[i] = ld_blk(nbe, s0 + kk, D::HP, t, nb.lane);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < ns && r[i] >= 0) acc += f[i] * x[i];
        }
        acc += ld_blk(zemb, n, D::HP, t, nb.lane);
        lds_st(sv, t, nb.lane, acc);
        if (nb.valid) st_blk(s, n, D::HP, t, nb.lane, acc);
    }
    __syncthreads();
    {
        TileJob job[TPW];
        f4 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = min(nb.wave + i * WAVES, HT - 1);
            job[i] = tile_job<HT>(wb + po.s2v, t, sv);
            acc[i] = ld_vec(wb + po.s2v_b, t, nb.lane);
        }
        dense_seq<HT, TPW>(job, nb.lane, acc);
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < HT) lds_st(yv, nb.wave + i * WAVES, nb.lane, acc[i]);
    }
    __syncthreads();
    float mean, rstd;
    ln_stats_lds<HT, D::H>(yv, nb.lane, mean, rstd);
    for (int t = nb.wave; t < HT; t += WAVES) {
        const int f0 = 16 * t + 4 * nb.g;
        f4 y = (lds_blk(yv, t, nb.lane) - mean) * rstd;
        y.x = f0 + 0 < D::H ? y.x : 0.f; y.y = f0 + 1 < D::H ? y.y : 0.f;
        y.z = f0 + 2 < D::H ? y.z : 0.f; y.w = f0 + 3 < D::H ? y.w : 0.f;
        if (nb.valid) st_blk(s1, n, D::HP, t, nb.lane, silu4(y));
    }
}

// CFConvS2V aggregation (see k_s2v_agg):  NE1[n][x][:] = sum_{m active->n} f(m->n) * s1[m] * coord_diff(m->n)[x]
template <class D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_s2v_agg_v1(TopoDev tp, const float* __restrict__ s1,
                                                           const float* __restrict__ ew, const float* __restrict__ geo,
                                                           float* __restrict__ ne1) {
    constexpr int HT = D::HT;
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    const int n = nb.n, a0 = tp.act_ptr[n], cnt = nb.valid ? tp.act_ptr[n + 1] - a0 : 0;
    const int mx = wave_max(cnt);
    const long long a_hi = max(tp.A - 1, 0LL);
    for (int t = nb.wave; t < HT; t += WAVES) {
        f4 ax = f4zero(), ay = f4zero(), az = f4zero();
        const bool fok = 16 * t + 4 * nb.g < D::H;
        for (int k = 0; k < mx; k += 4) {
            f4 f[4], x[4];
            float gx[4], gy[4], gz[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t a = (size_t)min((long long)a0 + min(k + i, max(cnt - 1, 0)), a_hi);
                const int m = tp.act_src[a];
                const float* g = geo + a * GEO_STRIDE;
                gx[i] = g[2]; gy[i] = g[3]; gz[i] = g[4];
                f[i] = fok ? ld_f4(ew + a * D::WP + 2 * D::H + 16 * t + 4 * nb.g) : f4zero();
                x[i] = ld_blk(s1, m, D::HP, t, nb.lane);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < cnt) {
                    const f4 p = f[i] * x[i];
                    ax += p * gx[i]; ay += p * gy[i]; az += p * gz[i];
                }
        }
        if (nb.valid) {
            st_blk(ne1, (size_t)n * 3 + 0, D::HP, t, nb.lane, ax);
            st_blk(ne1, (size_t)n * 3 + 1, D::HP, t, nb.lane, ay);
            st_blk(ne1, (size_t)n * 3 + 2, D::HP, t, nb.lane, az);
        }
    }
}

// output block (see k_out): dpos = gate * vec2_proj(vec), gate from update_net([s, |vec1_proj(vec)|]); h_out = embedding_out(s)
// ---- float64 pieces of the output head (round 6) ------------------------------------------------------------------------------------
// dpos = gate * vec2_proj(vec), gate = update_net(...)[1]: two dot products whose VALUES are ~10 x smaller than their terms, behind a
// 392 -> 196 layer.  In float32 this block alone costs 2e-6 ... 3.5e-6 of the velocity (plain torch float32: 2.4e-6; tools/stage_error.py,
// tools/config1_locate.py) - more than the whole network in front of it (1.8e-6).  It is O(N H^2) work, once per call: update_net and
// vec2_proj run on the float64 MFMA (v_mfma_f64_16x16x4_f64; ~100 of them per wave), SiLU and the two dots in float64 VALU.  vec1_proj and
// the norm stay float32 (measured with the oracle: their precision does not move the result).
typedef double d4 __attribute__((ext_vector_type(4)));
OARD_DEV double col_reduce64(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
// One 16-row output tile of a Linear layer over an LDS-resident float32 input, accumulated in float64.  Operands as the float32 instruction
// (A: lane 16 k + i = W[i][k], B: lane 16 k + j = x[k][j]), so the packed weight chunks and the LDS blocks are used as they are; the RESULT
// layout differs: component r of lane (g, j) is row g + 4 r of the tile (tools/micro/mfma_f64_layout.hip), not 4 g + r.
template <int KB>
OARD_DEV d4 dense_tile_lds_f64(const float* __restrict__ wp, int t, const float* in, int lane) {
    const float* base = wp + ((size_t)t * KB * 64 + lane) * 4;
    d4 c = {0.0, 0.0, 0.0, 0.0};
    constexpr int G = 13;
#pragma unroll
    for (int b0 = 0; b0 < KB; b0 += G) {
        f4 a[G];
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (b0 + i < KB) a[i] = ld_f4(base + (size_t)(b0 + i) * 256);
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (b0 + i < KB) {
                const f4 x = lds_blk(in, b0 + i, lane);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[i].x, (double)x.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[i].y, (double)x.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[i].z, (double)x.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[i].w, (double)x.w, c, 0, 0, 0);
            }
    }
    return c;
}

template <class D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_out_v1(TopoDev tp, const float* __restrict__ wb, PackOff po,
                                                       const float* __restrict__ s, const float* __restrict__ vec,
                                                       float* __restrict__ dpos, float* __restrict__ hout,
                                                       int* __restrict__ status) {
    constexpr int HT = D::HT, TPW = (HT + WAVES - 1) / WAVES;
    __shared__ __attribute__((aligned(16))) float sm[5 * HT * 256];
    __shared__ double red[4][16][16];      // [v2 x, y, z | gate][wave][column] partial sums
    float* vx = sm;                        // [3][HT]
    float* in = sm + 3 * HT * 256;         // [2 HT]: s | |vec1_proj(vec)|
    const NodeBlk nb = node_blk(tp.N, tp.npb);
    const int n = nb.n;
    double part[3] = {0.0, 0.0, 0.0};
    for (int t = nb.wave; t < HT; t += WAVES) {
        const f4 w = ld_vec(wb + po.v2p, t, nb.lane);
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const f4 v = ld_blk(vec, (size_t)n * 3 + x, D::HP, t, nb.lane);
            lds_st(vx + x * HT * 256, t, nb.lane, v);
            part[x] += (double)v.x * (double)w.x + (double)v.y * (double)w.y + (double)v.z * (double)w.z + (double)v.w * (double)w.w;
        }
        lds_st(in, t, nb.lane, ld_blk(s, n, D::HP, t, nb.lane));
    }
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double p = col_reduce64(part[x]);
        if (nb.g == 0 && nb.wave < 16) red[x][nb.wave][nb.lane & 15] = p;
    }
    __syncthreads();
    {
        TileJob job[TPW];
        f4 acc[3 * TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            job[i] = tile_job<HT>(wb + po.v1p, min(nb.wave + i * WAVES, HT - 1), vx);
#pragma unroll
            for (int x = 0; x < 3; ++x) acc[3 * i + x] = f4zero();
        }
        dense_seq_xyz<HT, TPW, HT * 256, OARD_NODE_SEQ_G, true>(job, nb.lane, acc);       // every chunk of vec1_proj feeds x, y and z
#pragma unroll
        for (int i = 0; i < TPW; ++i)
            if (nb.wave + i * WAVES < HT) {
                const f4 q = acc[3 * i] * acc[3 * i] + acc[3 * i + 1] * acc[3 * i + 1] + acc[3 * i + 2] * acc[3 * i + 2];
                lds_st(in, HT + nb.wave + i * WAVES, nb.lane, (f4){sqrtf(q.x), sqrtf(q.y), sqrtf(q.z), sqrtf(q.w)});
            }
    }
    __syncthreads();
    {
        // update_net: hidden = SiLU(W0 [s | v1] + b0) tile by tile in float64; the gate row of W2 is applied to the tile at once, so the
        // hidden vector is never stored: gate = b2[1] + sum over tiles, lane groups and components of W2[1][16 t + g + 4 r] h_r
        const float* b0 = wb + po.un0_b;
        const float* w2 = wb + po.un2;             // packed [1 tile][HT chunks]: chunk t, lane (g', o), component r' = W2[o][16 t + 4 g' + r']
        double gpart = 0.0;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = nb.wave + i * WAVES;
            if (t < HT) {
                const d4 z = dense_tile_lds_f64<2 * HT>(wb + po.un0, t, in, nb.lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + nb.g + 4 * r;                       // the float64 MFMA's result layout
                    const double zz = z[r] + (double)b0[row];
                    const double h = zz / (1.0 + exp(-zz));
                    gpart += (double)w2[(size_t)t * 256 + (16 * r + 1) * 4 + nb.g] * h;      // W2[1][row]: g' = r, o = 1, r' = g
                }
            }
        }
        const double gp = col_reduce64(gpart);
        if (nb.g == 0 && nb.wave < 16) red[3][nb.wave][nb.lane & 15] = gp;
    }
    __syncthreads();
    if (nb.wave == 0 && nb.valid && nb.g == 0) {
        double v[4] = {0.0, 0.0, 0.0, (double)(wb + po.un2_b)[1]};
        constexpr int NWV = WAVES < 16 ? WAVES : 16;
#pragma unroll
        for (int x = 0; x < 4; ++x)
            for (int w = 0; w < NWV; ++w) v[x] += red[x][w][nb.lane & 15];
        const float d0 = (float)(v[3] * v[0]), d1 = (float)(v[3] * v[1]), d2 = (float)(v[3] * v[2]);
        dpos[n * 3] = d0; dpos[n * 3 + 1] = d1; dpos[n * 3 + 2] = d2;
        if (isnan(d0) || isnan(d1) || isnan(d2)) atomicOr(status, 1);
    }
    if (nb.wave == (WAVES > 1 ? 1 : 0)) {
        const f4 ho = dense_tile_lds<HT>(wb + po.embout, 0, in, nb.lane, ld_vec(wb + po.embout_b, 0, nb.lane));
        if (nb.valid) st_blk(hout, n, 16, 0, nb.lane, ho);
    }
}
