// oard_conf.h — the readout of the Confidence model (oa_reactdiff/dynamics/confidence.py:157-163), behind the LEFTNet trunk run with
// for_conf=True (model/leftnet.py:875-876: the node scalars s after the last layer are the trunk's output):
//
//     g    = scatter_mean(s, combined_mask)                                   [B, H]
//     conf = mlp(g) * sigmoid(gmlp(g))                                        [B]     GatedMLP, model/core.py:95-131
//
// with mlp / gmlp two independent H -> H -> H -> 1 stacks of nn.Linear, SiLU behind layers 0 and 1 and nothing behind layer 2
// (last_layer_no_activation).  One workgroup of 16 waves per reaction, launched once per sub-batch on that sub-batch's stream.
//   1. pooling: the workgroup is 4 row groups x 256 column threads; thread (j, c) adds column c of the reaction's rows n0 + j, n0 + j + 4,
//      ... of s ([N][HP], the workspace's internal sample-major order) in ascending order, and the four partial sums are added in the
//      order j = 0 .. 3 and divided by the row count.  Columns H .. HP - 1 of s are padding that the trunk's kernels may leave in any
//      state: they are never read.
//   2. the dense layers: a wave owns four consecutive output rows at a time (of one branch: H is a multiple of 4), rows 4 w, 4 w + 64,
//      ... of the 2 H rows of both branches; its lanes read the four nn.Linear rows as float4 (coalesced, four loads in flight) and
//      wave_sum_f64 adds the 64 partial sums of each row in a fixed butterfly.  The launch is latency-bound - a reaction is ONE
//      workgroup, every row a load -> multiply-add -> butterfly chain -, hence sixteen waves and four rows in flight per wave.
// Everything behind the float32 loads is float64 (390 k multiply-adds per reaction at H = 196, against 0.6 MB of weight reads from L2), so
// the readout adds nothing measurable to the trunk's float32 error.  No atomics: a reaction's value depends on its own rows alone, bit
// for bit - not on the other reactions of the launch, nor on the sub-batch split.
// The raw nn.Linear tensors are read where the module keeps them (no packed form: 12 tensors, read once per reaction).
#pragma once
#include "oard_kernels.h"

#define CONF_WAVES 16
#define CONF_COLS 256                                   // column threads of the pooling step; CONF_WAVES * 64 / CONF_COLS row groups
#define CONF_GROUPS (CONF_WAVES * 64 / CONF_COLS)       // = 4: the partial sums fill the 4 H doubles of h1 | h2

static_assert(CONF_GROUPS == 4, "k_conf_readout adds four partial sums by hand");

// readout.{mlp,gmlp}.mlp.{0,1,2}.linear.{weight,bias} in state-dict order: p[6 * branch + 2 * layer + (0 = weight [out][in], 1 = bias)]
struct ConfReadout { const float* p[12]; };

OARD_DEV double conf_silu(double x) { return x / (1.0 + exp(-x)); }

OARD_DEV double conf_dot4(float4 w, const double* x, double acc) {
    return fma((double)w.x, x[0], fma((double)w.y, x[1], fma((double)w.z, x[2], fma((double)w.w, x[3], acc))));
}

// One dense layer of both branches: out[br][o] = SiLU(bias[o] + sum_i W[o][i] in[br][i]), o < H.  `shared_in`: both branches read in[0].
// `pre` != nullptr (the backward kernel, oard_conf_bwd.h): the pre-activations are kept there as well.
OARD_DEV void conf_dense(const ConfReadout& w, int layer, int H, const double* in, bool shared_in, double* out, double* pre = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, H4 = H >> 2;
    for (int r = 4 * wave; r < 2 * H; r += 4 * CONF_WAVES) {
        const int br = r >= H ? 1 : 0, o = r - br * H;
        const float4* __restrict__ W = (const float4*)(w.p[6 * br + 2 * layer] + (size_t)o * H);     // rows o .. o + 3, H4 float4 each
        const double* x = in + (shared_in ? 0 : br * H);
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int i = lane; i < H4; i += 64) {
            const float4 w0 = W[i], w1 = W[H4 + i], w2 = W[2 * H4 + i], w3 = W[3 * H4 + i];
            const double* xi = x + 4 * i;
            a0 = conf_dot4(w0, xi, a0); a1 = conf_dot4(w1, xi, a1); a2 = conf_dot4(w2, xi, a2); a3 = conf_dot4(w3, xi, a3);
        }
        a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2); a3 = wave_sum_f64(a3);
        if (lane < 4) {
            const double a = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
            const double z = a + (double)w.p[6 * br + 2 * layer + 1][o + lane];
            out[br * H + o + lane] = conf_silu(z);
            if (pre) pre[br * H + o + lane] = z;
        }
    }
}

// Step 1: g[c] = mean over the rows n0 .. n1 - 1 of column c < H of s, in the fixed order described above.  `part`: [CONF_GROUPS][H] doubles
// of scratch LDS.  Ends with a barrier: every thread may read g.
OARD_DEV void conf_pool(const float* __restrict__ s, int H, int HP, int n0, int n1, double* part, double* g) {
    const int j = threadIdx.x / CONF_COLS;
    for (int c = threadIdx.x % CONF_COLS; c < H; c += CONF_COLS) {
        double acc = 0.0;
        for (int n = n0 + j; n < n1; n += CONF_GROUPS) acc += (double)s[(size_t)n * HP + c];
        part[j * H + c] = acc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += CONF_WAVES * 64)
        g[c] = (((part[c] + part[H + c]) + part[2 * H + c]) + part[3 * H + c]) / (double)(n1 - n0);
    __syncthreads();
}

// Step 2's last layer (H -> 1, no activation): wave 0 the value branch, wave 1 the gate branch; out[0] = v, out[1] = z.  The caller
// puts a barrier behind it.
OARD_DEV void conf_last(const ConfReadout& w, int H, const double* h2, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 2) {
        const float4* __restrict__ row = (const float4*)w.p[6 * wave + 4];
        double acc = 0.0;
        for (int i = lane; i < (H >> 2); i += 64) acc = conf_dot4(row[i], h2 + wave * H + 4 * i, acc);
        acc = wave_sum_f64(acc) + (double)w.p[6 * wave + 5][0];
        if (lane == 0) out[wave] = acc;
    }
}

// lds: 5 H doubles (dynamic): g [H] | h1 [2][H] | h2 [2][H]
OARD_KERNEL __global__ __launch_bounds__(CONF_WAVES * 64) void k_conf_readout(TopoDev tp, const float* __restrict__ s, int H, int HP,
                                                                              ConfReadout w, float* __restrict__ conf,
                                                                              int* __restrict__ status) {
    extern __shared__ double conf_lds[];
    double* g = conf_lds; double* h1 = g + H; double* h2 = h1 + 2 * H;
    const int b = blockIdx.x;
    if (b >= tp.B) return;
    const int n0 = tp.sample_ptr[b], n1 = tp.sample_ptr[b + 1];
    conf_pool(s, H, HP, n0, n1, h1, g);
    conf_dense(w, 0, H, g, true, h1);
    __syncthreads();
    conf_dense(w, 1, H, h1, false, h2);
    __syncthreads();
    conf_last(w, H, h2, g);                    // (g is dead: layer 1 read h1, and every wave is past the barrier behind it)
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (float)(g[0] / (1.0 + exp(-g[1])));
        conf[tp.node_tidx[n0]] = v;            // row = the reaction's combined_mask value (the host checked: ids are 0 .. B - 1)
        if (v != v) status[0] = 1;
    }
}
