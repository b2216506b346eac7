// oard_conf_bwd.h — adjoint of the Confidence model's readout (oard_conf.h): mean pool + GatedMLP, the seed of the reverse sweep of
// oard_confidence_forward_train (oard_confidence_tail_backward).  What the reference does instead: torch autograd through
// scatter_mean and GatedMLP (oa_reactdiff/dynamics/confidence.py:157-163, model/core.py:95-131).
//
//   k_conf_readout_bwd   one workgroup of 16 waves per reaction.  No tape entry beyond the trunk's s: g, the pre-activations of both
//       branches and the two logits are RECOMPUTED in float64 with the forward's own device functions (conf_pool / conf_dense /
//       conf_last: same order, columns >= H of s never read).  With v = mlp(g), z = gmlp(g), conf = v sigmoid(z):
//           dv = dconf sigmoid(z),   dz = dconf v sigmoid(z) (1 - sigmoid(z)),
//       then layers 2, 1, 0 of both branches backwards.  W^T d reads W[o][i] with the threads along i (coalesced): the workgroup is
//       4 groups of o x 256 column threads, each thread adds its o = j, j + 4, ... in ascending order, and the four partial sums are
//       added in the order j = 0 .. 3 - the pooling's scheme.  The two branches' cotangents of g are added (value + gate), and
//           ds[n][c] = dg[c] / n_b  for every node n of the reaction, c < H;  exact zeros for c in [H, HP);  dvec rows of the reaction = 0
//       (nothing flows into vec under for_conf).  ds and dvec arrive uninitialised and leave fully written.
//       Left in scratch per reaction (float64, CONF_OPS(H) doubles): the operands of the weight gradients,
//           g [H] | h1 [2][H] | h2 [2][H] | da0 [2][H] | da1 [2][H] | da2 [2]      (da_l: cotangent of layer l's pre-activation)
//   k_conf_wgrad          dW[o][i] += sum_b da[b][o] x[b][i], db[o] += sum_b da[b][o] for the 12 tensors: one thread per destination
//       element, b = 0 .. B - 1 in ascending order in float64, ONE float32 add into the destination.  No atomics: bit-identical run to
//       run, like oard_wgrad.
#pragma once
#include "oard_conf.h"

#define CONF_OPS(H) (9 * (size_t)(H) + 2)               // doubles per reaction in scratch
#define CONF_BWD_LDS(H) (24 * (size_t)(H))              // doubles of dynamic LDS

struct ConfReadoutGrads { float* p[12]; };              // ConfReadout's order; nullptr = skipped

OARD_DEV double conf_dsilu(double x) { const double s = 1.0 / (1.0 + exp(-x)); return s * (1.0 + x * (1.0 - s)); }

// out[br][i] = sum_o W_layer[br][o][i] d[br][o], i < H, both branches; `part`: [CONF_GROUPS][2 H] doubles.  Ends with a barrier.
OARD_DEV void conf_dense_t(const ConfReadout& w, int layer, int H, const double* d, double* part, double* out) {
    const int j = threadIdx.x / CONF_COLS;
    for (int c = threadIdx.x % CONF_COLS; c < 2 * H; c += CONF_COLS) {
        const int br = c >= H ? 1 : 0, i = c - br * H;
        const float* __restrict__ W = w.p[6 * br + 2 * layer];
        const double* db = d + br * H;
        double acc = 0.0;
        for (int o = j; o < H; o += CONF_GROUPS) acc = fma((double)W[(size_t)o * H + i], db[o], acc);
        part[j * 2 * H + c] = acc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * H; c += CONF_WAVES * 64)
        out[c] = ((part[c] + part[2 * H + c]) + part[4 * H + c]) + part[6 * H + c];
    __syncthreads();
}

// lds (dynamic, CONF_BWD_LDS(H) doubles): g [H] | z1 [2H] | h1 [2H] | z2 [2H] | h2 [2H] | da1 [2H] | da0 [2H] | t [2H] | dg.. [H] | part [4][2H]
OARD_KERNEL __global__ __launch_bounds__(CONF_WAVES * 64) void k_conf_readout_bwd(TopoDev tp, const float* __restrict__ s, int H, int HP,
                                                                                  ConfReadout w, const float* __restrict__ dconf,
                                                                                  float* __restrict__ ds, float* __restrict__ dvec,
                                                                                  double* __restrict__ ops) {
    extern __shared__ double conf_lds[];
    double* g = conf_lds; double* z1 = g + H; double* h1 = z1 + 2 * H; double* z2 = h1 + 2 * H; double* h2 = z2 + 2 * H;
    double* da1 = h2 + 2 * H; double* da0 = da1 + 2 * H; double* t = da0 + 2 * H; double* lg = t + 2 * H; double* part = lg + H;
    const int b = blockIdx.x, tid = threadIdx.x, NT = CONF_WAVES * 64;
    if (b >= tp.B) return;
    const int n0 = tp.sample_ptr[b], n1 = tp.sample_ptr[b + 1];
    if (n1 <= n0) return;                               // (the host checked: every id 0 .. B - 1 names a reaction with nodes)
    // ---- the forward, again ----
    conf_pool(s, H, HP, n0, n1, part, g);
    conf_dense(w, 0, H, g, true, h1, z1);
    __syncthreads();
    conf_dense(w, 1, H, h1, false, h2, z2);
    __syncthreads();
    conf_last(w, H, h2, lg);
    __syncthreads();
    // ---- the logit, layer 2 ----
    const double v = lg[0], sg = 1.0 / (1.0 + exp(-lg[1])), dc = (double)dconf[tp.node_tidx[n0]];
    const double da2[2] = {dc * sg, dc * v * sg * (1.0 - sg)};
    double* o_b = ops + (size_t)b * CONF_OPS(H);
    for (int c = tid; c < 2 * H; c += NT) {
        const int br = c >= H ? 1 : 0;
        da1[c] = (double)w.p[6 * br + 4][c - br * H] * da2[br] * conf_dsilu(z2[c]);
        o_b[H + c] = h1[c]; o_b[3 * H + c] = h2[c];
    }
    for (int c = tid; c < H; c += NT) o_b[c] = g[c];
    if (tid < 2) o_b[9 * H + tid] = da2[tid];
    __syncthreads();
    // ---- layers 1 and 0 ----
    conf_dense_t(w, 1, H, da1, part, t);
    for (int c = tid; c < 2 * H; c += NT) { da0[c] = t[c] * conf_dsilu(z1[c]); o_b[7 * H + c] = da1[c]; }
    __syncthreads();
    conf_dense_t(w, 0, H, da0, part, t);
    for (int c = tid; c < 2 * H; c += NT) o_b[5 * H + c] = da0[c];
    // ---- the pool: every node of the reaction gets dg / n_b; the pad columns and the vector state's cotangent are zero ----
    const double inv = 1.0 / (double)(n1 - n0);
    for (int c = tid; c < HP; c += NT) {
        const float val = c < H ? (float)((t[c] + t[H + c]) * inv) : 0.f;
        for (int n = n0; n < n1; ++n) ds[(size_t)n * HP + c] = val;
    }
    float* dv = dvec + (size_t)3 * n0 * HP;
    for (size_t k = tid; k < (size_t)3 * (n1 - n0) * HP; k += NT) dv[k] = 0.f;
}

// One thread per element of the 12 gradients: branch br, then [W0 H*H | b0 H | W1 H*H | b1 H | W2 H | b2 1] (T = 2 H H + 3 H + 1 each).
OARD_KERNEL __global__ __launch_bounds__(256) void k_conf_wgrad(int B, int H, const double* __restrict__ ops, ConfReadoutGrads gr) {
    const long long T = 2LL * H * H + 3LL * H + 1, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * T) return;
    const int br = idx >= T ? 1 : 0;
    long long r = idx - br * T;
    // (tensor, element, offset of da[.][o] and of x[.][i] in a reaction's operands; x < 0: a bias)
    int tensor, da_off, x_off = -1;
    if (r < (long long)H * H) { tensor = 0; da_off = 5 * H + br * H + (int)(r / H); x_off = (int)(r % H); }
    else if ((r -= (long long)H * H) < H) { tensor = 1; da_off = 5 * H + br * H + (int)r; }
    else if ((r -= H) < (long long)H * H) { tensor = 2; da_off = 7 * H + br * H + (int)(r / H); x_off = H + br * H + (int)(r % H); }
    else if ((r -= (long long)H * H) < H) { tensor = 3; da_off = 7 * H + br * H + (int)r; }
    else if ((r -= H) < H) { tensor = 4; da_off = 9 * H + br; x_off = 3 * H + br * H + (int)r; }
    else { r -= H; tensor = 5; da_off = 9 * H + br; }
    float* dst = gr.p[6 * br + tensor];
    if (!dst) return;
    double acc = 0.0;
    const size_t ld = CONF_OPS(H);
    if (x_off >= 0) for (int b = 0; b < B; ++b) acc = fma(ops[b * ld + da_off], ops[b * ld + x_off], acc);
    else for (int b = 0; b < B; ++b) acc += ops[b * ld + da_off];
    dst[r] += (float)acc;
}
