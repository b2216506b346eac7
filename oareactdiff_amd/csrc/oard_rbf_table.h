// oard_rbf_table.h - EquiMessage's rbf_proj as a table in u = exp(-d): the arithmetic shared by the fill / check kernels, k_rbf and the
// edge kernel (oard_kernels.h, oard_edge_v1.h).  Plain C++ besides the RBT_HD qualifier: tests/rbf_table/harness.cpp compiles it with g++.
//
// edge_rbf[k] = rb(d) * mask * exp(-beta_k (exp(-d) - mu_k)^2) is the INITIAL radial embedding (leftnet.py:63-69, 781-782), rbf_proj has
// no bias and means / betas are buffers, so  rbf_proj(edge_rbf)[c] = (rb * mask) * G_c(u),  G_c(u) = sum_k W[c][k] exp(-beta_k (u - mu_k)^2):
// one smooth function of ONE variable per output channel and layer.  The grid is uniform in u, where the Gaussians have a constant
// width (1 / sqrt(2 beta) ~ 0.0147 at the reference's R = 96); cubic Hermite between the points; envelope and mask stay per-edge factors.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RBT_HD __host__ __device__ inline
#else
#define RBT_HD inline
#endif

#define RBT_N 2048              // intervals of u in [0, 1]; RBT_N + 1 points
#define RBT_TOL 2e-7            // worst midpoint deviation a channel may show, as a fraction of its range (the criterion of L3T_*)

// Layout of one layer's table (floats): [slot = 3 tt + th][point 0 .. RBT_N][g 0..3][f x 4 | h f' x 4] - slot in the order of the packed
// T2 stream, (g, component s) = channel th * HP + 16 tt + 4 g + s like a lane's output fragment: the two points of an interval are the 64
// contiguous floats an edge's four lanes g read, 8 + 8 each.  Padding channels are zero.
RBT_HD size_t rbt_slot_floats() { return (size_t)(RBT_N + 1) * 32; }
RBT_HD size_t rbt_layer_floats(int HT) { return (size_t)3 * HT * rbt_slot_floats(); }

// G_c(u) and G_c'(u) in float64 from the float32 weights row w[R]
RBT_HD void rbt_eval_f64(const float* w, const float* means, const float* betas, int R, double u, double& f, double& df) {
    f = 0.0; df = 0.0;
    for (int k = 0; k < R; ++k) {
        const double q = u - (double)means[k], b = (double)betas[k], e = (double)w[k] * exp(-b * q * q);
        f += e; df += -2.0 * b * q * e;
    }
}
// the two stored entries of a point: value and derivative times the step, rounded to float32 once
RBT_HD void rbt_entry(double f, double df, float& fo, float& dfo) { fo = (float)f; dfo = (float)(df * (1.0 / RBT_N)); }

// Hermite basis at fraction t of an interval, in float64: value = h[0] f0 + h[1] d0 + h[2] f1 + h[3] d1
RBT_HD void rbt_basis(double t, double (&h)[4]) {
    const double s = 1.0 - t;
    h[0] = (1.0 + 2.0 * t) * s * s; h[1] = t * s * s; h[2] = t * t * (3.0 - 2.0 * t); h[3] = t * t * (t - 1.0);
}
// the check's evaluation: an interval's midpoint from the STORED float32 entries, in float64 (basis 1/2, 1/8, 1/2, -1/8: exact)
RBT_HD double rbt_midpoint(float f0, float d0, float f1, float d1) {
    return 0.5 * (double)f0 + 0.125 * (double)d0 + 0.5 * (double)f1 - 0.125 * (double)d1;
}
RBT_HD bool rbt_channel_ok(double worst_dev, double range) { return worst_dev <= RBT_TOL * (range > 1e-30 ? range : 1e-30) && range < 3e38; }

// Per inner row and call (k_rbf): interval, fraction and the per-edge factor, all in float64 - a float32 u would cost 2e-6 of the result,
// the Gaussians are narrow.  u = exp(-d) lies in (0, 1]; u = 1 (d = 0) is the end of the LAST interval (fraction 1).
// factor = rb(d) * mask, rb = the cosine envelope, 0 from the cutoff on.
struct RbtAt { int idx; double frac, factor; };
RBT_HD RbtAt rbt_locate(double d, double cutoff, double mask) {
    RbtAt r;
    const double u = exp(-d), x = u * (double)RBT_N;
    int i = (int)floor(x);
    i = i < 0 ? 0 : (i > RBT_N - 1 ? RBT_N - 1 : i);
    r.idx = i;
    r.frac = x - (double)i;
    const double rb = 0.5 * (cos(d * 3.14159265358979323846 / cutoff) + 1.0);
    r.factor = (d < cutoff ? rb : 0.0) * mask;
    return r;
}
// what the edge kernel multiplies the four entries of a channel by: Hermite basis x factor, rounded to float32 once
RBT_HD void rbt_weights(const RbtAt& at, float (&w)[4]) {
    double h[4];
    rbt_basis(at.frac, h);
    for (int j = 0; j < 4; ++j) w[j] = (float)(h[j] * at.factor);
}
// One record per inner row (k_rbf -> k_equi_edge_v1): [interval as int bits, w0, w1, w2, w3, -, -, -]
#define RBT_ROW 8
