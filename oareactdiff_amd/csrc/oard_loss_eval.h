// oard_loss_eval.h — the evaluation half of the loss around the denoising call: the variational bound the reference logs per
// validation epoch (`_shared_eval`, oa_reactdiff/trainer/pl_trainer.py:349-382).
//
// What the reference does per validation batch in ~150 eager torch ops around two network calls, plus six .item() reads:
//   EnVariationalDiffusion.forward, `not self.training` branch   oa_reactdiff/diffusion/en_diffusion.py:56-248 (helpers :250-449)
//   DDPMModule.compute_loss, the `vlb` form                      oa_reactdiff/trainer/pl_trainer.py:246-282
// Here: k_eval_prep (normalise the batch once, CoM-free noise for BOTH noised representations, z_t = alpha_t x + sigma_t eps_t and
// z_0 = alpha_0 x + sigma_0 eps_0), TWO inference network calls (at t and at 0), k_vlb_terms (per sample: the unmasked error_t, the
// t = 0 likelihood terms of every sample on z_0, SNR_weight, neg_log_constants, and
//   nll = sum_k(-T/2 SNR_weight error_t_k) + sum_k(loss_0_x + loss_0_cat + loss_0_charge)_k + neg_log_constants - delta_log_px;
// kl_prior and log_pN are 0 as in oareactdiff_amd/loss.py).  k_loss_prep / k_loss_terms (oard_loss.h) stay the l2 training form.
//
// Precision.  nll cancels: neg_log_constants is negative (gamma_0 ~ -11.5 at precision 1e-5), everything else is positive - so every
// per-sample sum is carried in double and rounded once.  SNR_weight = 1 - exp(-(gamma_s - gamma_t)) loses most of its digits in
// float32 (the difference is ~1e-3): it is read from a [T+1] table the host evaluates in float64 and rounds once.  The discretised
// likelihoods (erf, log, logsumexp) are evaluated in double on the float32 z_0; the charge estimate is truncated in float32 exactly as
// k_loss_terms does.
#pragma once
#include "oard_loss.h"

struct EvalPrepPtrs {
    const float* pos[OARD_MAX_OBJECTS];          // [n_k][3]            dataset layout, reference rows (as LossPtrs)
    const long long* one_hot[OARD_MAX_OBJECTS];  // [n_k][nf_k - 4]
    const long long* charge[OARD_MAX_OBJECTS];   // [n_k][1]
    const float* noise_t[OARD_MAX_OBJECTS];      // [n_k][nf_k]         raw N(0,1) draws of z_t
    const float* noise_0[OARD_MAX_OBJECTS];      // [n_k][nf_k]         raw N(0,1) draws of z_0
    float* z_t[OARD_MAX_OBJECTS];                // [n_k][nf_k]         network input at t
    float* eps_t[OARD_MAX_OBJECTS];              // [n_k][nf_k]         the noise that was added (CoM-free positions)
    float* z_0[OARD_MAX_OBJECTS];                // [n_k][nf_k]         network input at 0
    float* eps_0[OARD_MAX_OBJECTS];
    int node_nf[OARD_MAX_OBJECTS];
};
struct VlbPtrs {
    const float* eps_t[OARD_MAX_OBJECTS];
    const float* net_t[OARD_MAX_OBJECTS];        // network output at t
    const float* eps_0[OARD_MAX_OBJECTS];
    const float* net_0[OARD_MAX_OBJECTS];        // network output at 0
    const float* z_0[OARD_MAX_OBJECTS];
    const long long* one_hot[OARD_MAX_OBJECTS];
    const long long* charge[OARD_MAX_OBJECTS];
    int node_nf[OARD_MAX_OBJECTS];
};

// index of a [T+1] schedule table for a time step held as a float: rounded, and clamped into [0, T] so that an out-of-contract t_int
// (negative, beyond T, NaN) cannot read out of bounds
OARD_DEV int table_index(float ti, int T) { return ti >= 0.f ? (ti < (float)T ? (int)(ti + 0.5f) : T) : 0; }      // NaN: 0

OARD_DEV double gauss_cdf_d(double x) { return 0.5 * (1.0 + erf(x * 0.70710678118654752440)); }

// one thread per node: z_t, eps_t, z_0, eps_0                    en_diffusion.py:250-306 (noised_representation, twice: :98-101, :181-186)
OARD_KERNEL __global__ void k_eval_prep(TopoDev tp, EvalPrepPtrs ep, LossCfg lc, const float* __restrict__ t_int,
                                        const float* __restrict__ gamma) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= tp.N) return;
    const int obj = tp.node_obj[n], row = tp.node_row[n], nf = ep.node_nf[obj];
    const int q = tp.node_sample[n] * tp.n_obj + obj;
    const int g0 = tp.grp_ptr[q], g1 = tp.grp_ptr[q + 1];
    const float gm_t = gamma[table_index(t_int[tp.node_tidx[n]], lc.T)];  // gamma_module(t) = gamma[round(t T)], t = t_int / T
    const float gm_0 = gamma[0];
    const float alpha_t = sqrtf(sigmoid_f(-gm_t)), sigma_t = sqrtf(sigmoid_f(gm_t));
    const float alpha_0 = sqrtf(sigmoid_f(-gm_0)), sigma_0 = sqrtf(sigmoid_f(gm_0));
    const float* Rt = ep.noise_t[obj];
    const float* R0 = ep.noise_0[obj];
    const bool fixed = (lc.fixed_mask >> obj) & 1;
    float mt[3] = {0.f, 0.f, 0.f}, m0[3] = {0.f, 0.f, 0.f};
    for (int k = g0; k < g1; ++k) {                                       // scatter_mean order = ascending row (_utils.py:22-31)
        const size_t o = (size_t)tp.node_row[k] * nf;
        mt[0] += Rt[o]; mt[1] += Rt[o + 1]; mt[2] += Rt[o + 2];
        m0[0] += R0[o]; m0[1] += R0[o + 1]; m0[2] += R0[o + 2];
    }
    const float inv = 1.0f / (float)(g1 - g0);
    const size_t o = (size_t)row * nf;
    for (int c = 0; c < nf; ++c) {
        float x, et, e0;
        if (c < 3) {
            x = (ep.pos[obj][(size_t)row * 3 + c] - lc.norm_bias[0]) / lc.norm_value[0];
            et = Rt[o + c] - mt[c] * inv;
            e0 = R0[o + c] - m0[c] * inv;
        } else {
            if (c < nf - 1) x = ((float)ep.one_hot[obj][(size_t)row * (nf - 4) + (c - 3)] - lc.norm_bias[1]) / lc.norm_value[1];
            else x = ((float)ep.charge[obj][row] - lc.norm_bias[2]) / lc.norm_value[2];
            et = lc.pos_only ? 0.f : Rt[o + c];
            e0 = lc.pos_only ? 0.f : R0[o + c];
        }
        if (fixed) { et = 0.f; e0 = 0.f; }
        ep.eps_t[obj][o + c] = et;
        ep.z_t[obj][o + c] = alpha_t * x + sigma_t * et;
        ep.eps_0[obj][o + c] = e0;
        ep.z_0[obj][o + c] = alpha_0 * x + sigma_0 * e0;
    }
}

// one 64-thread block per sample.  terms [5 n_obj + 2][B] (B: the row stride; the call owns the columns its t_int rows name):
//   rows [0, K)    error_t per object, normalised and scaled (the logged error_t_k is its mean / (scale_k + 1e-4))   pl_trainer.py:236-244, 265-269
//   rows [K, 2K)   error_t per object, un-normalised                        en_diffusion.py:129-137 (not masked in evaluation)
//   rows [2K, 3K)  loss_0_x       rows [3K, 4K)  loss_0_cat       rows [4K, 5K)  loss_0_charge            en_diffusion.py:181-199, 332-449
//   row 5K         SNR_weight = snr[t]                                      en_diffusion.py:139-140
//   row 5K + 1     neg_log_constants                                        en_diffusion.py:143-146, 308-330
// An empty (sample, object) group contributes 0 and gets exact zeros in its five entries; only the normalised row divides by a size.
OARD_KERNEL __global__ __launch_bounds__(64) void k_vlb_terms(TopoDev tp, VlbPtrs vp, LossCfg lc, const float* __restrict__ t_int,
                                                              const float* __restrict__ gamma, const float* __restrict__ snr,
                                                              double delta_log_px, int B, float* __restrict__ nll,
                                                              float* __restrict__ terms) {
    const int sb = blockIdx.x, lane = threadIdx.x, K = tp.n_obj;
    const int b = tp.node_tidx[tp.sample_ptr[sb]];                        // row of t_int / nll this sample belongs to
    const float w = snr[table_index(t_int[b], lc.T)];
    const float gm_0 = gamma[0];
    const float sigma0 = sqrtf(sigmoid_f(gm_0));
    const double s_cat = (double)(sigma0 * lc.norm_value[1]), s_chg = (double)(sigma0 * lc.norm_value[2]);
    double total = 0.0;
    int n_nodes = 0;
    for (int k = 0; k < K; ++k) {
        const int q = sb * K + k, g0 = tp.grp_ptr[q], g1 = tp.grp_ptr[q + 1], nf = vp.node_nf[k], ncat = nf - 4;
        const int ncol = lc.pos_only ? 3 : nf;                            // pos_only: the feature outputs are zeroed before the loss (:212-215)
        double e_t = 0.0, e_0 = 0.0, l_cat = 0.0, l_chg = 0.0;
        for (int i = g0 + lane; i < g1; i += 64) {
            const int row = tp.node_row[i];
            const size_t o = (size_t)row * nf;
            for (int c = 0; c < nf; ++c) {
                const float d = vp.eps_t[k][o + c] - (c < ncol ? vp.net_t[k][o + c] : 0.f);
                e_t += (double)d * (double)d;
            }
            for (int c = 0; c < 3; ++c) {
                const float d = vp.eps_0[k][o + c] - vp.net_0[k][o + c];
                e_0 += (double)d * (double)d;
            }
            // log p(h | z_0), en_diffusion.py:389-449 (discretised Gaussians), on every atom of every sample
            const float* Z = vp.z_0[k] + o;
            double lpv[16], mx = -1.0e300;
            for (int j = 0; j < ncat && j < 16; ++j) {
                const double cen = ((double)Z[3 + j] * (double)lc.norm_value[1] + (double)lc.norm_bias[1]) - 1.0;
                lpv[j] = log(gauss_cdf_d((cen + 0.5) / s_cat) - gauss_cdf_d((cen - 0.5) / s_cat) + 1e-10);
                mx = fmax(mx, lpv[j]);
            }
            double se = 0.0;
            for (int j = 0; j < ncat && j < 16; ++j) se += exp(lpv[j] - mx);
            const double lse = mx + log(se);
            for (int j = 0; j < ncat && j < 16; ++j) l_cat += (lpv[j] - lse) * (double)vp.one_hot[k][(size_t)row * ncat + j];
            const float est = truncf(Z[nf - 1] * lc.norm_value[2] + lc.norm_bias[2]);          // .long(): truncation, as the reference does
            const double cc = (double)((float)vp.charge[k][row] - est);
            l_chg += log(gauss_cdf_d((cc + 0.5) / s_chg) - gauss_cdf_d((cc - 0.5) / s_chg) + 1e-10);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            e_t += __shfl_xor(e_t, d, 64); e_0 += __shfl_xor(e_0, d, 64);
            l_cat += __shfl_xor(l_cat, d, 64); l_chg += __shfl_xor(l_chg, d, 64);
        }
        const int size = g1 - g0;
        n_nodes += size;
        const double width = lc.pos_only ? 3.0 : 3.0 + (double)nf;        // pl_trainer.py:236-244: (pos_dim + node_nf) * size
        const double err_n = size > 0 ? e_t / (width * (double)size) * (double)lc.scale[k] : 0.0;
        const double l0x = 0.5 * e_0, l0c = -l_cat, l0q = -l_chg;         // exact zeros for an empty group: nothing was summed
        total += -0.5 * (double)lc.T * (double)w * e_t + (l0x + l0c + l0q);
        if (lane == 0) {
            terms[(size_t)k * B + b] = (float)err_n;
            terms[(size_t)(K + k) * B + b] = (float)e_t;
            terms[(size_t)(2 * K + k) * B + b] = (float)l0x;
            terms[(size_t)(3 * K + k) * B + b] = size > 0 ? (float)l0c : 0.f;      // (-0.0 of an empty sum -> +0)
            terms[(size_t)(4 * K + k) * B + b] = size > 0 ? (float)l0q : 0.f;
        }
    }
    // -(dof (-(gamma_0 / 2) - log(2 pi) / 2)), dof = (atoms of the sample - 1) * 3
    const double nlc = -((double)((n_nodes - 1) * 3) * (-0.5 * (double)gm_0 - 0.5 * 1.8378770664093454836));
    if (lane == 0) {
        terms[(size_t)(5 * K) * B + b] = w;
        terms[(size_t)(5 * K + 1) * B + b] = (float)nlc;
        nll[b] = (float)(total + nlc - delta_log_px);
    }
}
