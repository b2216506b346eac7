// The float64 geometry block alone: k_geom, k_edge_geo, k_active_list, k_rbf and k_fill_edges (csrc/oard_kernels.h), launched as
// forward_impl launches them (oard_hip.hip) on tables the caller lays out.  TEST INFRASTRUCTURE (tests/test_geometry_block.py compiles
// it with hipcc and loads it with ctypes, local symbol scope).  Nothing in the product builds or loads it.  The caller has checked
// every index of every table against the buffer sizes: nothing is checked again here.
#include <algorithm>
#include <cstring>
#include "../../oareactdiff_amd/csrc/oard_kernels.h"

#define GEOM_TRY(x) do { if ((x) != hipSuccess) return OARD_EHIP; } while (0)
#define GEOM_LAUNCH(kern, grid, block, stream, ...) do { \
    hipLaunchKernelGGL(kern, dim3((unsigned)(grid)), dim3(block), 0, stream, __VA_ARGS__); GEOM_TRY(hipGetLastError()); } while (0)

static long long cdiv_ll(long long a, long long b) { return (a + b - 1) / b; }

// flags & 1: the training-mode form - k_edge_geo without block counts, no k_active_list.
// flags & 2: no radial basis and no edge state (k_rbf and k_fill_edges are not launched; H and R are not read).
extern "C" int geometry_block(int N, int B, int n_groups, long long A, long long E,
                              const int* grp_ptr, const int* node_sample, const int* sample_ptr, const int* node_ref,
                              const int* act_src, const int* act_tgt, const float* pos, double cutoff,
                              double* pf64, float* pf32, float* x1, float* pp0, int* labels, float* geo, double* d64,
                              int* blk_cnt, int* al_rows, int* al_src, int* al_pre, int* al_n,
                              const float* means, const float* betas, const float* c0row, float* rbuf, float* ew,
                              int H, int R, int flags, void* stream) {
    if (N < 1 || n_groups < 1 || A < 0 || E < A) return OARD_EINVAL;
    TopoDev tp;
    memset(&tp, 0, sizeof(tp));
    tp.N = N; tp.B = B; tp.n_groups = n_groups; tp.A = A; tp.E = E;
    tp.grp_ptr = grp_ptr; tp.node_sample = node_sample; tp.sample_ptr = sample_ptr; tp.node_ref = node_ref;
    tp.act_src = act_src; tp.act_tgt = act_tgt;
    hipStream_t st = (hipStream_t)stream;
    const bool use_al = !(flags & 1), radial = !(flags & 2);
    GEOM_LAUNCH(k_geom, n_groups, 64, st, tp, pos, cutoff, pf64, pf32, x1, pp0, labels);
    if (radial) {
        const RDims D(H, R);
        GEOM_LAUNCH(k_fill_edges, std::min<long long>(cdiv_ll((E - A + 1) * (D.WP / 4), 256), 8192), 256, st,
                    c0row, ew + (size_t)A * D.WP, E - A + 1, D.WP);
    }
    if (A > 0) {
        GEOM_LAUNCH(k_edge_geo, cdiv_ll(A, 256), 256, st, tp, pos, (const double*)pf64, cutoff, geo, d64, use_al ? blk_cnt : nullptr);
        if (use_al) GEOM_LAUNCH(k_active_list, cdiv_ll(A, 256), 256, st, tp, (const float*)geo, (const int*)blk_cnt, al_rows, al_src, al_pre, al_n);
        if (radial) {
            const RDims D(H, R);
            GEOM_LAUNCH(k_rbf, cdiv_ll(A * D.RP, 256), 256, st, tp, (const double*)d64, (const float*)geo, means, betas, cutoff,
                        rbuf, ew, D.R, D.RP, D.H, D.WP);
        }
    }
    GEOM_TRY(hipStreamSynchronize(st));
    return OARD_OK;
}
