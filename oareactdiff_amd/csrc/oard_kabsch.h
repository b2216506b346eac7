// oard_kabsch.h — optimal-superposition RMSD per segment (the validation metric of the trainer).
//
// Replaces the same-order branch of the reference's RMSD (oa_reactdiff/analyze/rmsd.py:30-35: pymatgen's KabschMatcher) and its
// chirality handling (:66-74: the z-mirrored structure is fitted too and the smaller RMSD kept), per molecule of a batch
// (batch_rmsd, :78-100).  Rows are compared in the order given; the permutation search of rmsd_core's other branch (:36-51) is
// k_matched_rmsd (csrc/oard_match.h), which builds on kabsch_rotation below.
//
// One wavefront per segment, no LDS, no scratch, no topology: a segment is rows seg_ptr[g] .. seg_ptr[g + 1] of two row-major float32
// arrays whose first three columns are the coordinates (row strides lda / ldb in elements), so the [n, node_nf] tensors of the samplers
// are read where they lie.  Everything after the loads is float64:
//   1. centroids c_a, c_b and the cross-covariance S = sum (b - c_b)(a - c_a)^T: lane-strided partial sums in ascending rows, then
//      wave_sum_f64 (a fixed butterfly: every lane ends with the same bits, and they depend on the segment alone);
//   2. Horn's symmetric 4 x 4 matrix of S, diagonalised by cyclic Jacobi (every lane runs the same 4 x 4 problem redundantly; the
//      (p, q) pairs of a sweep are unrolled, so every matrix index is a compile-time constant and the two matrices stay in registers);
//      the eigenvector of the largest eigenvalue is the unit quaternion of the rotation R taking centred b onto centred a.  Jacobi
//      rather than QCP's Newton iteration on the characteristic polynomial: it returns an orthonormal basis whatever the spectrum, so
//      n = 1, n = 2, collinear, coplanar and identical structures (repeated or zero eigenvalues; R not unique, the RMSD unique) need
//      no special case;
//   3. the RMSD from a second pass over the rows, sqrt(sum |R (b - c_b) - (a - c_a)|^2 / n) - not (G_a + G_b - 2 lambda) / n, which
//      cancels catastrophically for near-identical structures;
//   4. flags bit 0: steps 2 and 3 again for the mirror image of b (z of the centred b negated: only the sign of S's last row changes,
//      so no further pass forms it); the smaller RMSD is kept, with the improper map R' diag(1, 1, -1) (a tie keeps the rotation).
// Special segments: empty -> NaN; any non-finite coordinate -> cap if cap > 0 else NaN (the reference's `except: rmsd = 1.0`); with
// a cap the result is min(rmsd, cap) (its `min(rmsd, 1.0)`).  Their rot / aligned entries are NaN.
// The kernel is one call of kabsch_body, which k_pairwise_kabsch (csrc/oard_pairwise.h) calls too, with two members of one array.
#pragma once
#include "oard_kernels.h"

#define KABSCH_SWEEPS 10      // cyclic Jacobi on a symmetric 4 x 4 converges quadratically: 5 - 6 sweeps reach 1e-16; the rest are no-ops

// One Jacobi rotation in the (P, Q) plane: A <- J^T A J, V <- V J.  The angle is guarded: an exactly zero off-diagonal element rotates
// by nothing (t = 0; this also covers 0 / 0 when the two diagonal elements are equal), and a tiny one gives theta = +-inf -> t = 0.
template <int P, int Q>
OARD_DEV void kabsch_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = (apq != 0.0 && t == t) ? t : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                  // columns P and Q
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                  // rows P and Q
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
    }
}

// S[i][j] = sum b_i a_j (centred) -> R (row-major) with R b ~ a: Horn (1987), the quaternion of the largest eigenvalue of N(S).
// Returns that eigenvalue (k_matched_rmsd ranks permutations by it, csrc/oard_match.h).
OARD_DEV double kabsch_rotation(const double (&S)[3][3], double (&R)[3][3]) {
    double A[4][4], V[4][4];
    A[0][0] = S[0][0] + S[1][1] + S[2][2];
    A[1][1] = S[0][0] - S[1][1] - S[2][2];
    A[2][2] = -S[0][0] + S[1][1] - S[2][2];
    A[3][3] = -S[0][0] - S[1][1] + S[2][2];
    A[0][1] = A[1][0] = S[1][2] - S[2][1];
    A[0][2] = A[2][0] = S[2][0] - S[0][2];
    A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0];
    A[1][3] = A[3][1] = S[2][0] + S[0][2];
    A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < KABSCH_SWEEPS; ++sweep) {
        kabsch_rotate<0, 1>(A, V); kabsch_rotate<0, 2>(A, V); kabsch_rotate<0, 3>(A, V);
        kabsch_rotate<1, 2>(A, V); kabsch_rotate<1, 3>(A, V); kabsch_rotate<2, 3>(A, V);
    }
    // the column of the largest eigenvalue, picked with selects (a run-time column index would put V into scratch)
    double lam = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = A[k][k] > lam;
        lam = up ? A[k][k] : lam;
        w = up ? V[0][k] : w; x = up ? V[1][k] : x; y = up ? V[2][k] : y; z = up ? V[3][k] : z;
    }
    const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= inv; x *= inv; y *= inv; z *= inv;
    R[0][0] = w * w + x * x - y * y - z * z; R[0][1] = 2.0 * (x * y - w * z); R[0][2] = 2.0 * (x * z + w * y);
    R[1][0] = 2.0 * (x * y + w * z); R[1][1] = w * w - x * x + y * y - z * z; R[1][2] = 2.0 * (y * z - w * x);
    R[2][0] = 2.0 * (x * z - w * y); R[2][1] = 2.0 * (y * z + w * x); R[2][2] = w * w - x * x - y * y + z * z;
    return lam;
}

// One value into its output slot(s): a caller with two (the [i, j] and [j, i] entries of a pair matrix, csrc/oard_pairwise.h) gets the same
// bits in both; p2 / s / s2 may be null.
OARD_DEV void kabsch_store(float* p, float* p2, float v, int* s, int* s2, int code) {
    *p = v;
    if (p2 != nullptr) *p2 = v;
    if (s != nullptr) *s = code;
    if (s2 != nullptr) *s2 = code;
}

// The body of k_kabsch_rmsd for ONE segment, shared with k_pairwise_kabsch (csrc/oard_pairwise.h): A / B are the first rows of the target
// and of the structure fitted onto it, n the rows of both.  rmsd (and rmsd2, status, status2 if not null) are the slots of this segment;
// rot its nine floats, aligned its n rows (or null).  The status written is 0, or 4 for a non-finite coordinate (oard_match.h's code).
OARD_DEV void kabsch_body(const float* A, long long lda, const float* B, long long ldb, int n, int lane, int flags, float cap, float* rmsd,
                          float* rmsd2, int* status, int* status2, float* rot, float* aligned) {
    const float fnan = __builtin_nanf("");
    if (n <= 0) {
        if (lane == 0) kabsch_store(rmsd, rmsd2, fnan, status, status2, 0);
        if (rot != nullptr && lane < 9) rot[lane] = fnan;
        return;
    }
    // ---- pass 1: centroids, and is every coordinate finite ----------------------------------------
    double ca0 = 0, ca1 = 0, ca2 = 0, cb0 = 0, cb1 = 0, cb2 = 0;
    bool bad = false;
    for (int k = lane; k < n; k += 64) {
        const float* pa = A + (size_t)k * (size_t)lda;
        const float* pb = B + (size_t)k * (size_t)ldb;
        const float a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
        bad = bad || !(isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(b0) && isfinite(b1) && isfinite(b2));
        ca0 += (double)a0; ca1 += (double)a1; ca2 += (double)a2;
        cb0 += (double)b0; cb1 += (double)b1; cb2 += (double)b2;
    }
    if (__any(bad ? 1 : 0)) {
        if (lane == 0) kabsch_store(rmsd, rmsd2, cap > 0.f ? cap : fnan, status, status2, 4);
        if (rot != nullptr && lane < 9) rot[lane] = fnan;
        if (aligned != nullptr)
            for (int k = lane; k < n; k += 64) {
                float* o = aligned + (size_t)k * 3;
                o[0] = fnan; o[1] = fnan; o[2] = fnan;
            }
        return;
    }
    const double inv = 1.0 / (double)n;
    ca0 = wave_sum_f64(ca0) * inv; ca1 = wave_sum_f64(ca1) * inv; ca2 = wave_sum_f64(ca2) * inv;
    cb0 = wave_sum_f64(cb0) * inv; cb1 = wave_sum_f64(cb1) * inv; cb2 = wave_sum_f64(cb2) * inv;
    // ---- pass 2: S = sum (b - c_b)(a - c_a)^T -------------------------------------------------------
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = lane; k < n; k += 64) {
        const float* pa = A + (size_t)k * (size_t)lda;
        const float* pb = B + (size_t)k * (size_t)ldb;
        const double x0 = (double)pa[0] - ca0, x1 = (double)pa[1] - ca1, x2 = (double)pa[2] - ca2;
        const double y0 = (double)pb[0] - cb0, y1 = (double)pb[1] - cb1, y2 = (double)pb[2] - cb2;
        S[0][0] += y0 * x0; S[0][1] += y0 * x1; S[0][2] += y0 * x2;
        S[1][0] += y1 * x0; S[1][1] += y1 * x1; S[1][2] += y1 * x2;
        S[2][0] += y2 * x0; S[2][1] += y2 * x1; S[2][2] += y2 * x2;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = wave_sum_f64(S[i][j]);
    // ---- the rotation, its residual; then the same for the mirror image of b ----------------------
    double best = 0.0, M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};      // M: the kept map on centred b (R, or R' diag(1, 1, -1))
    const int tries = (flags & 1) ? 2 : 1;
#pragma unroll 1
    for (int m = 0; m < tries; ++m) {
        const double sz = m == 0 ? 1.0 : -1.0;     // sign of the centred b's z column
        double Sm[3][3], R[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { Sm[0][j] = S[0][j]; Sm[1][j] = S[1][j]; Sm[2][j] = sz * S[2][j]; }
        kabsch_rotation(Sm, R);
#pragma unroll
        for (int i = 0; i < 3; ++i) R[i][2] *= sz; // fold the mirror in: R' diag(1, 1, sz) acts on the un-mirrored centred b
        double e = 0.0;
        for (int k = lane; k < n; k += 64) {
            const float* pa = A + (size_t)k * (size_t)lda;
            const float* pb = B + (size_t)k * (size_t)ldb;
            const double x0 = (double)pa[0] - ca0, x1 = (double)pa[1] - ca1, x2 = (double)pa[2] - ca2;
            const double y0 = (double)pb[0] - cb0, y1 = (double)pb[1] - cb1, y2 = (double)pb[2] - cb2;
            const double d0 = R[0][0] * y0 + R[0][1] * y1 + R[0][2] * y2 - x0;
            const double d1 = R[1][0] * y0 + R[1][1] * y1 + R[1][2] * y2 - x1;
            const double d2 = R[2][0] * y0 + R[2][1] * y1 + R[2][2] * y2 - x2;
            e += d0 * d0 + d1 * d1 + d2 * d2;
        }
        e = sqrt(wave_sum_f64(e) * inv);
        const bool keep = m == 0 || e < best;      // wave-uniform: every lane holds the same bits
        best = keep ? e : best;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) M[i][j] = keep ? R[i][j] : M[i][j];
    }
    // ---- outputs: `aligned` applies the map as `rot` returns it, i.e. rounded to float32 ---------
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = (double)(float)M[i][j];
    if (lane == 0) {
        float r = (float)best;
        if (cap > 0.f) r = fminf(r, cap);
        kabsch_store(rmsd, rmsd2, r, status, status2, 0);
        if (rot != nullptr) {
            float* o = rot;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) o[i * 3 + j] = (float)M[i][j];
        }
    }
    if (aligned != nullptr)
        for (int k = lane; k < n; k += 64) {
            const float* pb = B + (size_t)k * (size_t)ldb;
            const double y0 = (double)pb[0] - cb0, y1 = (double)pb[1] - cb1, y2 = (double)pb[2] - cb2;
            float* o = aligned + (size_t)k * 3;
            o[0] = (float)(M[0][0] * y0 + M[0][1] * y1 + M[0][2] * y2 + ca0);
            o[1] = (float)(M[1][0] * y0 + M[1][1] * y1 + M[1][2] * y2 + ca1);
            o[2] = (float)(M[2][0] * y0 + M[2][1] * y1 + M[2][2] * y2 + ca2);
        }
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_kabsch_rmsd(const float* __restrict__ a, long long lda, const float* __restrict__ b,
                                                                long long ldb, const int* __restrict__ seg_ptr, int flags, float cap,
                                                                float* __restrict__ rmsd, float* __restrict__ rot,
                                                                float* __restrict__ aligned) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const long long r0 = seg_ptr[g];
    const int n = (int)((long long)seg_ptr[g + 1] - r0);
    const size_t row = n > 0 ? (size_t)r0 : 0;              // an empty segment reads nothing: no address is formed from its r0
    kabsch_body(a + row * (size_t)lda, lda, b + row * (size_t)ldb, ldb, n, lane, flags, cap, rmsd + g, nullptr, nullptr, nullptr,
                rot != nullptr ? rot + (size_t)g * 9 : nullptr, aligned != nullptr ? aligned + row * 3 : nullptr);
}
