// oard_match.h — order-matched RMSD per segment: the permutation search of the reference's rmsd_core (oa_reactdiff/analyze/rmsd.py:36-51)
// in front of the optimal superposition of oard_kabsch.h.
//
// M(a, b) = min over the permutations pi that map every row of a to a row of b of the same species, and with flags bit 0 over the z-mirror
// image of b too, of the optimal-superposition RMSD of a against b[pi].  pymatgen's matchers are not emulated (the genetic matcher's
// threshold and the Hungarian matcher's axis heuristics define no function of the inputs); the two things the reference does define are:
//   EXACT  (status 0): prod c_s! < exact_limit (c_s = rows of species s; the reference's `< 1e4`).  Every permutation is evaluated:
//          lanes take permutation indices lane-strided, decode them in the mixed factorial radix of the species blocks, form
//          S = sum b[pi(k)] a[k]^T from LDS and rank by the largest eigenvalue of Horn's matrix (kabsch_rotation's; every lane runs its
//          own 4 x 4 problem); a fixed-order wave reduction keeps the largest, ties to the lowest index (index 0 = the order given).
//   SEARCH (status 1): otherwise.  Alternate assignment and superposition from five starts per chirality - the same-order Kabsch
//          rotation, then the four proper alignments of the principal axes of the two centred clouds (3 x 3 cyclic Jacobi, eigenvectors
//          by ascending eigenvalue, signs (+,+,+), (+,-,-), (-,+,-), (-,-,+)):  pi := the minimum-cost assignment per species block for
//          the cost |a_i - R b_j|^2 (shortest augmenting paths, Jonker-Volgenant: lanes are columns, costs on the fly from LDS, the
//          column minimum a wave arg-min, the lowest column winning ties);  R := Kabsch(a, b[pi]);  until pi repeats or MATCH_ROUNDS
//          assignments were made.  The smallest RMSD over all starts is kept (a tie keeps the earlier start).  The objective never rises
//          along a run and the first start begins at the fit of the order given, so  M <= result <= same-order RMSD.
// In both branches the RMSD returned is the residual of a pass over the rows with the winning permutation and rotation (not
// G_a + G_b - 2 lambda, which cancels for near-identical structures).
//
// One wavefront per segment, float64 after the loads, no topology.  The centred rows live in LDS SORTED by (species, row), a and b each
// in its own order, so a species block is one index range of both and a permutation is q[] with q[t] in t's block; ord_a / ord_b map
// sorted positions back to rows.  Every decision is taken on values that a fixed-order wave reduction left identical in all lanes and
// that depend on the segment alone: a segment's bits do not depend on what else is in the launch.
// Special segments (rot / aligned NaN, perm the identity): more than MATCH_MAX rows -> status 3; a non-finite coordinate -> status 4;
// species lists that differ as multisets -> status 2 (checked in this order); each gives cap if cap > 0 else NaN (the reference's
// `except: rmsd = 1.0`).  An empty segment gives NaN, status 0.
// The kernel is one call of matched_body, which k_pairwise_matched (csrc/oard_pairwise.h) calls too, with two members of one array.
#pragma once
#include "oard_kabsch.h"

#define MATCH_MAX 256         // rows per segment (lane-strided above 64)
#define MATCH_ROUNDS 32       // assignments per run
#define MATCH_NT 13           // blocks of two or more rows in the exact branch: 2^14 > 10 000
#define MATCH_LIMIT 10000     // the largest exact_limit

struct MatchLds {
    double x[3][MATCH_MAX], y[3][MATCH_MAX], yr[3][MATCH_MAX];     // centred a, centred b (sorted), the mapped b of the running assignment
    double u[MATCH_MAX], v[MATCH_MAX], minv[MATCH_MAX];            // row / column potentials, column slack
    int sa[MATCH_MAX], sb[MATCH_MAX], ss[MATCH_MAX], st[MATCH_MAX];   // species by row (a, b) and by sorted position (a, b)
    int ord_a[MATCH_MAX], ord_b[MATCH_MAX];                        // sorted position -> row
    int q0[MATCH_MAX], q[MATCH_MAX], qn[MATCH_MAX], qbest[MATCH_MAX];   // the order given, the running, the new and the kept permutation
    int blk[MATCH_MAX + 1];                                        // block b is sorted positions blk[b] .. blk[b + 1]
    int prow[MATCH_MAX], way[MATCH_MAX], used[MATCH_MAX];          // column -> row, column -> previous column of its path, column in the tree
    int nt_off[MATCH_NT], nt_m[MATCH_NT], nt_f[MATCH_NT];          // exact branch: the blocks of two or more rows, their m!
};

OARD_DEV int match_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// One Jacobi rotation of a symmetric 3 x 3 (the guards of kabsch_rotate).
template <int P, int Q>
OARD_DEV void match_rotate3(double (&A)[3][3], double (&V)[3][3]) {
    const double apq = A[P][Q];
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = (apq != 0.0 && t == t) ? t : 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
    }
}

template <int I, int J>
OARD_DEV void match_order2(double (&lam)[3], double (&V)[3][3]) {      // compare-exchange of two eigenpairs, with selects
    const bool sw = lam[J] < lam[I];
    const double li = lam[I], lj = lam[J];
    lam[I] = sw ? lj : li; lam[J] = sw ? li : lj;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vi = V[k][I], vj = V[k][J];
        V[k][I] = sw ? vj : vi; V[k][J] = sw ? vi : vj;
    }
}

// Principal axes of sum c c^T over the n sorted rows of c: the columns of V, by ascending eigenvalue, det V = +1.
OARD_DEV void match_axes(const double (&c)[3][MATCH_MAX], int n, int lane, double (&V)[3][3]) {
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int t = lane; t < n; t += 64) {
        const double c0 = c[0][t], c1 = c[1][t], c2 = c[2][t];
        A[0][0] += c0 * c0; A[0][1] += c0 * c1; A[0][2] += c0 * c2; A[1][1] += c1 * c1; A[1][2] += c1 * c2; A[2][2] += c2 * c2;
    }
    A[0][0] = wave_sum_f64(A[0][0]); A[0][1] = wave_sum_f64(A[0][1]); A[0][2] = wave_sum_f64(A[0][2]);
    A[1][1] = wave_sum_f64(A[1][1]); A[1][2] = wave_sum_f64(A[1][2]); A[2][2] = wave_sum_f64(A[2][2]);
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[2][1] = A[1][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < KABSCH_SWEEPS; ++sweep) {
        match_rotate3<0, 1>(A, V); match_rotate3<0, 2>(A, V); match_rotate3<1, 2>(A, V);
    }
    double lam[3] = {A[0][0], A[1][1], A[2][2]};
    match_order2<0, 1>(lam, V); match_order2<1, 2>(lam, V); match_order2<0, 1>(lam, V);
    const double det = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                       V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    const double f = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) V[k][2] *= f;
}

// Digit d of [0, m!) -> a permutation of 0 .. m - 1 (m <= 7) as nibbles, position t in bits 4t: the Fisher-Yates decode, d = 0 the identity.
OARD_DEV unsigned match_decode(int d, int m) {
    unsigned L = 0x76543210u;
    for (int t = m - 1; t >= 1; --t) {
        const int j = t - d % (t + 1);
        d /= t + 1;
        const unsigned x = ((L >> (4 * t)) ^ (L >> (4 * j))) & 15u;
        L ^= (x << (4 * t)) | (x << (4 * j));
    }
    return L;
}

// The minimum-cost assignment of one species block (sorted positions o .. o + m, m >= 2) for the cost |x_row - yr_col|^2 -> qn.
// Shortest augmenting paths with potentials; lanes are columns; column -1 is the root of the tree (its row is the one being inserted).
OARD_DEV void match_assign_block(MatchLds& L, int o, int m, int lane) {
    const double inf = __builtin_huge_val();
    for (int c = lane; c < m; c += 64) { L.u[c] = 0.0; L.v[c] = 0.0; L.prow[c] = -1; }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < m; ++i) {
        for (int c = lane; c < m; c += 64) { L.minv[c] = inf; L.used[c] = 0; }
        __syncthreads();
        int j0 = -1, i0 = i;
#pragma unroll 1
        for (int step = 0; step < m; ++step) {               // a path visits every column at most once
            const double x0 = L.x[0][o + i0], x1 = L.x[1][o + i0], x2 = L.x[2][o + i0], ui = L.u[i0];
            double best = inf;
            int bestc = 0x7fffffff;
            for (int c = lane; c < m; c += 64) {
                if (L.used[c]) continue;
                const double d0 = x0 - L.yr[0][o + c], d1 = x1 - L.yr[1][o + c], d2 = x2 - L.yr[2][o + c];
                const double cur = d0 * d0 + d1 * d1 + d2 * d2 - ui - L.v[c];
                double mv = L.minv[c];
                if (cur < mv) { mv = cur; L.minv[c] = cur; L.way[c] = j0; }
                if (mv < best) { best = mv; bestc = c; }     // ascending c: the lowest column of the lane wins a tie
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double ob = __shfl_xor(best, d, 64);
                const int oc = __shfl_xor(bestc, d, 64);
                const bool take = ob < best || (ob == best && oc < bestc);
                best = take ? ob : best; bestc = take ? oc : bestc;
            }
            const int j1 = match_uniform(bestc);
            if (j1 < 0 || j1 >= m) break;                    // cannot happen with finite costs: leave rather than index outside the block
            const double delta = best;
            for (int c = lane; c < m; c += 64) {
                if (L.used[c]) { L.u[L.prow[c]] += delta; L.v[c] -= delta; }
                else L.minv[c] -= delta;
            }
            __syncthreads();
            if (lane == 0) { L.u[i] += delta; L.used[j1] = 1; }
            __syncthreads();
            j0 = j1;
            i0 = match_uniform(L.prow[j0]);
            if (i0 < 0) break;
        }
        // augment: walk the path back to the root, every column takes the row of the column before it
#pragma unroll 1
        for (int step = 0; step < m && j0 >= 0; ++step) {
            const int j1 = match_uniform(L.way[j0]);
            const int r = j1 < 0 ? i : match_uniform(L.prow[j1 < 0 ? 0 : j1]);
            if (lane == 0) L.prow[j0] = r;
            j0 = j1 < m ? j1 : -1;
        }
        __syncthreads();
    }
    for (int c = lane; c < m; c += 64) {
        const int r = L.prow[c];
        if (r >= 0 && r < m) L.qn[o + r] = o + c;
    }
    __syncthreads();
}

// The body of k_matched_rmsd for ONE segment, shared with k_pairwise_matched (csrc/oard_pairwise.h): A / B and SA / SB are the first rows
// and species of the target and of the structure fitted onto it, nl the rows of both, L the workgroup's LDS.  rmsd (and rmsd2, status,
// status2 if not null) are the slots of this segment, rot its nine floats, aligned / perm its nl rows (or null); perm holds row0 + the
// row inside the segment.
OARD_DEV void matched_body(MatchLds& L, const float* A, long long lda, const float* B, long long ldb, const int* SA, const int* SB,
                           long long nl, long long row0, int lane, int flags, float cap, int exact_limit, float* rmsd, float* rmsd2,
                           int* status, int* status2, float* rot, float* aligned, int* perm) {
    const float fnan = __builtin_nanf("");
    if (nl <= 0) {
        if (lane == 0) kabsch_store(rmsd, rmsd2, fnan, status, status2, 0);
        if (rot != nullptr && lane < 9) rot[lane] = fnan;
        return;
    }
    // a special segment: the status, cap or NaN, NaN maps, the identity permutation (nl rows: also more than MATCH_MAX of them)
    auto special = [&](int code) {
        if (lane == 0) kabsch_store(rmsd, rmsd2, cap > 0.f ? cap : fnan, status, status2, code);
        if (rot != nullptr && lane < 9) rot[lane] = fnan;
        for (long long k = lane; k < nl; k += 64) {
            if (aligned != nullptr) { float* o = aligned + (size_t)k * 3; o[0] = fnan; o[1] = fnan; o[2] = fnan; }
            if (perm != nullptr) perm[k] = (int)(row0 + k);
        }
    };
    if (nl > MATCH_MAX) { special(3); return; }
    const int n = (int)nl;
    // ---- pass 1: centroids, is every coordinate finite, the species into LDS ---------------------------
    double ca0 = 0, ca1 = 0, ca2 = 0, cb0 = 0, cb1 = 0, cb2 = 0;
    bool bad = false;
    for (int k = lane; k < n; k += 64) {
        const float* pa = A + (size_t)k * (size_t)lda;
        const float* pb = B + (size_t)k * (size_t)ldb;
        const float a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
        bad = bad || !(isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(b0) && isfinite(b1) && isfinite(b2));
        ca0 += (double)a0; ca1 += (double)a1; ca2 += (double)a2;
        cb0 += (double)b0; cb1 += (double)b1; cb2 += (double)b2;
        L.sa[k] = SA[k]; L.sb[k] = SB[k];
    }
    if (__any(bad ? 1 : 0)) { special(4); return; }
    const double inv = 1.0 / (double)n;
    ca0 = wave_sum_f64(ca0) * inv; ca1 = wave_sum_f64(ca1) * inv; ca2 = wave_sum_f64(ca2) * inv;
    cb0 = wave_sum_f64(cb0) * inv; cb1 = wave_sum_f64(cb1) * inv; cb2 = wave_sum_f64(cb2) * inv;
    __syncthreads();
    // ---- sort by (species, row): the rank of a row is the number of rows before it -------------------
    for (int k = lane; k < n; k += 64) {
        const int sa = L.sa[k], sb = L.sb[k];
        int ra = 0, rb = 0;
        for (int j = 0; j < n; ++j) {
            const int ja = L.sa[j], jb = L.sb[j];
            ra += (ja < sa || (ja == sa && j < k)) ? 1 : 0;
            rb += (jb < sb || (jb == sb && j < k)) ? 1 : 0;
        }
        const float* pa = A + (size_t)k * (size_t)lda;
        const float* pb = B + (size_t)k * (size_t)ldb;
        L.x[0][ra] = (double)pa[0] - ca0; L.x[1][ra] = (double)pa[1] - ca1; L.x[2][ra] = (double)pa[2] - ca2;
        L.y[0][rb] = (double)pb[0] - cb0; L.y[1][rb] = (double)pb[1] - cb1; L.y[2][rb] = (double)pb[2] - cb2;
        L.ord_a[ra] = k; L.ord_b[rb] = k; L.ss[ra] = sa; L.st[rb] = sb;
        L.q0[ra] = rb;                                     // the order given (species preserving iff the two lists are equal row by row)
    }
    __syncthreads();
    bool differ = false;
    for (int t = lane; t < n; t += 64) differ = differ || L.ss[t] != L.st[t];
    if (__any(differ ? 1 : 0)) { special(2); return; }
    // ---- the blocks, and the number of species-preserving permutations (saturating) -----------------
    int nblk = 0;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        const bool start = t < n && (t == 0 || L.ss[t] != L.ss[t - 1]);
        const unsigned long long mask = __ballot(start ? 1 : 0);
        if (start) L.blk[nblk + __popcll(mask & ((1ull << lane) - 1ull))] = t;
        nblk += __popcll(mask);
    }
    nblk = match_uniform(nblk);
    if (lane == 0) L.blk[nblk] = n;
    __syncthreads();
    int count = 1, nnt = 0;                                // count saturates above MATCH_LIMIT
#pragma unroll 1
    for (int bk = 0; bk < nblk; ++bk) {
        const int o = match_uniform(L.blk[bk]), m = match_uniform(L.blk[bk + 1]) - o;
        if (m < 2) continue;
        int f = 1;
        for (int k = 2; k <= m && f <= MATCH_LIMIT; ++k) f *= k;
        count = (f > MATCH_LIMIT || count > MATCH_LIMIT) ? MATCH_LIMIT + 1 : min(count * f, MATCH_LIMIT + 1);
        if (nnt < MATCH_NT && lane == 0) { L.nt_off[nnt] = o; L.nt_m[nnt] = m; L.nt_f[nnt] = f; }
        nnt += 1;
    }
    __syncthreads();
    const int tries = (flags & 1) ? 2 : 1;
    const bool exact = exact_limit > 0 && count < exact_limit && nnt <= MATCH_NT;      // count < 10 000: m <= 7 in every block
    int exact_m = 0;                                       // exact branch: the chirality of the winner
    if (exact) {
        // S of the blocks of one row, which every permutation shares
        double F[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int t = lane; t < n; t += 64) {
            const int s = L.ss[t];
            const bool single = (t == 0 || L.ss[t - 1] != s) && (t == n - 1 || L.ss[t + 1] != s);
            const double w = single ? 1.0 : 0.0;
            const double x0 = w * L.x[0][t], x1 = w * L.x[1][t], x2 = w * L.x[2][t], y0 = L.y[0][t], y1 = L.y[1][t], y2 = L.y[2][t];
            F[0][0] += y0 * x0; F[0][1] += y0 * x1; F[0][2] += y0 * x2;
            F[1][0] += y1 * x0; F[1][1] += y1 * x1; F[1][2] += y1 * x2;
            F[2][0] += y2 * x0; F[2][1] += y2 * x1; F[2][2] += y2 * x2;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) F[i][j] = wave_sum_f64(F[i][j]);
        const int total = count * tries;
        double blam = -__builtin_huge_val();
        int bidx = 0x7fffffff;
#pragma unroll 1
        for (int idx = lane; idx < total; idx += 64) {
            const int mir = idx >= count ? 1 : 0;
            int rem = idx - mir * count;
            double S[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) S[i][j] = F[i][j];
            for (int bk = 0; bk < nnt; ++bk) {
                const int o = L.nt_off[bk], m = L.nt_m[bk], f = L.nt_f[bk];
                const unsigned P = match_decode(rem % f, m);
                rem /= f;
                for (int t = 0; t < m; ++t) {
                    const int c = o + (int)((P >> (4 * t)) & 15u);
                    const double x0 = L.x[0][o + t], x1 = L.x[1][o + t], x2 = L.x[2][o + t], y0 = L.y[0][c], y1 = L.y[1][c], y2 = L.y[2][c];
                    S[0][0] += y0 * x0; S[0][1] += y0 * x1; S[0][2] += y0 * x2;
                    S[1][0] += y1 * x0; S[1][1] += y1 * x1; S[1][2] += y1 * x2;
                    S[2][0] += y2 * x0; S[2][1] += y2 * x1; S[2][2] += y2 * x2;
                }
            }
            const double sz = mir ? -1.0 : 1.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) S[2][j] *= sz;
            double R[3][3];
            const double lam = kabsch_rotation(S, R);
            if (lam > blam) { blam = lam; bidx = idx; }      // ascending idx: the lowest index of the lane wins a tie
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ol = __shfl_xor(blam, d, 64);
            const int oi = __shfl_xor(bidx, d, 64);
            const bool take = ol > blam || (ol == blam && oi < bidx);
            blam = take ? ol : blam; bidx = take ? oi : bidx;
        }
        int win = match_uniform(bidx);
        win = (win >= 0 && win < total) ? win : 0;
        exact_m = win >= count ? 1 : 0;
        int rem = win - exact_m * count;
        for (int t = lane; t < n; t += 64) L.q[t] = t;      // blocks of one row
        __syncthreads();
        for (int bk = 0; bk < nnt; ++bk) {
            const int o = L.nt_off[bk], m = L.nt_m[bk], f = L.nt_f[bk];
            const unsigned P = match_decode(rem % f, m);
            rem /= f;
            if (lane < m) L.q[o + lane] = o + (int)((P >> (4 * lane)) & 15u);
        }
        __syncthreads();
    }
    // ---- the runs: exact = one fit of the winner; search = tries x 5 starts of alternating assignment and fit ------------------------
    double Va[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Vb[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (!exact) { match_axes(L.x, n, lane, Va); match_axes(L.y, n, lane, Vb); }
    const int runs = exact ? 1 : 5 * tries, rounds = exact ? 0 : MATCH_ROUNDS;
    double best = 0.0, M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};        // M: the kept map on the centred b (mirror folded in)
#pragma unroll 1
    for (int run = 0; run < runs; ++run) {
        const int mir = exact ? exact_m : run / 5, start = exact ? 0 : run % 5;
        const double sz = mir ? -1.0 : 1.0;
        double R[3][3];
        if (start == 0) {
            if (!exact) { for (int t = lane; t < n; t += 64) L.q[t] = L.q0[t]; __syncthreads(); }
        } else {
            // Va diag(s) Vb'^T with Vb' = D Vb diag(1, 1, det D) the axes of the mirrored cloud, acting on the centred b as it lies: ... D
            const double s0 = (start == 1 || start == 2) ? 1.0 : -1.0, s1 = (start == 1 || start == 3) ? 1.0 : -1.0;
            const double s2 = ((start == 1 || start == 4) ? 1.0 : -1.0) * sz;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) R[i][j] = Va[i][0] * s0 * Vb[j][0] + Va[i][1] * s1 * Vb[j][1] + Va[i][2] * s2 * Vb[j][2];
        }
        int it = 0;
#pragma unroll 1
        while (true) {
            if (start == 0 || it > 0) {                    // R := Kabsch(a, b[q]) for this chirality
                double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
                for (int t = lane; t < n; t += 64) {
                    const int c = L.q[t];
                    const double x0 = L.x[0][t], x1 = L.x[1][t], x2 = L.x[2][t], y0 = L.y[0][c], y1 = L.y[1][c], y2 = L.y[2][c];
                    S[0][0] += y0 * x0; S[0][1] += y0 * x1; S[0][2] += y0 * x2;
                    S[1][0] += y1 * x0; S[1][1] += y1 * x1; S[1][2] += y1 * x2;
                    S[2][0] += y2 * x0; S[2][1] += y2 * x1; S[2][2] += y2 * x2;
                }
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) S[i][j] = wave_sum_f64(S[i][j]);
#pragma unroll
                for (int j = 0; j < 3; ++j) S[2][j] *= sz;
                kabsch_rotation(S, R);
#pragma unroll
                for (int i = 0; i < 3; ++i) R[i][2] *= sz; // fold the mirror in: R' diag(1, 1, sz) acts on the un-mirrored centred b
            }
            if (it >= rounds) break;
            for (int t = lane; t < n; t += 64) {
                const double y0 = L.y[0][t], y1 = L.y[1][t], y2 = L.y[2][t];
                L.yr[0][t] = R[0][0] * y0 + R[0][1] * y1 + R[0][2] * y2;
                L.yr[1][t] = R[1][0] * y0 + R[1][1] * y1 + R[1][2] * y2;
                L.yr[2][t] = R[2][0] * y0 + R[2][1] * y1 + R[2][2] * y2;
            }
            __syncthreads();
#pragma unroll 1
            for (int bk = 0; bk < nblk; ++bk) {
                const int o = match_uniform(L.blk[bk]), m = match_uniform(L.blk[bk + 1]) - o;
                if (m < 2) { if (lane == 0) L.qn[o] = o; }
                else match_assign_block(L, o, m, lane);
            }
            __syncthreads();
            bool moved = false;
            for (int t = lane; t < n; t += 64) moved = moved || L.qn[t] != L.q[t];
            const bool same = !__any(moved ? 1 : 0);
            if (it > 0 && same) break;
            for (int t = lane; t < n; t += 64) L.q[t] = L.qn[t];
            __syncthreads();
            it += 1;
        }
        // the residual of this run's permutation and rotation
        double e = 0.0;
        for (int t = lane; t < n; t += 64) {
            const int c = L.q[t];
            const double y0 = L.y[0][c], y1 = L.y[1][c], y2 = L.y[2][c];
            const double d0 = R[0][0] * y0 + R[0][1] * y1 + R[0][2] * y2 - L.x[0][t];
            const double d1 = R[1][0] * y0 + R[1][1] * y1 + R[1][2] * y2 - L.x[1][t];
            const double d2 = R[2][0] * y0 + R[2][1] * y1 + R[2][2] * y2 - L.x[2][t];
            e += d0 * d0 + d1 * d1 + d2 * d2;
        }
        e = sqrt(wave_sum_f64(e) * inv);
        const bool keep = run == 0 || e < best;            // wave-uniform: every lane holds the same bits
        if (keep) {
            best = e;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) M[i][j] = R[i][j];
            for (int t = lane; t < n; t += 64) L.qbest[t] = L.q[t];
        }
        __syncthreads();
    }
    // ---- outputs: `aligned` applies the map as `rot` returns it, i.e. rounded to float32; rows in a's order ------------------------
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = (double)(float)M[i][j];
    if (lane == 0) {
        float r = (float)best;
        if (cap > 0.f) r = fminf(r, cap);
        kabsch_store(rmsd, rmsd2, r, status, status2, exact ? 0 : 1);
        if (rot != nullptr) {
            float* o = rot;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) o[i * 3 + j] = (float)M[i][j];
        }
    }
    for (int t = lane; t < n; t += 64) {
        const int c = L.qbest[t];
        const size_t row = (size_t)L.ord_a[t];
        if (perm != nullptr) perm[row] = (int)(row0 + L.ord_b[c]);
        if (aligned != nullptr) {
            const double y0 = L.y[0][c], y1 = L.y[1][c], y2 = L.y[2][c];
            float* o = aligned + row * 3;
            o[0] = (float)(M[0][0] * y0 + M[0][1] * y1 + M[0][2] * y2 + ca0);
            o[1] = (float)(M[1][0] * y0 + M[1][1] * y1 + M[1][2] * y2 + ca1);
            o[2] = (float)(M[2][0] * y0 + M[2][1] * y1 + M[2][2] * y2 + ca2);
        }
    }
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_matched_rmsd(const float* __restrict__ a, long long lda, const float* __restrict__ b,
                                                                 long long ldb, const int* __restrict__ species_a,
                                                                 const int* __restrict__ species_b, const int* __restrict__ seg_ptr,
                                                                 int flags, float cap, int exact_limit, float* __restrict__ rmsd,
                                                                 float* __restrict__ rot, float* __restrict__ aligned,
                                                                 int* __restrict__ perm, int* __restrict__ status) {
    __shared__ MatchLds L;
    const int g = blockIdx.x, lane = threadIdx.x;
    const long long r0 = seg_ptr[g];
    const long long nl = (long long)seg_ptr[g + 1] - r0;
    const size_t row = nl > 0 ? (size_t)r0 : 0;             // an empty segment reads nothing: no address is formed from its r0
    matched_body(L, a + row * (size_t)lda, lda, b + row * (size_t)ldb, ldb, species_a + row,
                 (species_b != nullptr ? species_b : species_a) + row, nl, r0, lane, flags, cap, exact_limit, rmsd + g, nullptr,
                 status != nullptr ? status + g : nullptr, nullptr, rot != nullptr ? rot + (size_t)g * 9 : nullptr,
                 aligned != nullptr ? aligned + row * 3 : nullptr, perm != nullptr ? perm + row : nullptr);
}
