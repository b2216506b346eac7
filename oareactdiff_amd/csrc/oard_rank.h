// oard_rank.h — average ranks with ties ("midranks") inside segments, and the ranking metrics built on them.
//
// Replaces what the reference's ConfModule logs through torchmetrics (oa_reactdiff/trainer/pl_trainer.py:475 BinaryAUROC, :485-486
// PearsonCorrCoef / SpearmanCorrCoef, used at :568, :579, :581), per segment of two float32 arrays `score` and `target`: a segment is rows
// seg_ptr[g] .. seg_ptr[g + 1], the convention of k_kabsch_rmsd, with every boundary clamped to [0, n] on the device - a wrong seg_ptr
// cannot make a kernel read outside the arrays.  Nothing is sorted:
//   rank_i = less_i + (equal_i + 1) / 2,    less_i / equal_i = the rows j of i's segment with x_j < x_i / x_j == x_i (i itself included),
// 1-based, scipy.stats.rankdata(method="average").  The counts are int32 compare-and-count, O(sum n_g^2) compares, so a rank is an exact
// half-integer whatever the launch shape and the row order; score and target are counted in the same pass.
//
// k_rank_count (ranks asked for): 64 rows per workgroup, four lanes per row, each lane counting every fourth j; the four partial counts
//   meet in two integer shuffles.  When all rows of a workgroup lie in one segment, the j values go through LDS tiles (RANK_TILE per
//   array, read four at a time; the tile's tail is padded with NaN, which counts as neither less nor equal); otherwise a lane reads the j
//   of its own row's segment from global memory (short segments: the lanes of a row share the cache line).  A row finds its segment by
//   bisection of seg_ptr.  A row in no segment gets NaN.
// k_rank_stats: one wavefront per segment, as k_kabsch_rmsd: float64 lane-strided partial sums in ascending rows, then wave_sum_f64, so a
//   segment's output bits depend on that segment's values alone.  It reads the ranks k_rank_count stored; where a rank array was not asked
//   for it counts in the wave instead (every lane walks the segment for its own rows: meant for short segments).
// Output row of OARD_RANK_COLS = 8 float64:
//   0 n_g   1 n_pos = rows with target >= 0.5   2 AUROC   3 Pearson(score, target)   4 Spearman = Pearson(rank score, rank target)
//   5 mean |score - target|   6 mean score   7 mean target
// AUROC is the Mann-Whitney form (R_pos - n_pos (n_pos + 1) / 2) / (n_pos n_neg) with R_pos the sum of the score midranks of the positive
// rows, kept as an exact int64 of twice-ranks; one float64 division at the end.  Ties get half credit: BinaryAUROC(thresholds=None), the
// trapezoid over the distinct thresholds.  Pearson is two passes, means first and centred sums second (the raw-moment formula cancels for
// near-constant inputs); the mean of a segment's midranks is (n_g + 1) / 2 exactly.
// Special segments:
//   empty                                   col 0 = 0, cols 1-7 NaN;
//   n_pos == 0 or n_pos == n_g              AUROC = 0 (torchmetrics' "0 where undefined", as the trainer's precision / F1);
//   zero variance in either argument        Pearson / Spearman = NaN (0 / 0), as scipy returns;
//   a NaN anywhere in score or target       cols 2-7 NaN and the segment's ranks NaN; nothing faults, other segments are untouched;
//   +-inf                                   ordered like any value: ranks, AUROC and Spearman are defined, the moment columns follow IEEE.
#pragma once
#include "oard_kernels.h"

#define RANK_BLOCK 256        // threads of k_rank_count
#define RANK_ROWS 64          // its rows: 16 per wave, 4 lanes (every fourth j each) per row
#define RANK_TILE 2048        // j values per LDS tile and array (a multiple of 16): 2 x 8 KB

OARD_DEV int rank_clamp(int v, int n) { return min(max(v, 0), n); }

OARD_DEV void rank_count1(float xj, float xi, int& less, int& equal) {
    less += xj < xi ? 1 : 0;
    equal += xj == xi ? 1 : 0;
}

OARD_DEV double rank_value(int less, int equal) { return (double)less + 0.5 * (double)(equal + 1); }

OARD_KERNEL __global__ __launch_bounds__(RANK_BLOCK) void k_rank_count(const float* __restrict__ score, const float* __restrict__ target, int n,
                                                                       const int* __restrict__ seg_ptr, int G, double* __restrict__ rank_s,
                                                                       double* __restrict__ rank_t) {
    __shared__ __attribute__((aligned(16))) float tile_s[RANK_TILE];
    __shared__ __attribute__((aligned(16))) float tile_t[RANK_TILE];
    __shared__ int seg_of_block[2];
    const int tid = threadIdx.x, lane = tid & 63, jq = lane >> 4;
    const long long i_first = (long long)blockIdx.x * RANK_ROWS;
    const long long i_last = min(i_first + RANK_ROWS - 1, (long long)n - 1);
    const long long i = i_first + (tid >> 6) * 16 + (lane & 15);
    const bool valid = i < n;
    // the segment of row i: the first boundary above i, by bisection (empty segments repeat a boundary and are stepped over)
    int lo = 0, hi = G + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rank_clamp(seg_ptr[mid], n) > i) hi = mid; else lo = mid + 1;
    }
    int s0 = 0, s1 = 0;
    if (valid && lo >= 1 && lo <= G) { s0 = rank_clamp(seg_ptr[lo - 1], n); s1 = rank_clamp(seg_ptr[lo], n); }
    const bool in_seg = valid && s0 <= i && i < s1;          // (a seg_ptr that does not ascend: whatever it names, inside the arrays)
    if (!in_seg) s0 = s1 = 0;
    const float xs = in_seg ? score[i] : 0.f, xt = in_seg ? target[i] : 0.f;
    int less_s = 0, eq_s = 0, less_t = 0, eq_t = 0, bad = 0;
    const bool covers = !valid || (in_seg && s0 <= i_first && i_last < s1);
    if (__syncthreads_and(covers ? 1 : 0)) {
        // ---- every row of the workgroup lies in one segment: its values pass through LDS once per workgroup --------------------------
        if (tid == 0) { seg_of_block[0] = s0; seg_of_block[1] = s1; }
        __syncthreads();
        const long long S0 = seg_of_block[0], S1 = seg_of_block[1];
        const float fnan = __builtin_nanf("");
        for (long long t0 = S0; t0 < S1; t0 += RANK_TILE) {
            const int m = (int)min((long long)RANK_TILE, S1 - t0), m_pad = (m + 15) & ~15;
            __syncthreads();
            for (int k = tid; k < m_pad; k += RANK_BLOCK) {
                float a = fnan, b = fnan;
                if (k < m) {
                    a = score[t0 + k]; b = target[t0 + k];
                    bad |= (a != a || b != b) ? 1 : 0;
                }
                tile_s[k] = a; tile_t[k] = b;
            }
            __syncthreads();
#pragma unroll 4
            for (int k = jq * 4; k < m_pad; k += 16) {          // unrolled: one wave per SIMD has nothing else to cover the LDS latency
                const f4 a = *reinterpret_cast<const f4*>(tile_s + k);
                const f4 b = *reinterpret_cast<const f4*>(tile_t + k);
                rank_count1(a.x, xs, less_s, eq_s); rank_count1(a.y, xs, less_s, eq_s);
                rank_count1(a.z, xs, less_s, eq_s); rank_count1(a.w, xs, less_s, eq_s);
                rank_count1(b.x, xt, less_t, eq_t); rank_count1(b.y, xt, less_t, eq_t);
                rank_count1(b.z, xt, less_t, eq_t); rank_count1(b.w, xt, less_t, eq_t);
            }
        }
        bad = __syncthreads_or(bad);
    } else {
        // ---- rows of several segments (or of none): each lane reads every fourth j of its own row's segment ---------------------------
        for (long long j = (long long)s0 + jq; j < s1; j += 4) {
            const float a = score[j], b = target[j];
            bad |= (a != a || b != b) ? 1 : 0;
            rank_count1(a, xs, less_s, eq_s);
            rank_count1(b, xt, less_t, eq_t);
        }
    }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {                     // the four lanes of a row: integer sums, exact in any order
        less_s += __shfl_xor(less_s, d, 64); eq_s += __shfl_xor(eq_s, d, 64);
        less_t += __shfl_xor(less_t, d, 64); eq_t += __shfl_xor(eq_t, d, 64);
        bad |= __shfl_xor(bad, d, 64);
    }
    if (valid && jq == 0) {
        const bool ok = in_seg && !bad;
        const double dnan = __builtin_nan("");
        if (rank_s != nullptr) rank_s[i] = ok ? rank_value(less_s, eq_s) : dnan;
        if (rank_t != nullptr) rank_t[i] = ok ? rank_value(less_t, eq_t) : dnan;
    }
}

OARD_DEV long long wave_sum_i64(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_rank_stats(const float* __restrict__ score, const float* __restrict__ target, int n,
                                                               const int* __restrict__ seg_ptr, const double* __restrict__ rank_s,
                                                               const double* __restrict__ rank_t, double* __restrict__ out) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = rank_clamp(seg_ptr[g], n);
    const int ng = rank_clamp(seg_ptr[g + 1], n) - r0;
    const double dnan = __builtin_nan("");
    double* o = out + (size_t)g * OARD_RANK_COLS;
    if (ng <= 0) {
        if (lane < OARD_RANK_COLS) o[lane] = lane == 0 ? 0.0 : dnan;
        return;
    }
    const float* S = score + r0;
    const float* T = target + r0;
    // ---- pass 1: means, mean absolute difference, the positives, and is there a NaN --------------------------------------------------
    double sum_s = 0, sum_t = 0, sum_ad = 0;
    long long pos = 0;
    bool bad = false;
#pragma unroll 8
    for (int k = lane; k < ng; k += 64) {                    // unrolled for loads in flight; the order of a lane's additions is unchanged
        const float s = S[k], t = T[k];
        bad = bad || s != s || t != t;
        sum_s += (double)s; sum_t += (double)t; sum_ad += fabs((double)s - (double)t);
        pos += t >= 0.5f ? 1 : 0;
    }
    const long long n_pos = wave_sum_i64(pos), n_neg = (long long)ng - n_pos;
    if (__any(bad ? 1 : 0)) {
        if (lane < OARD_RANK_COLS) o[lane] = lane == 0 ? (double)ng : lane == 1 ? (double)n_pos : dnan;
        return;
    }
    const double inv = 1.0 / (double)ng;
    const double mean_s = wave_sum_f64(sum_s) * inv, mean_t = wave_sum_f64(sum_t) * inv, mae = wave_sum_f64(sum_ad) * inv;
    // ---- pass 2: centred sums of the values and of the ranks; twice the rank sum of the positives ------------------------------------
    const bool stored = rank_s != nullptr && rank_t != nullptr;
    const double mean_r = 0.5 * (double)(ng + 1);
    double vss = 0, vtt = 0, vst = 0, rss = 0, rtt = 0, rst = 0;
    long long r_pos2 = 0;
#pragma unroll 8
    for (int k = lane; k < ng; k += 64) {
        const float s = S[k], t = T[k];
        double rs, rt;
        if (stored) {
            rs = rank_s[(size_t)r0 + k]; rt = rank_t[(size_t)r0 + k];
        } else {
            int less_s = 0, eq_s = 0, less_t = 0, eq_t = 0;
            for (int j = 0; j < ng; ++j) {
                rank_count1(S[j], s, less_s, eq_s);
                rank_count1(T[j], t, less_t, eq_t);
            }
            rs = rank_value(less_s, eq_s); rt = rank_value(less_t, eq_t);
        }
        const double ds = (double)s - mean_s, dt = (double)t - mean_t, es = rs - mean_r, et = rt - mean_r;
        vss += ds * ds; vtt += dt * dt; vst += ds * dt;
        rss += es * es; rtt += et * et; rst += es * et;
        r_pos2 += t >= 0.5f ? (long long)(2.0 * rs) : 0;
    }
    vss = wave_sum_f64(vss); vtt = wave_sum_f64(vtt); vst = wave_sum_f64(vst);
    rss = wave_sum_f64(rss); rtt = wave_sum_f64(rtt); rst = wave_sum_f64(rst);
    r_pos2 = wave_sum_i64(r_pos2);
    const double auroc = (n_pos == 0 || n_neg == 0) ? 0.0 : (double)(r_pos2 - n_pos * (n_pos + 1)) / (2.0 * (double)n_pos * (double)n_neg);
    double pearson = vst / (sqrt(vss) * sqrt(vtt)), spearman = rst / (sqrt(rss) * sqrt(rtt));
    pearson = pearson > 1.0 ? 1.0 : pearson < -1.0 ? -1.0 : pearson;          // rounding may step outside [-1, 1]; a NaN passes through
    spearman = spearman > 1.0 ? 1.0 : spearman < -1.0 ? -1.0 : spearman;
    if (lane < OARD_RANK_COLS)
        o[lane] = lane == 0 ? (double)ng : lane == 1 ? (double)n_pos : lane == 2 ? auroc : lane == 3 ? pearson : lane == 4 ? spearman
                : lane == 5 ? mae : lane == 6 ? mean_s : mean_t;
}
