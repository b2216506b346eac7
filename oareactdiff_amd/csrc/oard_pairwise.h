// oard_pairwise.h — how many DIFFERENT structures do K candidates hold: the all-pairs RMSD matrix of every group of structures, and the
// greedy de-duplication on it.
//
// Replaces two host loops over pymatgen of the reference's walkthrough: the all-pairs matrix over the transition states of one reaction
// (demo.py:401-480, pymatgen_rmsd(..., ignore_chirality=True) over every i < j) and the de-duplication of generated structures
// (demo.py:544-557: a structure is new when its smallest RMSD to the structures kept so far exceeds 0.1).
//
// LAYOUT.  A MEMBER is a segment of ONE row-major array x (rows seg_ptr[s] .. seg_ptr[s + 1], coordinates in the first three columns, row
// stride ldx), read where it lies.  A GROUP is a list of members: group g is group_members[group_ptr[g] .. group_ptr[g + 1]], segment
// indices in any order (K candidates of R reactions, candidate-major: group r holds segments r, R + r, 2 R + r, ...).  With K_g members,
//   pair_ptr[g] = sum over g' < g of K_g' (K_g' - 1) / 2      (int64)      the first pair of group g
//   mat_ptr[g]  = sum over g' < g of K_g'^2                    (int64)      the first entry of its K_g x K_g matrix, row-major
// and the pairs of a group are its upper triangle row by row: (0, 1), (0, 2), ..., (1, 2), ...
//
// k_pairwise_kabsch / k_pairwise_matched: one wavefront per pair.  It finds its group by binary search in pair_ptr, decodes (i, j), and
// calls kabsch_body (csrc/oard_kabsch.h) / matched_body (csrc/oard_match.h) - the bodies of k_kabsch_rmsd / k_matched_rmsd, not a copy of
// them - with member i as the target and member j fitted onto it, and writes the value to [i, j] AND [j, i]: the matrix is symmetric bit
// for bit, and entry [i, j] has the bits the per-segment kernel gives for explicit copies of the two members.
// k_pairwise_diag: one wavefront per member writes the diagonal: 0, or what a pair of this member with itself would give where the
// member is special (below).  It also serves K_g = 1, which has no pair.
//
// STATUS (optional, packed like the matrices): 0 exact / same-order fit, 1 search, 2 the species lists differ, 3 a member of more than
// MATCH_MAX rows (matched mode only), 4 a non-finite coordinate, 5 the two members have different row counts.  A pair with an EMPTY member
// (no rows, or a member index outside [0, S)) gives NaN and status 0.  Otherwise 3, 4 and 5 are checked in this order - what is wrong with
// a member alone comes before what is wrong with the pair, so a non-finite or over-long member carries ONE code along its whole row and
// column, the diagonal included - and then 2.  Statuses 2 .. 5 give cap if cap > 0, else NaN; with a cap every value is min(value, cap).
//
// THE PAIR DECODE.  Row i of a K x K upper triangle starts at pair off(i) = i (2 K - i - 1) / 2.  A float64 square root proposes
// i ~ ((2 K - 1) - sqrt((2 K - 1)^2 - 8 q)) / 2; the answer is the i with off(i) <= q < off(i + 1), found from the proposal by integer
// comparisons alone (tests/_pairwise_cases.py holds the same arithmetic in numpy).
//
// SAFETY.  Every index read from device memory is clamped before it is used: group boundaries into [0, n_members], member indices into
// [0, S) (outside: an empty member), segment boundaries into [0, seg_ptr[S]] (the rows the caller named), and a group whose matrix does
// not lie inside [0, mat_ptr[G]) or whose pairs do not fit pair_ptr is not written at all.  Wrong tables give wrong numbers, never an
// access outside the arrays.
//
// k_leader_cluster: the de-duplication, one wavefront per group.  The members are visited in a given order (`order`: group-local
// indices packed like the members; NULL: index order).  The lanes stride over the leaders found so far; the member joins the leader at the
// smallest distance if that distance is <= threshold (float32 compare on the stored entry dist[member, leader]; a tie goes to the leader
// created first), else it becomes a leader.  A NaN is never close, so a poisoned member ends up alone.  The leader list lives in LDS
// behind a barrier, LEADER_MAX entries: a group of more members gets label -1 throughout and n_clusters -1.  An `order` entry outside
// [0, K_g) is skipped (its slot's member keeps label -1 unless visited otherwise).  Integer work and float compares only: no tolerance.
#pragma once
#include "oard_match.h"

#define LEADER_MAX 1024       // members per group of k_leader_cluster (the LDS leader list)
#define PAIR_UNEQUAL 5        // status: the two members have different row counts

OARD_DEV long long pair_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// pairs before row i of a K x K upper triangle
OARD_DEV long long pair_row_start(long long i, long long K) { return i * (2 * K - i - 1) / 2; }

// q in [0, K (K - 1) / 2) -> (i, j), i < j.  The square root only proposes; the two loops decide, and end after at most K steps.
OARD_DEV void pair_decode(long long q, long long K, int& i_out, int& j_out) {
    const double b = (double)(2 * K - 1);
    double disc = b * b - 8.0 * (double)q;
    disc = disc > 0.0 ? disc : 0.0;
    long long i = (long long)((b - sqrt(disc)) * 0.5);
    i = pair_clamp(i, 0, K - 2);
    while (i > 0 && pair_row_start(i, K) > q) --i;
    while (i < K - 2 && pair_row_start(i + 1, K) <= q) ++i;
    i_out = (int)i;
    j_out = (int)(i + 1 + (q - pair_row_start(i, K)));
}

// The largest g in [0, G) with ptr[g] <= v (ptr ascending; G >= 1).
OARD_DEV int pair_find_group(const long long* __restrict__ ptr, int G, long long v) {
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

struct PairMember { long long r0; long long n; };

// Member `m` of the launch (an entry of group_members) -> its rows, every boundary clamped; outside [0, S): empty.
OARD_DEV PairMember pair_member(const int* __restrict__ seg_ptr, int S, int m) {
    PairMember out = {0, 0};
    if (m < 0 || m >= S) return out;
    const long long rows = pair_clamp(seg_ptr[S], 0, 0x7fffffffLL);
    const long long r0 = pair_clamp(seg_ptr[m], 0, rows), r1 = pair_clamp(seg_ptr[m + 1], r0, rows);
    out.r0 = r0; out.n = r1 - r0;
    return out;
}

// Is every coordinate of the member finite (wave-uniform answer)?
OARD_DEV bool pair_member_finite(const float* __restrict__ x, long long ldx, PairMember m, int lane) {
    bool bad = false;
    for (long long k = lane; k < m.n; k += 64) {
        const float* p = x + (size_t)(m.r0 + k) * (size_t)ldx;
        bad = bad || !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
    }
    return !__any(bad ? 1 : 0);
}

// Where one pair (or, with i == j, one diagonal entry) writes: the group, the two members and the slots, all checked.
struct PairSlots {
    bool ok;
    PairMember a, b;
    float *o, *ot;
    int *s, *st;
};

// Group g with K members (already clamped) and the local indices i, j -> members and output slots; ok = false: write nothing.
OARD_DEV PairSlots pair_slots(const int* __restrict__ seg_ptr, int S, const int* __restrict__ group_members, long long m0, long long K,
                              const long long* __restrict__ mat_ptr, int g, int G, int i, int j, float* out, int* status) {
    PairSlots p = {};
    const long long base = mat_ptr[g], total = mat_ptr[G];
    if (base < 0 || K * K > total - base || total < 0) return p;      // the matrix must lie inside [0, mat_ptr[G])
    p.ok = true;
    p.a = pair_member(seg_ptr, S, group_members[m0 + i]);
    p.b = pair_member(seg_ptr, S, group_members[m0 + j]);
    p.o = out + base + (long long)i * K + j;
    p.ot = out + base + (long long)j * K + i;
    p.s = status != nullptr ? status + base + (long long)i * K + j : nullptr;
    p.st = status != nullptr ? status + base + (long long)j * K + i : nullptr;
    return p;
}

// The pair of this wavefront: group by binary search in pair_ptr, (i, j) from pair_decode.
OARD_DEV PairSlots pair_of_wave(const int* __restrict__ seg_ptr, int S, const int* __restrict__ group_members,
                                const int* __restrict__ group_ptr, const long long* __restrict__ pair_ptr,
                                const long long* __restrict__ mat_ptr, int G, int M, float* out, int* status) {
    PairSlots none = {};
    const long long p = blockIdx.x;
    const int g = pair_find_group(pair_ptr, G, p);
    const long long m0 = pair_clamp(group_ptr[g], 0, M), K = pair_clamp(group_ptr[g + 1], m0, M) - m0;
    const long long q = p - pair_ptr[g];
    if (K < 2 || q < 0 || q >= K * (K - 1) / 2) return none;            // pair_ptr does not fit group_ptr: not this wavefront's to write
    int i, j;
    pair_decode(q, K, i, j);
    return pair_slots(seg_ptr, S, group_members, m0, K, mat_ptr, g, G, i, j, out, status);
}

// What is wrong with the two members before any fit is tried -> true if the pair was written here.  matched: MATCH_MAX applies.
OARD_DEV bool pair_special(const float* __restrict__ x, long long ldx, const PairSlots& p, bool matched, float cap, int lane) {
    const float fnan = __builtin_nanf("");
    if (p.a.n <= 0 || p.b.n <= 0) {
        if (lane == 0) kabsch_store(p.o, p.ot, fnan, p.s, p.st, 0);
        return true;
    }
    if (p.a.n == p.b.n) return false;                                    // the shared body checks 3, 4, 2 itself
    int code = PAIR_UNEQUAL;
    if (matched && (p.a.n > MATCH_MAX || p.b.n > MATCH_MAX)) code = 3;
    else if (!(pair_member_finite(x, ldx, p.a, lane) && pair_member_finite(x, ldx, p.b, lane))) code = 4;
    if (lane == 0) kabsch_store(p.o, p.ot, cap > 0.f ? cap : fnan, p.s, p.st, code);
    return true;
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_pairwise_kabsch(const float* __restrict__ x, long long ldx,
                                                                    const int* __restrict__ seg_ptr, int S,
                                                                    const int* __restrict__ group_members,
                                                                    const int* __restrict__ group_ptr,
                                                                    const long long* __restrict__ pair_ptr,
                                                                    const long long* __restrict__ mat_ptr, int G, int M, int flags, float cap,
                                                                    float* __restrict__ out, int* __restrict__ status) {
    const int lane = threadIdx.x;
    const PairSlots p = pair_of_wave(seg_ptr, S, group_members, group_ptr, pair_ptr, mat_ptr, G, M, out, status);
    if (!p.ok || pair_special(x, ldx, p, false, cap, lane)) return;
    kabsch_body(x + (size_t)p.a.r0 * (size_t)ldx, ldx, x + (size_t)p.b.r0 * (size_t)ldx, ldx, (int)p.a.n, lane, flags, cap, p.o, p.ot, p.s,
                p.st, nullptr, nullptr);
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_pairwise_matched(const float* __restrict__ x, long long ldx,
                                                                     const int* __restrict__ species, const int* __restrict__ seg_ptr,
                                                                     int S, const int* __restrict__ group_members,
                                                                     const int* __restrict__ group_ptr,
                                                                     const long long* __restrict__ pair_ptr,
                                                                     const long long* __restrict__ mat_ptr, int G, int M, int flags, float cap,
                                                                     int exact_limit, float* __restrict__ out, int* __restrict__ status) {
    __shared__ MatchLds L;
    const int lane = threadIdx.x;
    const PairSlots p = pair_of_wave(seg_ptr, S, group_members, group_ptr, pair_ptr, mat_ptr, G, M, out, status);
    if (!p.ok || pair_special(x, ldx, p, true, cap, lane)) return;
    matched_body(L, x + (size_t)p.a.r0 * (size_t)ldx, ldx, x + (size_t)p.b.r0 * (size_t)ldx, ldx, species + p.a.r0, species + p.b.r0, p.a.n,
                 p.a.r0, lane, flags, cap, exact_limit, p.o, p.ot, p.s, p.st, nullptr, nullptr, nullptr);
}

// The diagonal: one wavefront per member slot m of group_members.  0 for a finite member; the member's own code otherwise.
OARD_KERNEL __global__ __launch_bounds__(64) void k_pairwise_diag(const float* __restrict__ x, long long ldx, const int* __restrict__ seg_ptr,
                                                                  int S, const int* __restrict__ group_members,
                                                                  const int* __restrict__ group_ptr, const long long* __restrict__ mat_ptr,
                                                                  int G, int M, int matched, float cap, float* __restrict__ out,
                                                                  int* __restrict__ status) {
    const int lane = threadIdx.x, m = blockIdx.x;
    // the largest g with group_ptr[g] <= m whose group is not empty there: binary search on the clamped boundaries, then the check
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pair_clamp(group_ptr[mid], 0, M) <= m) lo = mid; else hi = mid;
    }
    const int g = lo;
    const long long m0 = pair_clamp(group_ptr[g], 0, M), K = pair_clamp(group_ptr[g + 1], m0, M) - m0;
    if (m < m0 || m >= m0 + K) return;                                   // a slot of no group (group_ptr not ascending from 0)
    const int i = (int)(m - m0);
    const PairSlots p = pair_slots(seg_ptr, S, group_members, m0, K, mat_ptr, g, G, i, i, out, status);
    if (!p.ok) return;
    const float fnan = __builtin_nanf("");
    int code = 0;
    float v = 0.f;
    if (p.a.n <= 0) v = fnan;
    else if (matched && p.a.n > MATCH_MAX) code = 3;
    else if (!pair_member_finite(x, ldx, p.a, lane)) code = 4;
    if (code != 0) v = cap > 0.f ? cap : fnan;
    if (lane == 0) kabsch_store(p.o, nullptr, v, p.s, nullptr, code);
}

OARD_KERNEL __global__ __launch_bounds__(64) void k_leader_cluster(const float* __restrict__ dist, const long long* __restrict__ mat_ptr,
                                                                   const int* __restrict__ group_ptr, const int* __restrict__ order, int G,
                                                                   float threshold, int* __restrict__ label, int* __restrict__ n_clusters) {
    __shared__ int leaders[LEADER_MAX];
    const int g = blockIdx.x, lane = threadIdx.x;
    const long long M = pair_clamp(group_ptr[G], 0, 0x7fffffffLL);
    const long long m0 = pair_clamp(group_ptr[g], 0, M), K = pair_clamp(group_ptr[g + 1], m0, M) - m0;
    const long long base = mat_ptr[g], total = mat_ptr[G];
    const bool fits = K <= LEADER_MAX && base >= 0 && total >= 0 && K * K <= total - base;
    for (long long t = lane; t < K; t += 64) label[m0 + t] = -1;
    if (!fits) {
        if (lane == 0) n_clusters[g] = -1;
        return;
    }
    __syncthreads();
    const float* D = dist + base;
    int nl = 0;
#pragma unroll 1
    for (int t = 0; t < (int)K; ++t) {
        const int m = order != nullptr ? order[m0 + t] : t;
        if (m < 0 || m >= (int)K) continue;                              // wave-uniform: every lane read the same entry
        float best = 0.f;
        int bl = 0x7fffffff;
        for (int l = lane; l < nl; l += 64) {
            const float d = D[(long long)m * K + leaders[l]];
            if (d <= threshold && (bl == 0x7fffffff || d < best)) { best = d; bl = l; }      // ascending l: the first leader of the lane wins a tie
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const float ob = __shfl_xor(best, s, 64);
            const int ol = __shfl_xor(bl, s, 64);
            const bool take = ol != 0x7fffffff && (bl == 0x7fffffff || ob < best || (ob == best && ol < bl));
            best = take ? ob : best; bl = take ? ol : bl;
        }
        bl = match_uniform(bl);
        if (lane == 0) {
            if (bl != 0x7fffffff && bl >= 0 && bl < nl) label[m0 + m] = leaders[bl];
            else { leaders[nl] = m; label[m0 + m] = m; }
        }
        if (bl == 0x7fffffff) nl += 1;
        __syncthreads();                                                 // the next member's lanes see the list
    }
    if (lane == 0) n_clusters[g] = nl;
}
