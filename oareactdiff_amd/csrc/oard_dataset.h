// oard_dataset.h — one launch that assembles a training batch from a reaction store held in flat device arrays.
//
// Replaces the reference's per-reaction `__getitem__` plus `collate_fn` (oa_reactdiff/dataset/base_dataset.py:51-88, one torch.cat of B
// tiny tensors per property and object) and what `ProcessedTS1x.__init__` materialises per sample (dataset/transition1x.py:64-150,
// base_dataset.py:142-217): the swapped and the reflected copies, the one-hot rows, the centred positions.
//
// Store (oard_reaction_store, include/oard.h): per SOURCE object (0 reactant, 1 transition state, 2 product) `offsets [n_raw + 1]`, raw
// float32 positions `[sum n, 3]`, atomic numbers `[sum n]`; `sel [n_sel]` the selected raw reactions.  A virtual sample index v in
// [0, n_sel * s * f), s = 1 + swap, f = 1 + reflect, decodes in the reference's list order (original block, swapped block, then the
// reflected copy of both):
//     f_bit = v / (n_sel * s),  j = v % (n_sel * s),  s_bit = j / n_sel,  r = sel[j % n_sel].
// Output object k reads source src_obj[k]; under s_bit the sources 0 and 2 change places.  Under f_bit the last coordinate of an object
// with reflect_obj[k] changes sign (on the raw value, before centring).
//
// k_reaction_gather: one wavefront per (sample, object), four per workgroup.  Lanes stride over the molecule's atoms.  With `center` the
// three coordinate sums are float64: lane partials in ascending rows, then wave_sum_f64 (a fixed butterfly), one float64 division by n,
// and pos = (float)((double)x - mean): one rounding of the exactly centred float32 input, where the reference rounds the float32 sum n
// times, the mean once and the difference once.  A one-atom molecule gives exactly 0.  The int64 rows (one_hot, charge, mask) are
// written as flat runs in 16-byte stores, with a scalar head / tail element where the run does not start or end on 16 bytes.
// Sample b of object k lands at row epoch_off[k][first + b] - epoch_off[k][first]; the rows written are bounded by the span the table
// gives the sample, so a table that disagrees with the store cannot make the kernel write outside the batch.  Every output element has
// one writer (no atomics), and a sample's values depend on that sample alone: the same bits in any batch, at any position.
#pragma once
#include "oard_kernels.h"

#define DATASET_WAVES 4       // (sample, object) pairs per workgroup

struct DatasetOut {
    long long* size[OARD_STORE_OBJECTS];
    float* pos[OARD_STORE_OBJECTS];
    long long* one_hot[OARD_STORE_OBJECTS];
    long long* charge[OARD_STORE_OBJECTS];
    long long* mask[OARD_STORE_OBJECTS];
    const long long* epoch_off[OARD_STORE_OBJECTS];
    long long* condition;
    long long* target;
    float* rmsd;
    float* ediff;
};

OARD_DEV long long dataset_class(int z) { return z == 1 ? 0 : z - 5; }        // ATOM_MAPPING {1: 0, 6: 1, 7: 2, 8: 3, 9: 4}

// p[0 .. count) = f(e), two elements per 16-byte store wherever the address allows
template <typename F>
OARD_DEV void dataset_store_run(long long* __restrict__ p, long long count, int lane, F f) {
    if (count <= 0) return;
    const long long head = (reinterpret_cast<unsigned long long>(p) & 8ull) ? 1 : 0;
    if (head && lane == 0) p[0] = f(0);
    const long long pairs = (count - head) >> 1;
    for (long long q = lane; q < pairs; q += 64) {
        const long long e = head + 2 * q;
        longlong2 v; v.x = f(e); v.y = f(e + 1);
        *reinterpret_cast<longlong2*>(p + e) = v;
    }
    if (((count - head) & 1) && lane == 63) p[count - 1] = f(count - 1);
}

OARD_KERNEL __global__ __launch_bounds__(DATASET_WAVES * 64) void k_reaction_gather(oard_reaction_store st, const long long* __restrict__ index,
                                                                                    long long first, long long B, DatasetOut o) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * DATASET_WAVES + (threadIdx.x >> 6);
    if (w >= B * st.n_obj) return;                                   // whole waves leave: no barrier below
    const long long b = w / st.n_obj;
    const int k = (int)(w - b * st.n_obj);
    const long long v = index[first + b];
    const long long block = st.n_sel * (1 + st.swap);
    if (v < 0 || v >= block * (1 + st.reflect)) return;
    const int f_bit = (int)(v / block);
    const long long j = v - f_bit * block;
    const int s_bit = (int)(j / st.n_sel);
    const long long r = st.sel[j - s_bit * st.n_sel];
    if (r < 0 || r >= st.n_raw) return;
    int src = st.src_obj[k];
    if (s_bit) src = 2 - src;                                        // FRAG_MAPPING: reactant <-> product, the transition state stays
    const long long s0 = st.offsets[src][r];
    const long long* __restrict__ off = o.epoch_off[k];
    const long long d0 = off[first + b] - off[first];
    const long long n = min((long long)(st.offsets[src][r + 1] - s0), (long long)(off[first + b + 1] - off[first + b]));
    const float* __restrict__ x = st.pos[src] + 3 * s0;
    const int* __restrict__ z = st.z[src] + s0;
    const float sign = (f_bit && st.reflect_obj[k]) ? -1.f : 1.f;

    double m0 = 0, m1 = 0, m2 = 0;
    if (st.center) {
        for (long long i = lane; i < n; i += 64) {
            m0 += (double)x[3 * i]; m1 += (double)x[3 * i + 1]; m2 += (double)(sign * x[3 * i + 2]);
        }
        const double dn = (double)n;
        m0 = wave_sum_f64(m0) / dn; m1 = wave_sum_f64(m1) / dn; m2 = wave_sum_f64(m2) / dn;
    }
    float* __restrict__ pos = o.pos[k] + 3 * d0;
    for (long long i = lane; i < n; i += 64) {
        pos[3 * i] = (float)((double)x[3 * i] - m0);
        pos[3 * i + 1] = (float)((double)x[3 * i + 1] - m1);
        pos[3 * i + 2] = (float)((double)(sign * x[3 * i + 2]) - m2);
    }
    dataset_store_run(o.one_hot[k] + 5 * d0, 5 * n, lane, [&](long long e) {
        const long long row = e / 5;
        return (long long)(dataset_class(z[row]) == e - 5 * row ? 1 : 0);
    });
    if (st.append_frag) {
        const long long extra = st.append_charge[k];
        dataset_store_run(o.charge[k] + 2 * d0, 2 * n, lane, [&](long long e) {
            return (e & 1) ? extra : (st.zero_charge ? 0ll : (long long)z[e >> 1]);
        });
    } else {
        dataset_store_run(o.charge[k] + d0, n, lane, [&](long long e) { return st.zero_charge ? 0ll : (long long)z[e]; });
    }
    dataset_store_run(o.mask[k] + d0, n, lane, [&](long long) { return b; });
    if (lane == 0) {
        o.size[k][b] = n;
        if (k == 0) {
            o.condition[b] = 0;
            // the reference's target / rmsd columns are the RAW lists times `repeat`, neither selected nor reflected, read at the sample's
            // own index (transition1x.py:92-98, base_dataset.py:52)
            if (o.target) o.target[b] = st.target[v % st.n_raw];
            if (o.rmsd) o.rmsd[b] = st.rmsd[v % st.n_raw];
            if (o.ediff) o.ediff[b] = st.ediff[s_bit][r];
        }
    }
}
