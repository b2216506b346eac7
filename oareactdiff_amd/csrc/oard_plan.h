// oard_plan.h - the launch plan of the forward pass: which kernel shape every launch of one call and sub-batch takes, decided ONCE, by a
// pure function of the options, the call and the sizes.  forward_impl and its launchers (oard_hip.hip) only switch on the plan's fields.
// Host only, plain C++17, no HIP: tests/launch_plan/harness.cpp compiles it with g++ and tests/test_launch_plan.py enumerates it.
#pragma once
#include <algorithm>
#include "../../include/oard.h"

// The forward-shape debug options (oard_debug_option).  oard_forward / oard_forward_train copy the process-wide value once at entry:
// every sub-batch of a call is planned from that copy.
struct FwdOptions {
    int gcl_variant = 2;     // 0: first generation (weights straight from L2), 2: LDS-streamed 8-wave shape, 3: 4-wave shape, 6: latency kernel
    int equi_variant = 2;    // 0: first generation, 2: LDS-streamed 8-wave shape, 1: 4-wave shape, 4: latency kernel
    int node_variant = 1;    // 0: one wave per 16 nodes, 1: 8 waves per 16 nodes with LDS-resident activations
    int auto_small = 4;      // launches of <= 1024 (GCL) / 512 (EquiMessage) x this many 16-edge tiles, all concurrent sub-batches together,
                             //    use the 4-wave workgroups (one wave per SIMD: a launch that cannot fill the chip finishes sooner); 0 = never
    int auto_tiny = 8;       // launches of <= 512 x this many tiles use the latency kernels of oard_edge_small.h (8 waves share 16 edges); 0 = never
    int small_split = 128;   // EquiMessage latency kernel: launches of <= this many tiles run one launch per dense stage; 0 = never
    int gcl_persist = 1;     // the fp32 GCL throughput shape as persistent workgroups (oard_edge_p.h) when the launch has the chip to itself;
                             //    2: also beside concurrent sub-batches, 0: always one 128-edge tile per workgroup
    int gcl_grid = 0;        // workgroups per persistent launch: 0 = one per CU (half of them beside concurrent sub-batches), > 0 = that
                             //    many, -k = k rounds (128-row tiles) per workgroup
    int gcl_skip = 1;        // skip S1 (first layer) / S3 (last layer) on inter-object edges
    int equi_skip = 1;       // EquiMessage runs the inner edges inside the cutoff only (ActList; exact: it is zero on the others)
    int equi_l0_skip = 1;    // 0: layer 0 runs the whole EquiMessage like every other layer (A/B and tests; FwdPlan::l0_skip)
    int gcl_msum = 1;        // 0: the GCL edge kernels store one message row per edge and the node stage gathers them (A/B and tests; FwdPlan::msum)
    int equi_rbf_table = 1;  // 0: EquiMessage's rbf_proj always runs as an MFMA chain, never from its table in exp(-d) (A/B and tests; FwdPlan::rbf_table)
};

enum GclShape {
    GCL_INVALID = 0,         // no kernel for this variant in this build: the launch returns OARD_EINVAL
    GCL_V0,                  // first generation (experiment builds)
    GCL_PERSIST, GCL_RING3,  // fp32 throughput shape: persistent workgroups over half-tiles / one 8-wave tile (three LDS slabs) per workgroup
    GCL_W4, GCL_SMALL, GCL_B3,   // 4 waves x 16 edges / latency kernel / split precision (OARD_PREC_GCL_BF16X3)
    GCL_TRAIN_PERSIST, GCL_TRAIN_RING3, GCL_TRAIN_B3,   // training-mode forward: pre-activations taped
    GCL_X0 = 100             // + gcl_variant: the A/B shapes of experiment builds (tools/ab_gcl.sh)
};
enum EquiShape { EQ_INVALID = 0, EQ_V0, EQ_W8, EQ_W4, EQ_SMALL, EQ_SMALL_SPLIT, EQ_B3, EQ_TRAIN, EQ_TRAIN_B3 };
enum NodeForm { NODE_V0 = 0, NODE_ROWS, NODE_LARGE };   // first generation / small batches (gathers walk rows, npb <= 4) / large batches

struct GclLaunch { long long r0, r1; bool s1, s3; GclShape shape; long long grid; };   // rows (msum: columns) [r0, r1), stages run, workgroups
struct GclLayer { int n; GclLaunch l[2]; };
struct FwdPlanIn {
    FwdOptions opt;
    int precision;           // oard_config::precision
    bool train;
    int conc, npb, cus;      // concurrent sub-batches, nodes per node-stage workgroup, compute units
    long long A, E, CI, CX;  // inner edges, edges, columns of the inner / inter-object list (TopoDev)
    int num_layers;
    bool scratch;            // the stage-split scratch exists (WsOff::small_a)
    unsigned rbf_good = 0;   // bit l: layer l's rbf_proj table exists in the blob and passed its check (oard_rbf_table.h); 0 = none built
};
struct FwdPlan {
    int num_layers;
    bool fill_edges;         // k_fill_edges materialises the constant inter-object rows (nobody reads them where layer 0 skips S1)
    bool init_v1;            // init and output stages: 8-wave node kernels (else first generation)
    bool scalarize_tiles;    // k_scalarize: one workgroup per (64 edges, hidden tile) - small launches
    // GCL messages summed per node inside the edge kernels and ~6 partial rows per node gathered instead of one row per edge - edge
    // kernels and node stage both or neither, the node stage must not read what the edge kernels did not write: only where the node stage is
    // the large-batch one and the inner and the inter-object list, each as a launch of its own, take the fp32 throughput shape.  (With
    // gcl_skip the first layer launches them apart, so that is: EVERY launch of the call.)  The launches then run columns, not rows.
    bool msum;
    GclLayer gcl[4];         // by kind of layer: bit 0 = first, bit 1 = last
    EquiShape equi;
    bool use_al;             // the inner rows inside the cutoff are compacted per call; EquiMessage (edge kernel and gather) runs those only
    NodeForm node;
    // layer 0 of an inference forward: vec is exactly zero there, so the third of q that only multiplies vec[src] is neither computed
    // (8-wave streamed fp32 edge kernel) nor gathered (large-batch node stage) - both or neither.  The training-mode forward tapes it.
    bool l0_skip;
    // per layer: the 8-wave streamed fp32 EquiMessage kernel of an inference forward takes rbf_proj from the layer's table in exp(-d)
    // instead of an MFMA chain - only where that table passed its check (FwdPlanIn::rbf_good).  The training-mode forward never does.
    bool rbf_table[16];   // [OARD_MAX_LAYERS]
    const GclLayer& gcl_at(int l) const { return gcl[(l == 0 ? 1 : 0) | (l == num_layers - 1 ? 2 : 0)]; }
};

inline long long plan_cdiv(long long a, long long b) { return (a + b - 1) / b; }
// The thresholds, in 16-edge tiles in flight (all concurrent sub-batches together): a launch of the throughput variant 2 of at most
// small_tiles * auto_small tiles takes the 4-wave variant `w4`, one of at most 512 * auto_tiny the latency variant `lat`.
inline int plan_demote(const FwdPlanIn& in, int v, long long n, long long small_tiles, int w4, int lat) {
    const long long load = plan_cdiv(n, 16) * in.conc;
    if (v == 2 && load <= small_tiles * in.opt.auto_small) v = w4;
    if ((v == 2 || v == w4) && load <= 512LL * in.opt.auto_tiny) v = lat;
    return v;
}
inline GclShape plan_gcl_shape(const FwdPlanIn& in, long long n) {
    const int persist = in.opt.gcl_persist;
    if (in.train) return (in.precision & OARD_PREC_TRAIN_BF16X3) ? GCL_TRAIN_B3 : persist ? GCL_TRAIN_PERSIST : GCL_TRAIN_RING3;
    const int v = plan_demote(in, in.opt.gcl_variant, n, 1024, 3, 6);
    switch (v) {
        case 0: return GCL_V0;
        // A launch that has the chip to itself runs as persistent workgroups (same arithmetic, bit-identical rows): its last round is
        // balanced (isolated 9.01 -> 8.62 ms per B = 64 step).  Concurrent sub-batches keep one tile per workgroup: there the other streams'
        // kernels fill the tail, and workgroups that hold a CU for several tiles make THEM wait (17.93 ms per step with tiles, 18.05 - 18.3
        // with 64 ... 256 persistent workgroups per launch).
        case 2: return (in.precision & OARD_PREC_GCL_BF16X3) ? GCL_B3 : (persist > 1 || (persist == 1 && in.conc == 1)) ? GCL_PERSIST : GCL_RING3;
        case 3: return GCL_W4;
        case 6: return GCL_SMALL;
#ifdef OARD_EXPERIMENTS
        case 4: case 5: case 7: case 8: case 9: case 10: case 11: case 12: return GclShape(GCL_X0 + v);
#endif
        default: return GCL_INVALID;
    }
}
inline long long plan_gcl_grid(const FwdPlanIn& in, GclShape s, long long n) {
    if (s == GCL_PERSIST || s == GCL_TRAIN_PERSIST) {       // (the training-mode forward is one sub-batch)
        const long long nhalf = plan_cdiv(plan_cdiv(n, 16), 4), g = in.opt.gcl_grid;
        return std::min(nhalf, g > 0 ? g : g < 0 ? plan_cdiv(nhalf, 2 * -g) : in.conc > 1 ? std::max(1, in.cus / 2) : in.cus);
    }
    // rows per workgroup: 16 per wave, the latency kernel's 8 waves share 16
    return plan_cdiv(n, s == GCL_SMALL ? 16 : (s == GCL_V0 || s == GCL_W4 || s == GCL_X0 + 12) ? 64 : (s == GCL_X0 + 10 || s == GCL_X0 + 11) ? 192 : 128);
}
// (the latency kernels run every inner row: their q is zero outside the cutoff, where the node stage does not read it)
inline EquiShape plan_equi_shape(const FwdPlanIn& in) {
    if (in.train) return (in.precision & OARD_PREC_TRAIN_BF16X3) ? EQ_TRAIN_B3 : EQ_TRAIN;
    switch (plan_demote(in, in.opt.equi_variant, in.A, 512, 1, 4)) {
        case 0: return EQ_V0;
        case 1: return EQ_W4;
        case 2: return (in.precision & OARD_PREC_EQUI_BF16X3) ? EQ_B3 : EQ_W8;
        case 4: return in.scratch && plan_cdiv(in.A, 16) * in.conc <= in.opt.small_split ? EQ_SMALL_SPLIT : EQ_SMALL;
        default: return EQ_INVALID;
    }
}
// could this call take rbf_proj from its tables if they are good?  (forward_impl asks for FwdPlanIn::rbf_good only then)
inline bool plan_rbf_wanted(const FwdPlanIn& in) {
    return !in.train && in.opt.equi_rbf_table && in.A > 0 && plan_equi_shape(in) == EQ_W8;
}
// The training-mode forward has one shape per stage: variants 2 / 2 / 1, the layer-0 / last-layer shortcuts of the GCL always on.
inline FwdPlan make_fwd_plan(FwdPlanIn in) {
    if (in.train) { in.opt.gcl_variant = in.opt.equi_variant = 2; in.opt.node_variant = 1; in.opt.gcl_skip = 1; }
    const FwdOptions& o = in.opt;
    const bool nv1 = o.node_variant == 1 && o.equi_variant != 0, skip = o.gcl_skip && o.gcl_variant != 0;
    FwdPlan p = {};
    p.num_layers = in.num_layers;
    p.fill_edges = !skip;
    p.init_v1 = o.node_variant >= 1;
    p.scalarize_tiles = plan_cdiv(in.A, 64) * in.conc <= 2048;
    p.node = !nv1 ? NODE_V0 : in.npb <= 4 ? NODE_ROWS : NODE_LARGE;
    p.equi = plan_equi_shape(in);
    p.use_al = !in.train && o.equi_skip && in.A > 0 && nv1;
    p.l0_skip = !in.train && o.equi_l0_skip && in.A > 0 && p.node == NODE_LARGE && p.equi == EQ_W8;
    for (int l = 0; l < 16; ++l)
        p.rbf_table[l] = !in.train && o.equi_rbf_table && in.A > 0 && p.equi == EQ_W8 && l < in.num_layers && ((in.rbf_good >> l) & 1u);
    auto throughput = [&](long long n) { const GclShape s = plan_gcl_shape(in, n); return n == 0 || s == GCL_PERSIST || s == GCL_RING3; };
    p.msum = !in.train && o.gcl_msum && in.E > 0 && o.gcl_variant == 2 && p.node == NODE_LARGE && throughput(in.CI) && throughput(in.CX);
    // Inner edges run every stage; inter-object edges skip S1 in the first layer (constant initial state) and S3 in the last (their
    // updated state is never read).  Where both lists run every stage they are ONE launch (msum: the inter-object list starts on a
    // multiple of 16 columns, so the wave tiles - and with them every partial sum - are the same as in two launches).
    const long long inner = p.msum ? in.CI : in.A, all = p.msum ? in.CI + in.CX : in.E;
    for (int k = 0; k < 4; ++k) {
        GclLayer& g = p.gcl[k];
        auto add = [&](long long r0, long long r1, bool s1, bool s3) {
            const GclShape s = plan_gcl_shape(in, r1 - r0);
            if (r1 > r0) g.l[g.n++] = GclLaunch{r0, r1, s1, s3, s, plan_gcl_grid(in, s, r1 - r0)};
        };
        const bool s1 = !(skip && (k & 1)), s3 = !(skip && (k & 2));
        if (s1 && s3) add(0, all, true, true);
        else { add(0, inner, true, true); add(inner, all, s1, s3); }
    }
    return p;
}
