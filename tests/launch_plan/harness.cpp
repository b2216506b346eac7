// Prints the forward launch plan (csrc/oard_plan.h) of every case read from stdin, one line per case.  TEST INFRASTRUCTURE:
// tests/test_launch_plan.py compiles it with g++ (address + undefined-behaviour sanitizers), runs it as a child process and checks the
// lines against its own restatement of the rules.
//   in : 12 options in FwdOptions order, then precision train conc npb cus A E CI CX num_layers scratch
//   out: msum l0_skip use_al fill_edges init_v1 scalarize_tiles node equi, then for the layer kinds 0..3 (bit 0 = first, bit 1 = last):
//        n, and per launch r0 r1 s1 s3 shape grid
#include <cstdio>
#include "../../oareactdiff_amd/csrc/oard_plan.h"

int main(int argc, char**) {
    FwdPlanIn in;
    FwdOptions& o = in.opt;
    int train, scratch;
    if (argc > 1) {           // any argument: print the library's default options, in FwdOptions order
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", o.gcl_variant, o.equi_variant, o.node_variant, o.auto_small, o.auto_tiny, o.small_split,
               o.gcl_persist, o.gcl_grid, o.gcl_skip, o.equi_skip, o.equi_l0_skip, o.gcl_msum);
        return 0;
    }
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %d", &o.gcl_variant, &o.equi_variant, &o.node_variant,
                 &o.auto_small, &o.auto_tiny, &o.small_split, &o.gcl_persist, &o.gcl_grid, &o.gcl_skip, &o.equi_skip, &o.equi_l0_skip, &o.gcl_msum,
                 &in.precision, &train, &in.conc, &in.npb, &in.cus, &in.A, &in.E, &in.CI, &in.CX, &in.num_layers, &scratch) == 23) {
        in.train = train != 0;
        in.scratch = scratch != 0;
        const FwdPlan p = make_fwd_plan(in);
        printf("%d %d %d %d %d %d %d %d", p.msum, p.l0_skip, p.use_al, p.fill_edges, p.init_v1, p.scalarize_tiles, (int)p.node, (int)p.equi);
        for (const GclLayer& g : p.gcl) {
            printf(" %d", g.n);
            for (int i = 0; i < g.n; ++i)
                printf(" %lld %lld %d %d %d %lld", g.l[i].r0, g.l[i].r1, g.l[i].s1, g.l[i].s3, (int)g.l[i].shape, g.l[i].grid);
        }
        printf("\n");
    }
    return 0;
}
