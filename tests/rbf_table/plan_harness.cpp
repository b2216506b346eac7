// Prints FwdPlan::rbf_table (csrc/oard_plan.h) of every case read from stdin, one line per case.  TEST INFRASTRUCTURE of
// tests/test_rbf_table_cpu.py (g++, address + undefined-behaviour sanitizers, a child process); tests/launch_plan/harness.cpp prints the
// rest of the plan.
//   in : equi_variant auto_small auto_tiny equi_rbf_table precision train conc npb A E num_layers rbf_good
//   out: equi shape, then rbf_table[0 .. 15], then plan_rbf_wanted
#include <cstdio>
#include "../../oareactdiff_amd/csrc/oard_plan.h"

int main() {
    FwdPlanIn in = {};
    in.opt = FwdOptions{};
    int train;
    in.cus = 256; in.scratch = true;      // (the stage-split latency shape needs its scratch)
    while (scanf("%d %d %d %d %d %d %d %d %lld %lld %d %u", &in.opt.equi_variant, &in.opt.auto_small, &in.opt.auto_tiny, &in.opt.equi_rbf_table,
                 &in.precision, &train, &in.conc, &in.npb, &in.A, &in.E, &in.num_layers, &in.rbf_good) == 12) {
        in.train = train != 0;
        in.CI = in.A; in.CX = in.E - in.A;
        const FwdPlan p = make_fwd_plan(in);
        printf("%d", (int)p.equi);
        for (int l = 0; l < 16; ++l) printf(" %d", (int)p.rbf_table[l]);
        printf(" %d\n", (int)plan_rbf_wanted(in));
    }
    return 0;
}
