// The arithmetic of the rbf_proj table (csrc/oard_rbf_table.h) on the CPU.  TEST INFRASTRUCTURE: tests/test_rbf_table_cpu.py compiles it
// with g++ (address + undefined-behaviour sanitizers), runs it as a child process and checks what it prints.
//   check BETA_MULT CHANNELS : tables of CHANNELS channels (R = 96, the reference's means / betas at cutoff 10, betas x BETA_MULT, Xavier-scale
//                              weights of a 588 x 96 layer) filled and checked as k_rbf_table_fill / k_rbf_table_check do
//                              -> "worst midpoint deviation / range" "channels that pass" "channels"
//   locate D CUTOFF MASK     : -> idx frac factor w0 w1 w2 w3        (%a: exact)
//   eval BETA_MULT D         : one channel's value at distance D through rbt_locate / rbt_weights and the float32 FMAs of the edge kernel,
//                              and the float64 sum -> "table value" "float64 value" "range of the channel"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../oareactdiff_amd/csrc/oard_rbf_table.h"

static const int R = 96, C = 588;
static unsigned long long lcg = 0x9E3779B97F4A7C15ull;
static double uni() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0; }

struct Model { std::vector<float> means, betas, w; };
static Model model(double beta_mult, int channels) {
    Model m;
    const double start = exp(-10.0), end = 1.0;                  // rbf_buffers (spec.py): linspace(exp(-cutoff), 1, R), (2 / R (1 - start))^-2
    for (int k = 0; k < R; ++k) {
        m.means.push_back((float)(start + (end - start) * k / (R - 1)));
        m.betas.push_back((float)(beta_mult / ((2.0 / R * (end - start)) * (2.0 / R * (end - start)))));
    }
    const double a = sqrt(6.0 / (R + C));
    for (int i = 0; i < channels * R; ++i) m.w.push_back((float)((2.0 * uni() - 1.0) * a));
    return m;
}
static void fill(const Model& m, int c, std::vector<float>& f, std::vector<float>& d) {
    f.resize(RBT_N + 1); d.resize(RBT_N + 1);
    for (int i = 0; i <= RBT_N; ++i) {
        double v, dv;
        rbt_eval_f64(&m.w[(size_t)c * R], m.means.data(), m.betas.data(), R, (double)i * (1.0 / RBT_N), v, dv);
        rbt_entry(v, dv, f[i], d[i]);
    }
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "check")) {
        const int channels = atoi(argv[3]);
        const Model m = model(atof(argv[2]), channels);
        double worst = 0.0;
        int pass = 0;
        std::vector<float> f, d;
        for (int c = 0; c < channels; ++c) {
            fill(m, c, f, d);
            double e = 0.0, range = 0.0;
            for (int i = 0; i < RBT_N; ++i) {
                double v, dv;
                rbt_eval_f64(&m.w[(size_t)c * R], m.means.data(), m.betas.data(), R, ((double)i + 0.5) * (1.0 / RBT_N), v, dv);
                e = fmax(e, fabs(rbt_midpoint(f[i], d[i], f[i + 1], d[i + 1]) - v));
                range = fmax(range, fmax(fabs((double)f[i]), fabs(v)));
            }
            worst = fmax(worst, e / range);
            pass += rbt_channel_ok(e, range) ? 1 : 0;
        }
        printf("%.6e %d %d\n", worst, pass, channels);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "locate")) {
        const RbtAt at = rbt_locate(strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr));
        float w[4];
        rbt_weights(at, w);
        printf("%d %a %a %a %a %a %a\n", at.idx, at.frac, at.factor, (double)w[0], (double)w[1], (double)w[2], (double)w[3]);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "eval")) {
        const Model m = model(atof(argv[2]), 1);
        const double dist = strtod(argv[3], nullptr), cutoff = 10.0;
        std::vector<float> f, d;
        fill(m, 0, f, d);
        const RbtAt at = rbt_locate(dist, cutoff, 1.0);
        float w[4];
        rbt_weights(at, w);
        const float v = fmaf(w[3], d[at.idx + 1], fmaf(w[2], f[at.idx + 1], fmaf(w[1], d[at.idx], w[0] * f[at.idx])));
        double g, dg, range = 0.0;
        rbt_eval_f64(m.w.data(), m.means.data(), m.betas.data(), R, exp(-dist), g, dg);
        for (int i = 0; i <= RBT_N; ++i) range = fmax(range, fabs((double)f[i]));
        printf("%.9e %.9e %.9e\n", (double)v, g * at.factor, range);
        return 0;
    }
    fprintf(stderr, "usage: harness check BETA_MULT CHANNELS | locate D CUTOFF MASK | eval BETA_MULT D\n");
    return 2;
}
