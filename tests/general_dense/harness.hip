// One dense layer of the general-edge-list path, alone: HipExec::gemm (k_general_gemm_f64<RT> on the float64 matrix pipe, or og::Gemm on
// plain threads) on operands the caller lays out.  TEST INFRASTRUCTURE (tests/test_general_dense.py compiles it with hipcc and loads it with
// ctypes): HipExec and the kernel live in the anonymous namespace of oard_general.hip, so this unit includes that file whole - and with it
// re-defines the oard_graph_* entry points, which is why the test loads it with local symbol scope.  Nothing in the product builds or loads it.
#include "../../oareactdiff_amd/csrc/oard_general.hip"

extern "C" int general_dense_gemm(long long rows, int nout, int nseg,
                                  const float* x0, int ld0, int K0, const int32_t* idx0,
                                  const float* x1, int ld1, int K1, const int32_t* idx1,
                                  const float* x2, int ld2, int K2, const int32_t* idx2,
                                  const float* W, int ldw, const float* bias, float* Y, int ldy, int act, int mode, const float* resid, int ldr,
                                  const float* rowscale, int matrix_pipe, void* stream) {
    if (rows <= 0 || nseg < 1 || nseg > 3) return OARD_EINVAL;
    const og::Seg segs[3] = {og::seg(x0, ld0, K0, idx0), og::seg(x1, ld1, K1, idx1), og::seg(x2, ld2, K2, idx2)};
    og::Gemm k;                                          // filled as og::dense fills it
    memset(&k, 0, sizeof(k));
    k.rows = rows; k.nout = nout; k.nseg = nseg;
    for (int i = 0; i < nseg; ++i) k.seg[i] = segs[i];
    k.W = W; k.ldw = ldw; k.bias = bias; k.Y = Y; k.ldy = ldy; k.act = act; k.mode = mode; k.resid = resid; k.ldr = ldr; k.rowscale = rowscale;
    HipExec ex{(hipStream_t)stream, matrix_pipe != 0};
    return ex.gemm(k);
}
