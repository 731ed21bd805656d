// MXFP4 W4A6 linear layer for gfx950: the MXFP4 weights of mxfp4.hip (qweight / scales, unchanged) against activations quantised to
// MXFP6 (OCP E2M3 elements, E8M0 block scales) on the fly by the W6A6 layer's quantiser, contracted on the block-scaled matrix
// instructions with an FP4 A operand and an FP6 B operand: the FP4 matrix rate (an E4M3 operand costs twice the cycles) at the
// activation accuracy of MXFP8 (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A6 linear layer").
//
//   xq6 uint8 [M, 3K/4], xs uint8 [M, K/32], row_flag uint8 [M]: the outputs of mx6a6_quantize_kernel (mxfp6_a6.hip), byte for byte:
//       e = clamp(floor(log2 amax) - 2, -127, 127), code = e2m3(clamp(|v * 2^-e|, 7.5)) round to nearest, ties to the even code;
//       24 bytes per block, code j in bits 6 j .. 6 j + 5; row_flag[m] = 1 where row m of x holds a NaN or +-inf
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m1(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255 (a weight block with scale code 255)
//
// How the instructions read this mixed pair was pinned on the card by tools/probe/probe_mx_fp4x6.hip (profiles/mxfp4_a6_probe.txt),
// A = FP4 (cbsz 4, four VGPRs), B = FP6 E2M3 (blgp 2, six VGPRs), both shapes:
//   (a)  either operand is one block of 32 per lane: lane group g (l >> 5 in v_mfma_scale_f32_32x32x64_f8f6f4, l >> 4 in
//        v_mfma_scale_f32_16x16x128_f8f6f4) holds k = 32 g .. 32 g + 31; the FP4 element j sits in bits 4 j .. 4 j + 3 of the four
//        registers, the FP6 element j in bits 6 j .. 6 j + 5 of the six, little-endian: the layouts of qweight and of xq6, so the weight
//        fragment is a 16-byte copy and the x fragment a 24-byte copy (unlike the E4M3 B operand of W4A8, which is split in two halves)
//   (b)  the scale byte of lane group g applies to block g of the instruction's K on either operand (byte select 0)
//   (c)  under one scale an instruction is exact (the products lie on a 2^-4 grid); where its blocks differ in scale it is inexact
//        against float64, the figure in tests/mxfp4_a6_ref.py (PROBE_ULPS)
// The one-hot selector test of tests/test_mxfp4_a6_gpu.py holds the element maps in the suite.
//
// There is no quantise kernel here: mxfp6_a6_quantize_launch is called as it stands.  Decode form (mx4a6_decode_kernel, M <= 64):
// mx_scaled_decode_rows (FP4 x FP6) of mx_scaled_decode.cuh; a lane's weight fragment is one non-temporal 16-byte load and its x
// fragment its block's 24 bytes in three 8-byte loads.  Prefill form (mx4a6_gemm_kernel): mx_scaled_gemm_tile (FP4 x FP6) of mx_scaled_tile.cuh.
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// A workgroup per 16 output columns, M <= 16 G rows (mx_scaled_decode_rows).
template <int DT, int G>
__global__ __launch_bounds__(256) void mx4a6_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                           const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    mx_scaled_decode_rows<DT, G, mx_op_fp4, mx_op_fp6>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K);
}

// ---- prefill form -----------------------------------------------------------------------------------------------------------------------
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void mx4a6_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_fp4, mx_op_fp6>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= A46_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.
// The plan's bound is measured (tools/mxfp4_a6_bench.py, profiles/mxfp4_a6_bench.jsonl, the "sweep" rows: both forms forced at M = 8 .. 64,
// alternated, the median of three passes, the quantise launch included, fp16 and bf16 alike within 2 %): the decode form was ahead at
// every M <= 32 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 (0.27 - 0.74 x the prefill form's time), level at M = 48 on 4096 -> 11008
// (40.8 against 41.3 us) and ahead there on the other two (0.51 / 0.39), and at M = 64 ahead on two of the three shapes (22.6 / 41.3 us
// against 41.2 / 92.4) and 13 % behind on 4096 -> 11008 (47.7 against 42.1 us).  The bound stays at 64: what the prefill form would
// lose there on the other two shapes (82 % and 124 %) outweighs that, as for W4A8 and W6A6.
constexpr int A46_DECODE_ROWS = 64;
constexpr int A46_PLAN_ROWS = 64;

struct mx4a6_layer {
    using act = mx_act_fp6;  // the W6A6 layer's quantiser and workspace layout
    static constexpr const char* form_knob = "BIE_MXFP4_A6_FORM";
    static constexpr int decode_rows = A46_DECODE_ROWS, plan_rows = A46_PLAN_ROWS;
    static constexpr const char* decode_name = "mx4a6_decode_kernel";
    static constexpr const char* gemm_name = "mx4a6_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mx4a6_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mx4a6_gemm_kernel<DT, W, W>; }
};

bool mxfp4_a6_decode_ok(long M) { return mx_dense_decode_ok<mx4a6_layer>(M); }
int mxfp4_a6_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mx4a6_layer>(M); }
size_t mxfp4_a6_workspace_bytes(long M, long K) { return mx_dense_workspace_bytes<mx4a6_layer>(M, K); }

int mxfp4_a6_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mx4a6_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp4_a6_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mx4a6_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
