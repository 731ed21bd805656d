// MXFP6 W6A6 linear layer for gfx950: MXFP6 weights (OCP E2M3 elements, E8M0 scale per block of 32 along K: the qweight / scales of
// mxfp6_a8.hip, unchanged) against activations quantised to the SAME format on the fly, contracted on the block-scaled matrix
// instructions with two FP6 operands, which run at the FP4 rate where any E4M3 operand costs twice that (include/bie_hip.h,
// INTEGRATION.md "MXFP6 W6A6 linear layer").
//
//   xq6 uint8 [M, 3K/4], xs uint8 [M, K/32]: x per row and block of 32 by exactly the weight quantiser's rule, in the weight's byte format:
//       e = clamp(floor(log2 amax) - 2, -127, 127), code = e2m3(clamp(|v * 2^-e|, 7.5)) round to nearest, ties to the even code, the sign
//       bit of v kept; 24 bytes per block, code j in bits 6 j .. 6 j + 5; an all-zero block: scale code 0, 24 zero bytes
//   row_flag uint8 [M]: 1 where row m of x holds a NaN or +-inf (its codes are unspecified), else 0
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m3(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255
//
// How the instructions read two FP6 operands was pinned on the card by tools/probe/probe_mx_fp6x6.hip (profiles/mxfp6_a6_probe.txt),
// A = B = FP6 E2M3 (cbsz 2, blgp 2, six VGPRs each), both shapes:
//   (a)  the B operand is read as the A operand is: lane group g holds k = 32 g .. 32 g + 31, element j in bits 6 j .. 6 j + 5,
//        little-endian over the six registers: the layout of qweight and of xq6, so either fragment is a 24-byte copy
//   (b)  the scale byte of lane group g applies to block g of the instruction's K on either operand (byte select 0)
//   (c)  under one scale an instruction is exact (the products lie on a 2^-6 grid); where its blocks differ in scale it is inexact
//        against float64, the figure in tests/mxfp6_a6_ref.py (PROBE_ULPS)
// The one-hot selector test of tests/test_mxfp6_a6_gpu.py holds the element maps in the suite.
//
// Quantise kernel (mx6a6_quantize_kernel): a workgroup per row of x, a block of 32 per 4 lanes (16-byte loads), the block maximum over
// the quad on the DPP network, 48 bits of codes per lane; lane i < 3 of a quad takes its right neighbour's 48 bits over the DPP network
// and stores the i-th 8 bytes of the block; the row's non-finite flag through the workgroup's barrier.
// Decode form (mx6a6_decode_kernel, M <= 64): mx_scaled_decode_rows (FP6 x FP6) of mx_scaled_decode.cuh; a lane's x fragment is its
// block's 24 bytes in three 8-byte loads, as its weight fragment is (non-temporal).  Prefill form (mx6a6_gemm_kernel): mx_scaled_gemm_tile (FP6 x FP6) of mx_scaled_tile.cuh.
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- activation quantiser -------------------------------------------------------------------------------------------------------------
// Workgroup = one row (mx_quantize_row of mxfp6_common.cuh).
template <int DT>
__global__ __launch_bounds__(256) void mx6a6_quantize_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ xq, uint8_t* __restrict__ xs,
                                                             uint8_t* __restrict__ row_flag, int K) {
    const long m = blockIdx.x;
    const int KB = K >> 5;
    int bad = 0;
    mx_quantize_row<DT>(mx_op_fp6{}, x + m * K, K, xq + m * ((long)KB * MX6_BLOCK_BYTES), xs + m * KB, bad);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) row_flag[m] = (uint8_t)(bad ? 1 : 0);
}

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// A workgroup per 16 output columns, M <= 16 G rows (mx_scaled_decode_rows).
template <int DT, int G>
__global__ __launch_bounds__(256) void mx6a6_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                           const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    mx_scaled_decode_rows<DT, G, mx_op_fp6, mx_op_fp6>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K);
}

// ---- prefill form -----------------------------------------------------------------------------------------------------------------------
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void mx6a6_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_fp6, mx_op_fp6>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= A66_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.  The plan's bound is
// measured (tools/mxfp6_a6_bench.py, profiles/mxfp6_a6_bench.jsonl, the "sweep" rows: both forms forced at M = 8 .. 64, alternated, the
// median of three passes, the quantise launch included, fp16 and bf16 alike within 1 %): the decode form was ahead at every M <= 32 on
// 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 (0.24 - 0.80 x the prefill form's time), level at M = 48 on 4096 -> 11008 (45.6 against
// 45.8 us), and at M = 64 ahead on two of the three shapes (24.4 / 48.0 us against 45.3 / 108.7) and 13 % behind on 4096 -> 11008 (52.6
// against 46.7 us).  The bound stays at 64: what the prefill form would lose there on the other two shapes (86 % and 127 %) outweighs
// that, as for W6A8.
constexpr int A66_DECODE_ROWS = 64;
constexpr int A66_PLAN_ROWS = 64;

int mxfp6_a6_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st) {
    const uint16_t* xp = reinterpret_cast<const uint16_t*>(x);
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx6a6_quantize_kernel<BIE_F16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    else hipLaunchKernelGGL(mx6a6_quantize_kernel<BIE_BF16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    return check_launch("mx6a6_quantize_kernel");
}

// Workspace of bie_mxfp6_a6_linear_forward: xq6 [M, 3K/4] (16-byte aligned), xs [M, K/32], row_flag [M]
struct mx6a6_layer {
    using act = mx_act_fp6;
    static constexpr const char* form_knob = "BIE_MXFP6_A6_FORM";
    static constexpr int decode_rows = A66_DECODE_ROWS, plan_rows = A66_PLAN_ROWS;
    static constexpr const char* decode_name = "mx6a6_decode_kernel";
    static constexpr const char* gemm_name = "mx6a6_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mx6a6_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mx6a6_gemm_kernel<DT, W, W>; }
};

bool mxfp6_a6_decode_ok(long M) { return mx_dense_decode_ok<mx6a6_layer>(M); }
int mxfp6_a6_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mx6a6_layer>(M); }
size_t mxfp6_a6_workspace_bytes(long M, long K) { return mx_dense_workspace_bytes<mx6a6_layer>(M, K); }

int mxfp6_a6_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mx6a6_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp6_a6_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mx6a6_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
