// MXFP4 W4A8 linear layer for gfx950: the MXFP4 weights of mxfp4.hip against activations quantised to MXFP8 (E4M3 elements, E8M0 block
// scales) on the fly, contracted on the block-scaled matrix instructions with an FP4 A operand and an E4M3 B operand
// (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A8 linear layer").
//
//   xq uint8 [M, K], xs uint8 [M, K/32]: x quantised per row and block of 32 by the OCP MX v1.0 rule with E4M3 elements (emax = 8):
//       e = clamp(floor(log2 amax) - 8, -127, 127), code = e4m3fn(clamp(v * 2^-e, +-448)) round to nearest even, never a NaN code
//   row_flag uint8 [M]: 1 where row m of x holds a NaN or +-inf (its codes are unspecified), else 0
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m1(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255 (a weight block with scale code 255)
//
// How the instructions read a mixed pair of operands was pinned on the card by tools/probe/probe_mx_a8.hip
// (profiles/mxfp4_a8_probe.txt), A = FP4 (cbsz 4, four VGPRs), B = E4M3 (blgp 0, eight VGPRs).  The FP4 operand is read as in the
// W4A4 kernels: lane group g (l >> 5 in v_mfma_scale_f32_32x32x64_f8f6f4, l >> 4 in v_mfma_scale_f32_16x16x128_f8f6f4) holds the
// elements k = 32 g .. 32 g + 31 of the instruction's K.  The E4M3 operand is NOT one block per lane: with G = 2 / 4 lane groups,
// group g holds k = 16 g .. + 15 in bytes 0 .. 15 and k = 16 G + 16 g .. + 15 in bytes 16 .. 31.  xq stays row-major E4M3 in memory
// and nothing is permuted in registers: a lane loads its two 16-byte halves from two places of the row (a8_frag of
// mxfp4_a8_common.cuh).  The scale byte of lane group g applies to block g of the instruction's K on either operand; the kernels keep
// it in byte 0 of the scale register (byte select 0).  The one-hot selector test of tests/test_mxfp4_a8_gpu.py holds the element map
// in the suite.
//
// Quantise kernel (mxa8_quantize_kernel): a workgroup per row of x, a block of 32 per 4 lanes (16-byte loads, 8 bytes of codes per
// lane), the block maximum over the 4 lanes on the DPP network, the row's non-finite flag through the workgroup's barrier.
// Decode form (mxa8_decode_kernel, M <= 64): mx_scaled_decode_rows (FP4 x E4M3) of mx_scaled_decode.cuh; a lane's weight fragment is
// one non-temporal 16-byte load, its x fragment two 16-byte loads 64 bytes apart.
// Prefill form (mxa8_gemm_kernel): mx_scaled_gemm_tile (FP4 x E4M3) of mx_scaled_tile.cuh, a (64 WM) x (64 WN) tile GEMM on 32x32x64, 4 waves as 2 x 2,
// codes and scale bytes staged through registers into double-buffered LDS (128 k per stage), on the rows m0 .. of xq / xs.
#include "mxfp4_a8_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- activation quantiser -------------------------------------------------------------------------------------------------------------
// Workgroup = one row (mx_quantize_row of mxfp4_a8_common.cuh).
template <int DT>
__global__ __launch_bounds__(256) void mxa8_quantize_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ xq, uint8_t* __restrict__ xs,
                                                            uint8_t* __restrict__ row_flag, int K) {
    const long m = blockIdx.x;
    int bad = 0;
    mx_quantize_row<DT>(mx_op_e4m3{}, x + m * K, K, xq + m * K, xs + m * (K >> 5), bad);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) row_flag[m] = (uint8_t)(bad ? 1 : 0);
}

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// A workgroup per 16 output columns, M <= 16 G rows (mx_scaled_decode_rows).
template <int DT, int G>
__global__ __launch_bounds__(256) void mxa8_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                          const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                          const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    mx_scaled_decode_rows<DT, G, mx_op_fp4, mx_op_e4m3>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K);
}

// ---- prefill form -----------------------------------------------------------------------------------------------------------------------
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void mxa8_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                        const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                        const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_fp4, mx_op_e4m3>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= A8_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.  The plan's bound was
// measured (tools/mxfp4_a8_bench.py, profiles/mxfp4_a8_bench.jsonl, the "sweep" rows, both forms forced at M = 8 .. 64, the quantise
// launch included, fp16 and bf16 alike): the decode form was ahead at every M <= 32 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096
// (0.26 - 0.76 x the prefill form's time), and at M = 48 and 64 on two of the three shapes (M = 64: 22.8 / 42.8 us against 40.0 / 85.8);
// on 4096 -> 11008 it was 3 % behind at M = 48 (40.5 against 39.4 us) and 17 % behind at M = 64 (47.2 against 40.4).  The bound stays
// at 64: what the prefill form would lose there on the other two shapes (75 % and 100 %) outweighs that.
constexpr int A8_DECODE_ROWS = 64;
constexpr int A8_PLAN_ROWS = 64;

int mxfp4_a8_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st) {
    const uint16_t* xp = reinterpret_cast<const uint16_t*>(x);
    if (dtype == BIE_F16) hipLaunchKernelGGL(mxa8_quantize_kernel<BIE_F16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    else hipLaunchKernelGGL(mxa8_quantize_kernel<BIE_BF16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    return check_launch("mxa8_quantize_kernel");
}

// Workspace of bie_mxfp4_a8_linear_forward: xq [M, K] (16-byte aligned; M * K is a multiple of 32), xs [M, K/32], row_flag [M]
struct mxa8_layer {
    using act = mx_act_e4m3;
    static constexpr const char* form_knob = "BIE_MXFP4_A8_FORM";
    static constexpr int decode_rows = A8_DECODE_ROWS, plan_rows = A8_PLAN_ROWS;
    static constexpr const char* decode_name = "mxa8_decode_kernel";
    static constexpr const char* gemm_name = "mxa8_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mxa8_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mxa8_gemm_kernel<DT, W, W>; }
};

bool mxfp4_a8_decode_ok(long M) { return mx_dense_decode_ok<mxa8_layer>(M); }
int mxfp4_a8_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mxa8_layer>(M); }
size_t mxfp4_a8_workspace_bytes(long M, long K) { return mx_dense_workspace_bytes<mxa8_layer>(M, K); }

int mxfp4_a8_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mxa8_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp4_a8_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mxa8_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
