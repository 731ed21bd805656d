// MXFP4 W4A4 linear layer for gfx950: the MXFP4 weights of mxfp4.hip against activations quantised to MXFP4 on the fly, contracted on the
// block-scaled matrix instructions with REAL block scales (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A4 linear layer").
//
//   xq uint8 [M, K/2], xs uint8 [M, K/32]: x quantised per row and block of 32 by the OCP MX v1.0 rule of the weight quantiser (mxfp4_common.cuh)
//   row_flag uint8 [M]: 1 where row m of x holds a NaN or +-inf (its codes are unspecified), else 0
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e2m1(xq) * e2m1(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255 (a weight block with scale code 255)
//
// How the instructions read their scale operands was pinned on the card by tools/probe/probe_mx_scale.hip
// (profiles/mxfp4_a4_scale_probe.txt): in v_mfma_scale_f32_32x32x64_f8f6f4 lane l holds the 32 values of row (column) l & 31, k-block
// l >> 5, and its OWN scale byte applies to exactly those 32 values; in v_mfma_scale_f32_16x16x128_f8f6f4 row l & 15, k-block l >> 4.
// A lane's operand is therefore 16 contiguous bytes of qweight [N, K/2] (or xq) and its scale the matching byte of scales [N, K/32]:
// nothing is converted or re-arranged.  The kernels keep the lane's scale in byte 0 of the scale register (byte select 0).
//
// Quantise kernel (mxa4_quantize_kernel): a workgroup per row of x, a block of 32 per 4 lanes (16-byte loads, one dword of codes per
// lane), the block maximum over the 4 lanes on the DPP network, the row's non-finite flag through the workgroup's barrier.
// Decode form (mxa4_decode_kernel, M <= 64): a workgroup per 16 output columns, K split over its 4 waves; every wave loads its B
// fragments straight from qweight (non-temporal, 16 bytes per lane) and the x fragments from xq (cache-resident), one
// 16x16x128 MFMA per 16 rows and 128 k; the four partial tiles are summed in LDS.
// Prefill form (mxa4_gemm_kernel): mx_scaled_gemm_tile (FP4 x FP4) of mx_scaled_tile.cuh, a (64 WM) x (64 WN) tile GEMM on 32x32x64, 4 waves as 2 x 2,
// packed codes and scale bytes staged through registers into double-buffered LDS (128 k per stage), on the rows m0 .. of xq / xs.
#include "mxfp4_a4_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- activation quantiser -------------------------------------------------------------------------------------------------------------
// Workgroup = one row (mx_quantize_row of mxfp4_a4_common.cuh).
template <int DT>
__global__ __launch_bounds__(256) void mxa4_quantize_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ xq, uint8_t* __restrict__ xs,
                                                            uint8_t* __restrict__ row_flag, int K) {
    const long m = blockIdx.x;
    int bad = 0;
    mx_quantize_row<DT>(mx_op_fp4{}, x + m * K, K, xq + m * (K >> 1), xs + m * (K >> 5), bad);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) row_flag[m] = (uint8_t)(bad ? 1 : 0);
}

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// Workgroup: columns 16 * blockIdx.x .. + 15 (reads past N clamped, never stored), rows 0 .. M - 1 (M <= 16 G).  Wave w takes the
// 128-k steps w, w + 4, ...; lane l holds column (row) l & 15 and block l >> 4 of the step.  Blocks past K and rows past M enter as zero
// codes under scale 2^0.
template <int DT, int G>
__global__ __launch_bounds__(256) void mxa4_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                          const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                          const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    __shared__ mxa4_v4f red[3][G][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const int n0 = blockIdx.x * 16;
    const long nl = min(n0 + r16, N - 1);
    const uint8_t* wrow = qw + nl * (K >> 1);
    const uint8_t* srow = sc + nl * KB;
    mxa4_v4f acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);  // loads are clamped and unconditional, then masked
        const bool kin = kb < KB;
        uint4_t b = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wrow) + kc);
        int sb = __builtin_nontemporal_load(srow + kc);
        uint4_t a[G];
        int sa[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const long m = min(g * 16 + r16, M - 1);
            a[g] = reinterpret_cast<const uint4_t*>(xq + m * (K >> 1))[kc];
            sa[g] = xs[m * KB + kc];
        }
        if (!kin) {
            b = uint4_t{0u, 0u, 0u, 0u};
            sb = 127;
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (!kin || g * 16 + r16 >= M) {
                a[g] = uint4_t{0u, 0u, 0u, 0u};
                sa[g] = 127;
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++)
            acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a4_frag(a[g]), a4_frag(b), acc[g], 4, 4, 0, sa[g], 0, sb);
    }
    if (wave) {
#pragma unroll
        for (int g = 0; g < G; g++) red[wave - 1][g][lane] = acc[g];
    }
    __syncthreads();
    if (wave) return;
    // C/D: column n = lane & 15, row m = 4 (lane >> 4) + r
    const int n = n0 + r16;
    if (n >= N) return;
    const bool ncol = ecol[n] == 255u;
    const float bv = bias ? dt_traits<DT>::load(bias, n) : 0.0f;
#pragma unroll
    for (int g = 0; g < G; g++) {
        const mxa4_v4f p1 = red[0][g][lane], p2 = red[1][g][lane], p3 = red[2][g][lane];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = g * 16 + kq * 4 + r;
            if (m < M) {
                float v = ((acc[g][r] + p1[r]) + p2[r]) + p3[r];
                if (ncol || row_flag[m]) v = a4_nan();
                if (bias) v += bv;
                dt_traits<DT>::store(y, (long)m * N + n, v);
            }
        }
    }
}

// ---- prefill form -----------------------------------------------------------------------------------------------------------------------
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void mxa4_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                        const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                        const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_fp4, mx_op_fp4>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= A4_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.  The plan's bound was
// measured (tools/mxfp4_a4_bench.py, profiles/mxfp4_a4_bench.jsonl, the "sweep" rows, both forms forced at M = 8 .. 64, the quantise
// launch included): the decode form was ahead at every M <= 48 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 in fp16 and bf16, and at
// M = 64 on two of the three shapes (19.5 / 37.4 us against 37.4 / 80.9); on 4096 -> 11008 it was 2 % behind there (39.1 against 38.2).
constexpr int A4_DECODE_ROWS = 64;
constexpr int A4_PLAN_ROWS = 64;

int mxfp4_a4_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st) {
    const uint16_t* xp = reinterpret_cast<const uint16_t*>(x);
    if (dtype == BIE_F16) hipLaunchKernelGGL(mxa4_quantize_kernel<BIE_F16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    else hipLaunchKernelGGL(mxa4_quantize_kernel<BIE_BF16>, dim3((unsigned)M), dim3(256), 0, st, xp, xq, xs, row_flag, (int)K);
    return check_launch("mxa4_quantize_kernel");
}

// Workspace of bie_mxfp4_a4_linear_forward: xq [M, K/2] (16-byte aligned), xs [M, K/32] from a 16-byte boundary, row_flag [M]
struct mxa4_layer {
    using act = mx_act_fp4;
    static constexpr const char* form_knob = "BIE_MXFP4_A4_FORM";
    static constexpr int decode_rows = A4_DECODE_ROWS, plan_rows = A4_PLAN_ROWS;
    static constexpr const char* decode_name = "mxa4_decode_kernel";
    static constexpr const char* gemm_name = "mxa4_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mxa4_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mxa4_gemm_kernel<DT, W, W>; }
};

bool mxfp4_a4_decode_ok(long M) { return mx_dense_decode_ok<mxa4_layer>(M); }
int mxfp4_a4_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mxa4_layer>(M); }
size_t mxfp4_a4_workspace_bytes(long M, long K) { return mx_dense_workspace_bytes<mxa4_layer>(M, K); }

int mxfp4_a4_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mxa4_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp4_a4_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mxa4_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
