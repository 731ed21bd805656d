// MXFP6 W6A8 linear layer for gfx950: MXFP6 weights (OCP E2M3 elements, E8M0 scale per block of 32 along K) against the MXFP8
// activations of the W4A8 layer (mxfp4_a8.hip: bie_mxfp8_quantize_act, unchanged), contracted on the block-scaled matrix instructions
// with an FP6 A operand and an E4M3 B operand; nothing is converted on either side (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A8 linear
// layer").
//
//   qweight uint8 [N, 3K/4]: per row K/32 blocks of 24 bytes in k order, code j of a block in bits 6 j .. 6 j + 5 of its little-endian
//       192-bit integer; code = sign << 5 | exponent (bias 1) << 3 | mantissa: +-{0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5}
//   scales uint8 [N, K/32]: E8M0, 2^(s - 127), 255 = a NaN block; e_col = bie_mxfp4_col_exp(scales)
//   quantiser, per block, in fp32: e = clamp(floor(log2 amax) - 2, -127, 127) (mx_block_scale), code = e2m3(clamp(|v * 2^-e|, 7.5)) round
//       to nearest, ties to the even code, the sign bit of v kept; an all-zero block: scale code 0, 24 zero bytes
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m3(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255
//
// How the instructions read this pair of operands was pinned on the card by tools/probe/probe_mx_fp6.hip (profiles/mxfp6_a8_probe.txt),
// A = FP6 E2M3 (cbsz 2, six VGPRs), B = E4M3 (blgp 0, eight VGPRs), both shapes:
//   (a1) the E4M3 operand is split in two 16-byte halves exactly as with an FP4 partner: with G = 2 / 4 lane groups, group g holds
//        k = 16 g .. + 15 in bytes 0 .. 15 and k = 16 G + 16 g .. + 15 in bytes 16 .. 31 (a8_frag serves unchanged)
//   (a2) the FP6 operand of lane group g holds k = 32 g .. 32 g + 31, element j in bits 6 j .. 6 j + 5, little-endian over the six
//        registers: the layout of qweight, so a fragment is a 24-byte copy
//   (b)  the scale byte of lane group g applies to block g of the instruction's K on either operand (byte select 0)
//   (c)  one instruction is inexact against float64: at worst 1853 fp32 ulps of its sum |products| (32x32x64; 790.25 in 16x16x128)
// The one-hot selector test of tests/test_mxfp6_a8_gpu.py holds the element maps in the suite.
//
// Decode form (mx6a8_decode_kernel, M <= 64): a workgroup per 16 output columns, K split over its 4 waves; every wave loads its weight
// fragments straight from qweight (non-temporal, three 8-byte pieces per lane: a block is only 8-byte aligned) and the x fragments from
// xq (two 16-byte loads 64 bytes apart), one 16x16x128 MFMA per 16 rows and 128 k; the four partial tiles are summed in LDS in a fixed
// order.  Prefill form (mx6a8_gemm_kernel): mx_scaled_gemm_tile (FP6 x E4M3) of mx_scaled_tile.cuh.  Both run behind mxa8_quantize_kernel (mxfp4_a8.hip).
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

int mxfp4_a8_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st);  // mxfp4_a8.hip

// ---- quantise / dequant -------------------------------------------------------------------------------------------------------------------
// One thread per 32-value block: amax, the block's scale 2^e (mx_block_scale), codes of w * 2^-e.  An all-zero block: scale 0, codes 0.
template <int DT>
__global__ __launch_bounds__(256) void mx6_quantize_kernel(const void* __restrict__ w, uint8_t* __restrict__ qw, uint8_t* __restrict__ sc, long nblk) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    float v[32];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        v[i] = dt_traits<DT>::load(w, b * 32 + i);
        amax = fmaxf(amax, fabsf(v[i]));
    }
    uint64_t words[3] = {0ull, 0ull, 0ull};
    uint32_t scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mx_block_scale(amax, inv);
        uint32_t c[32];
#pragma unroll
        for (int i = 0; i < 32; i++) c[i] = mx6_round_e2m3(fminf(fabsf(v[i] * inv), 7.5f)) | ((__float_as_uint(v[i]) >> 26) & 32u);
        mx6_pack(c, words);
    }
    uint2_t* out = reinterpret_cast<uint2_t*>(qw + b * MX6_BLOCK_BYTES);
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = uint2_t{(uint32_t)words[i], (uint32_t)(words[i] >> 32)};
    sc[b] = (uint8_t)scode;
}

// One thread per 32-value block: W in fp32 (exact), rounded once to the output dtype
template <int DT>
__global__ __launch_bounds__(256) void mx6_dequant_kernel(const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, void* __restrict__ w, long nblk) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const uint2_t* in = reinterpret_cast<const uint2_t*>(qw + b * MX6_BLOCK_BYTES);
    uint64_t words[3];
#pragma unroll
    for (int i = 0; i < 3; i++) words[i] = (uint64_t)in[i].x | ((uint64_t)in[i].y << 32);
    const float s = e8m0_f32(sc[b]);
#pragma unroll
    for (int i = 0; i < 32; i++) {  // the sign goes on after the multiply: a multiply fused into the 16-bit convert (a * b + 0) would turn -0.0 into +0.0
        const uint32_t c = mx6_code(words, i);
        dt_traits<DT>::store(w, b * 32 + i, __uint_as_float(__float_as_uint(mx6_e2m3(c & 31u) * s) | ((c & 32u) << 26)));
    }
}

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// Workgroup: columns 16 * blockIdx.x .. + 15 (reads past N clamped, never stored), rows 0 .. M - 1 (M <= 16 G).  Wave w takes the
// 128-k steps w, w + 4, ...; lane l holds column (row) l & 15, block l >> 4 of the step's weights and x scales, and the x bytes
// 16 (l >> 4) .. + 15 and 64 + 16 (l >> 4) .. + 15 of the step (a8_frag).  Blocks past K and rows past M enter as zero codes under
// scale 2^0 (code 127).  The weight fragment is the A operand, so a lane's accumulator holds 4 consecutive columns of one row of y.
template <int DT, int G>
__global__ __launch_bounds__(256) void mx6a8_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                           const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    __shared__ mxa4_v4f red[3][G][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const int n0 = blockIdx.x * 16;
    const long nl = min(n0 + r16, N - 1);
    const uint8_t* wrow = qw + nl * ((long)KB * MX6_BLOCK_BYTES);
    const uint8_t* srow = sc + nl * KB;
    mxa4_v4f acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);  // loads are clamped and unconditional, then masked
        const bool kin = kb < KB;
        const uint2_t* wp = reinterpret_cast<const uint2_t*>(wrow + (long)kc * MX6_BLOCK_BYTES);
        uint2_t w0 = __builtin_nontemporal_load(wp), w1 = __builtin_nontemporal_load(wp + 1), w2 = __builtin_nontemporal_load(wp + 2);
        int sw = __builtin_nontemporal_load(srow + kc);
        // this lane's x halves: 16 bytes of block b0 = kq >> 1 of the step and 16 bytes of block b0 + 2, at offset 16 (kq & 1) in each
        const int kb0 = s * 4 + (kq >> 1), kb1 = kb0 + 2;
        const bool in0 = kb0 < KB, in1 = kb1 < KB;
        const int o0 = min(kb0, KB - 1) * 32 + (kq & 1) * 16, o1 = min(kb1, KB - 1) * 32 + (kq & 1) * 16;
        uint4_t a0[G], a1[G];
        int sa[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const long m = min(g * 16 + r16, M - 1);
            a0[g] = *reinterpret_cast<const uint4_t*>(xq + m * K + o0);
            a1[g] = *reinterpret_cast<const uint4_t*>(xq + m * K + o1);
            sa[g] = xs[m * KB + kc];
        }
        if (!kin) {
            w0 = w1 = w2 = uint2_t{0u, 0u};
            sw = 127;
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool dead = g * 16 + r16 >= M;
            if (!in0 || dead) a0[g] = uint4_t{0u, 0u, 0u, 0u};
            if (!in1 || dead) a1[g] = uint4_t{0u, 0u, 0u, 0u};
            if (!kin || dead) sa[g] = 127;
        }
        const mxa4_v8i fw = a6_frag(w0, w1, w2);
#pragma unroll
        for (int g = 0; g < G; g++) acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, a8_frag(a0[g], a1[g]), acc[g], 2, 0, 0, sw, 0, sa[g]);
    }
    if (wave) {
#pragma unroll
        for (int g = 0; g < G; g++) red[wave - 1][g][lane] = acc[g];
    }
    __syncthreads();
    if (wave) return;
    // C/D: D column (= row m of the 16) = lane & 15, D row (= column n of y) = 4 (lane >> 4) + r: four consecutive n of one row of y (mx_store4)
    const int n = n0 + 4 * kq;
    if (n >= N) return;
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int m = g * 16 + r16;
        if (m >= M) continue;
        const mxa4_v4f p1 = red[0][g][lane], p2 = red[1][g][lane], p3 = red[2][g][lane];
        const bool rbad = row_flag[m] != 0;
        uint16_t* yr = reinterpret_cast<uint16_t*>(y) + (long)m * N;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = ((acc[g][r] + p1[r]) + p2[r]) + p3[r];
        mx_store4<DT>(v, rbad, ecol, bias, n, yr, n, N);
    }
}

// ---- prefill form -----------------------------------------------------------------------------------------------------------------------
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void mx6a8_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_fp6, mx_op_e4m3>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= A6_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.  The plan's bound was
// measured, not inherited from W4A8 (tools/mxfp6_a8_bench.py, profiles/mxfp6_a8_bench.jsonl, the "sweep" rows: both forms forced at
// M = 8 .. 64, alternated, the median of three passes, the quantise launch included, fp16 and bf16 alike within 1 %): the decode form
// was ahead at every M <= 48 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 (0.29 - 0.98 x the prefill form's time; the closest is
// M = 48 on 4096 -> 11008, 43.4 against 44.3 us), and at M = 64 on two of the three shapes (22.3 / 42.6 us against 44.3 / 104.9); on
// 4096 -> 11008 it was 12 % behind at M = 64 (50.6 against 45.0 us).  The bound stays at 64: what the prefill form would lose there
// on the other two shapes (99 % and 146 %) outweighs that.
constexpr int A6_DECODE_ROWS = 64;
constexpr int A6_PLAN_ROWS = 64;

int mxfp6_quantize_launch(const void* w, uint8_t* qw, uint8_t* sc, long N, long K, int dtype, hipStream_t st) {
    const long nblk = N * (K >> 5);
    const dim3 grid((unsigned)cdivl(nblk, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx6_quantize_kernel<BIE_F16>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx6_quantize_kernel<BIE_BF16>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    else hipLaunchKernelGGL(mx6_quantize_kernel<BIE_F32>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    return check_launch("mx6_quantize_kernel");
}

int mxfp6_dequant_launch(const uint8_t* qw, const uint8_t* sc, void* w, long N, long K, int dtype, hipStream_t st) {
    const long nblk = N * (K >> 5);
    const dim3 grid((unsigned)cdivl(nblk, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx6_dequant_kernel<BIE_F16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx6_dequant_kernel<BIE_BF16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else hipLaunchKernelGGL(mx6_dequant_kernel<BIE_F32>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    return check_launch("mx6_dequant_kernel");
}

// Workspace of bie_mxfp6_a8_linear_forward, the layout of the W4A8 one: xq [M, K] (16-byte aligned), xs [M, K/32], row_flag [M]
struct mx6a8_layer {
    using act = mx_act_e4m3;  // the W4A8 layer's quantiser and workspace layout
    static constexpr const char* form_knob = "BIE_MXFP6_A8_FORM";
    static constexpr int decode_rows = A6_DECODE_ROWS, plan_rows = A6_PLAN_ROWS;
    static constexpr const char* decode_name = "mx6a8_decode_kernel";
    static constexpr const char* gemm_name = "mx6a8_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mx6a8_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mx6a8_gemm_kernel<DT, W, W>; }
};

bool mxfp6_a8_decode_ok(long M) { return mx_dense_decode_ok<mx6a8_layer>(M); }
int mxfp6_a8_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mx6a8_layer>(M); }
size_t mxfp6_a8_workspace_bytes(long M, long K) { return mx_dense_workspace_bytes<mx6a8_layer>(M, K); }

int mxfp6_a8_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mx6a8_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp6_a8_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mx6a8_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
