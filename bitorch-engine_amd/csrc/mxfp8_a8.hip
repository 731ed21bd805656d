// MXFP8 W8A8 linear layer for gfx950: MXFP8 weights (OCP e4m3fn elements, E8M0 block scales, one byte per weight, row-major) against
// the MXFP8 activations of mxa8_quantize_kernel (mxfp4_a8.hip, unchanged), contracted on the block-scaled matrix instructions with an
// E4M3 A operand and an E4M3 B operand (include/bie_hip.h, INTEGRATION.md "MXFP8 W8A8 linear layer").
//
//   qweight uint8 [N, K], scales uint8 [N, K/32]: W[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k/32] - 127); scale code 255 = a NaN block
//   xq uint8 [M, K], xs uint8 [M, K/32], row_flag uint8 [M]: the outputs of bie_mxfp8_quantize_act, byte for byte
//   y[m, n] = dt( sum_b 2^(xs[m, b] + scales[n, b] - 254) * (sum_{k in b} e4m3(xq) * e4m3(qweight)) + bias[n] )
//   y[m, :] = NaN where row_flag[m]; y[:, n] = NaN where e_col[n] == 255
//
// How the instructions read two byte operands was pinned on the card by tools/probe/probe_mx_fp8x8.hip (profiles/mxfp8_a8_probe.txt),
// A = E4M3 (cbsz 0, eight VGPRs), B = E4M3 (blgp 0, eight VGPRs), both shapes, G = 2 (32x32x64) or 4 (16x16x128) lane groups:
//   (a)  byte j of lane group g of A multiplies byte j of lane group g of B
//   (b)  on either operand bytes 0 .. 15 of lane group g lie in block g / 2 of the instruction's K and bytes 16 .. 31 in block
//        G / 2 + g / 2 (k = 16 g .. + 15 and k = 16 G + 16 g .. + 15: a8_frag's map, which the W4A8 probe found for the B side beside an
//        FP4 A); the scale byte of lane group g applies to block g (byte select 0).  Both operands stay row-major in memory and a lane
//        takes its two 16-byte halves from two places of the row
//   (c)  the accumulation error of one instruction: the figure in tests/mxfp8_a8_ref.py (PROBE_ULPS)
//   (d)  a NaN code (0x7F / 0xFF) in either operand makes every output of its row / column NaN, whatever the partner holds, and leaves
//        the other outputs alone; bie_mx8_quantize never writes one
// The one-hot selector test of tests/test_mxfp8_a8_gpu.py holds the element map in the suite.
//
// Weight quantiser (mx8_quantize_kernel): a8_quantize_unit's rule per 8-value unit (the four lanes of a quad hold a block; the quad
// maximum on DPP, the clamp before v_cvt_pk_fp8_f32) on fp16 / bf16 / fp32 rows, plus the NaN-block rule: a block with a NaN or +-inf
// gets scale code 255 and zero bytes.  Dequant (mx8_dequant_kernel): one thread per block, exact in fp32, one rounding to the dtype.
// Decode form (mx8a8_decode_kernel, M <= 64): mxa8_decode_kernel's structure: a workgroup per 16 output columns, K split over its 4
// waves, one 16x16x128 MFMA per 16 rows and 128 k; a lane's weight fragment is 32 bytes per k-step in two non-temporal 16-byte loads
// 64 bytes apart, so that the 64 lanes of a wave read one whole 128-byte line of each of their 16 weight rows per step.
// Prefill form (mx8a8_gemm_kernel): mx_scaled_gemm_tile (E4M3 x E4M3) of mx_scaled_tile.cuh on 32x32x64, 4 waves as 2 x 2, double-buffered LDS.
#include "mxfp4_a8_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

int mxfp4_a8_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st);  // mxfp4_a8.hip

// ---- weight quantiser / dequant -----------------------------------------------------------------------------------------------------------
// a8_quantize_unit's rule on 8 fp32 values: the same block scale, clamp and convert, so that an fp32 row whose values are fp16 / bf16
// values gives the bytes of the 16-bit path.  All lanes of the quad must call it together.
__device__ __forceinline__ void mx8_quantize_unit_f32(const float (&v)[8], int& bad, uint2_t& codes, uint32_t& scode) {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        amax = fmaxf(amax, fabsf(v[i]));
        bad |= (__float_as_uint(v[i]) & 0x7f800000u) == 0x7f800000u;
    }
    amax = a4_dpp_max<0xB1>(amax);  // quad_perm [1, 0, 3, 2]
    amax = a4_dpp_max<0x4E>(amax);  // quad_perm [2, 3, 0, 1]
    codes = uint2_t{0u, 0u};
    scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mxa8_block_scale(amax, inv);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[0], inv), a8_clamp(v[1], inv), lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[2], inv), a8_clamp(v[3], inv), lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[4], inv), a8_clamp(v[5], inv), hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[6], inv), a8_clamp(v[7], inv), hi, true);
        codes = uint2_t{(uint32_t)lo, (uint32_t)hi};
    }
}

// Thread u takes the 8-value unit u of the flat [N * K] weights; the 4 lanes of a quad hold one block of 32 (nunits is a multiple of 4,
// so whole quads are in or out).  w is 4-byte aligned only: the unit is loaded dword by dword.
template <int DT>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(const void* __restrict__ w, uint8_t* __restrict__ qw, uint8_t* __restrict__ sc, long nunits) {
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= nunits) return;
    int bad = 0;
    uint2_t codes;
    uint32_t scode;
    if constexpr (DT == BIE_F32) {
        const float* p = reinterpret_cast<const float*>(w) + u * 8;
        const float v[8] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
        mx8_quantize_unit_f32(v, bad, codes, scode);
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(w) + u * 4;
        a8_quantize_unit<DT>(uint4_t{p[0], p[1], p[2], p[3]}, bad, codes, scode);
    }
    // the NaN-block rule: a non-finite value anywhere in the quad's block -> scale code 255, zero bytes
    float b = bad ? 1.0f : 0.0f;
    b = a4_dpp_max<0xB1>(b);
    b = a4_dpp_max<0x4E>(b);
    if (b != 0.0f) {
        codes = uint2_t{0u, 0u};
        scode = 255u;
    }
    *reinterpret_cast<uint2_t*>(qw + u * 8) = codes;
    if ((u & 3) == 0) sc[u >> 2] = (uint8_t)scode;
}

// One thread per 32-value block: e4m3(code) * 2^(s - 127) in fp32 (exact), rounded once to the output dtype.  A NaN code and scale code
// 255 decode to NaN.
template <int DT>
__global__ __launch_bounds__(256) void mx8_dequant_kernel(const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, void* __restrict__ w, long nblk) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const uint4_t* in = reinterpret_cast<const uint4_t*>(qw + b * 32);
    const uint4_t lo = in[0], hi = in[1];
    const uint32_t words[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const float s = e8m0_f32(sc[b]);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int wd = (int)(words[i] & 0x7f7f7f7fu);  // magnitudes; the sign goes on after the multiply, as in mx6_dequant_kernel
        const float m[4] = {__builtin_amdgcn_cvt_f32_fp8(wd, 0), __builtin_amdgcn_cvt_f32_fp8(wd, 1), __builtin_amdgcn_cvt_f32_fp8(wd, 2),
                            __builtin_amdgcn_cvt_f32_fp8(wd, 3)};
#pragma unroll
        for (int j = 0; j < 4; j++)
            dt_traits<DT>::store(w, b * 32 + i * 4 + j, __uint_as_float(__float_as_uint(m[j] * s) | (((words[i] >> (8 * j)) & 0x80u) << 24)));
    }
}

// ---- decode form ------------------------------------------------------------------------------------------------------------------------
// Workgroup: columns 16 * blockIdx.x .. + 15 (reads past N clamped, never stored), rows 0 .. M - 1 (M <= 16 G).  Wave w takes the
// 128-k steps w, w + 4, ...; lane l holds column (row) l & 15, the scale of block l >> 4 of the step on either side, and of weights and
// x alike the bytes 16 (l >> 4) .. + 15 and 64 + 16 (l >> 4) .. + 15 of the step (a8_frag).  Blocks past K and rows past M enter as zero
// codes under scale 2^0 (code 127).  The weight fragment is the A operand, so a lane's accumulator holds 4 consecutive columns of one
// row of y.
template <int DT, int G>
__global__ __launch_bounds__(256) void mx8a8_decode_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                           const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    __shared__ mxa4_v4f red[3][G][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const int n0 = blockIdx.x * 16;
    const long nl = min(n0 + r16, N - 1);
    const uint8_t* wrow = qw + nl * K;
    const uint8_t* srow = sc + nl * KB;
    mxa4_v4f acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);  // loads are clamped and unconditional, then masked
        const bool kin = kb < KB;
        // this lane's halves: 16 bytes of block b0 = kq >> 1 of the step and 16 bytes of block b0 + 2, at offset 16 (kq & 1) in each
        const int kb0 = s * 4 + (kq >> 1), kb1 = kb0 + 2;
        const bool in0 = kb0 < KB, in1 = kb1 < KB;
        const int o0 = min(kb0, KB - 1) * 32 + (kq & 1) * 16, o1 = min(kb1, KB - 1) * 32 + (kq & 1) * 16;
        uint4_t w0 = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wrow + o0));
        uint4_t w1 = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wrow + o1));
        int sw = __builtin_nontemporal_load(srow + kc);
        uint4_t a0[G], a1[G];
        int sa[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const long m = min(g * 16 + r16, M - 1);
            a0[g] = *reinterpret_cast<const uint4_t*>(xq + m * K + o0);
            a1[g] = *reinterpret_cast<const uint4_t*>(xq + m * K + o1);
            sa[g] = xs[m * KB + kc];
        }
        if (!in0) w0 = uint4_t{0u, 0u, 0u, 0u};
        if (!in1) w1 = uint4_t{0u, 0u, 0u, 0u};
        if (!kin) sw = 127;
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool dead = g * 16 + r16 >= M;
            if (!in0 || dead) a0[g] = uint4_t{0u, 0u, 0u, 0u};
            if (!in1 || dead) a1[g] = uint4_t{0u, 0u, 0u, 0u};
            if (!kin || dead) sa[g] = 127;
        }
#pragma unroll
        for (int g = 0; g < G; g++)
            acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8_frag(w0, w1), a8_frag(a0[g], a1[g]), acc[g], 0, 0, 0, sw, 0, sa[g]);
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
// A workgroup per (64 WM) x (64 WN) tile (mx_scaled_gemm_tile at BK k per stage), the tiles walked in pipe_tile's order.
template <int DT, int WM, int WN, int BK>
__global__ __launch_bounds__(256) void mx8a8_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_scaled_gemm_tile<DT, WM, WN, mx_op_e4m3, mx_op_e4m3, mx_rows_dense, BK>(mx_rows_dense{tile_m * 64 * WM, M}, xq, xs, row_flag, qw, sc, ecol, bias, y, 0L, tile_n * 64 * WN, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The decode form serves M <= MX8_DECODE_ROWS (instances of 16, 32 and 64 rows); larger M takes the prefill form.  The plan's bound was
// measured (tools/mxfp8_a8_bench.py, profiles/mxfp8_a8_bench.jsonl, the "sweep" rows, both forms forced at M = 8 .. 64, the quantise
// launch included, fp16 and bf16 alike): the decode form was ahead at every M <= 48 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096
// (0.24 - 0.94 x the prefill form's time), and at M = 64 on two of the three shapes (24.7 / 48.0 us against 46.3 / 102.5); on
// 4096 -> 11008 it was 7 % behind there (51.2 against 47.8).  The bound stays at 64: what the prefill form would lose at M = 64 on the
// other two shapes (87 % and 114 %) outweighs that.
constexpr int MX8_DECODE_ROWS = 64;
constexpr int MX8_PLAN_ROWS = 64;

int mxfp8_quantize_launch(const void* w, uint8_t* qw, uint8_t* sc, long N, long K, int dtype, hipStream_t st) {
    const long nunits = N * (K >> 3);
    const dim3 grid((unsigned)cdivl(nunits, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx8_quantize_kernel<BIE_F16>, grid, dim3(256), 0, st, w, qw, sc, nunits);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx8_quantize_kernel<BIE_BF16>, grid, dim3(256), 0, st, w, qw, sc, nunits);
    else hipLaunchKernelGGL(mx8_quantize_kernel<BIE_F32>, grid, dim3(256), 0, st, w, qw, sc, nunits);
    return check_launch("mx8_quantize_kernel");
}

int mxfp8_dequant_launch(const uint8_t* qw, const uint8_t* sc, void* w, long N, long K, int dtype, hipStream_t st) {
    const long nblk = N * (K >> 5);
    const dim3 grid((unsigned)cdivl(nblk, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx8_dequant_kernel<BIE_F16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx8_dequant_kernel<BIE_BF16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else hipLaunchKernelGGL(mx8_dequant_kernel<BIE_F32>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    return check_launch("mx8_dequant_kernel");
}

// The large tile (taken under the shared rule of mx_scaled_launch.cuh: where it gives every CU of the card at least two workgroups) is
// 128 x 128 at 64 k per stage, the small one 64 x 64 at 128 k per stage.  The large one was measured at M = 4096 against 128 x 64 at
// 128 k per stage and against 64 x 64 tiles everywhere (the "tile" rows of profiles/mxfp8_a8_bench.jsonl, fp16, us): 243.6 / 252.8 /
// 251.3 on 4096 x 4096 and 562.4 / 726.5 / 686.3 on 4096 -> 11008, but 673.8 / 629.8 / 716.1 on 11008 -> 4096, where 128 x 64 with the
// longer stage is 7 % ahead: the tile that wins on two shapes of three ships and the 128 x 64 instance is not kept; a per-call choice
// was not tried.  A 128 x 128 tile at 128 k per stage in a dynamic allocation of 75776 bytes was not built: nothing in this library
// launches more than 65536 bytes of LDS.
// The workspace is bie_mxfp4_a8_linear_forward's: xq [M, K] (16-byte aligned), xs [M, K/32], row_flag [M]
struct mx8a8_layer {
    using act = mx_act_e4m3;  // the W4A8 layer's quantiser and workspace layout
    static constexpr const char* form_knob = "BIE_MXFP8_A8_FORM";
    static constexpr int decode_rows = MX8_DECODE_ROWS, plan_rows = MX8_PLAN_ROWS;
    static constexpr const char* decode_name = "mx8a8_decode_kernel";
    static constexpr const char* gemm_name = "mx8a8_gemm_kernel";
    template <int DT, int G> static constexpr auto decode() { return mx8a8_decode_kernel<DT, G>; }
    template <int DT, int W> static constexpr auto gemm() { return mx8a8_gemm_kernel<DT, W, W, W == 2 ? 64 : 128>; }
};

bool mxfp8_a8_decode_ok(long M) { return mx_dense_decode_ok<mx8a8_layer>(M); }
int mxfp8_a8_form(long M, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_dense_form<mx8a8_layer>(M); }

int mxfp8_a8_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_gemm_launch<mx8a8_layer>(xq, xs, row_flag, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

int mxfp8_a8_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    return mx_dense_forward_launch<mx8a8_layer>(x, qw, sc, ecol, bias, y, workspace, M, N, K, dtype, form, st);
}

}  // namespace bie
