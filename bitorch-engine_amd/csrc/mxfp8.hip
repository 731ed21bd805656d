// MXFP8 (OCP microscaling FP8, E4M3 elements) weight-only linear layer for gfx950: y = x . W^T (+ bias), x fp16 / bf16 (W8A16).  No
// reference implementation exists; the format is MXFP8A8LinearCuda's (mxfp8_a8.hip, whose quantiser and dequant serve this layer too) and
// the arithmetic MXFP6LinearCuda's (include/bie_hip.h, INTEGRATION.md "MXFP8 linear layer"):
//
//   qweight uint8 [N, K]: one e4m3fn byte per weight, row-major: per row K/32 blocks of 32 bytes
//   scales  uint8 [N, K/32]: E8M0, code s = 2^(s - 127) for s in 0..254, 255 = NaN
//   W[n, k] = e4m3(qweight[n, k]) * 2^(s - 127)   (exact in fp32; a NaN code 0x7f / 0xff is NaN)
//   y[m, n] = dt( sum_k x[m, k] * W[n, k] + bias[n] ), products exact, the sum in fp32, one rounding to the dtype
//
// Decode form (mx8_decode_kernel, M <= MX8W_DECODE_ROWS): one launch.  The unit of work is HALF a block: MX8_UNIT = 16 bytes, one
// non-temporal 16-byte load.  Its four dwords become eight pairs of exact 16-bit values with eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at
// scale 1.0 (two per dword, op_sel picking the half), v_dot2_f32_{bf16,f16} sums the 16 products of a row into an fp32 partial, and the
// partial is multiplied by the block's fp32 scale (a power of two: exact; the two lanes of a block load the same scale byte).  No 16-bit
// image of W exists, so the fp16 form has the fp32 range of W.
//   Why the half block: with one unit per lane the 64 lanes of a wave read 1024 CONTIGUOUS bytes of a weight row per load instruction
//   (eight whole 128-byte lines).  With a whole block per lane (two loads 16 bytes apart) each of the two instructions touches every
//   other 16 bytes of 2048, and a lane holds 16 converted VGPRs per column where the half block holds 8: the compiled loops are 137
//   VGPRs (3 waves per SIMD) against 176 (2) at R = 16, 107 against 132 at R = 32 (profiles/mxfp8_resources.txt).  The kernel is written
//   over MX8_UNIT, so the whole-block map is this file at MX8_UNIT = 32; both were measured in one call (the plan comment below).  One
//   unit has to serve every instance, since a row's bits must not depend on the instance.
//   The thread-to-unit map: a row of W has K / 16 units (256 at K = 4096, 180 at K = 2880), so the workgroup is split over its columns
//   as MXFP6's is: 256 / G groups of G threads (G = 128, 64 or 32 by mx6_decode_group's rule on the unit count: 128 at K = 4096, two
//   passes; 64 at K = 2880, where 3 passes of 64 cover the 180 units), each group striding the units of its own CT columns, which share
//   the x registers.  A thread holds one converted unit per column (8 VGPRs each) across the R rows: the converts, 8 VALU instructions
//   per unit and column, are done once per unit whatever R is.  CT is 4, and 2 for the 32-row instance (its accumulators are CT * 32).
//   The K-split partials are summed on the DPP network per half-wave (mx6_half_sum_f32), then across the group's half-waves in LDS in a
//   fixed order: the unit-to-lane map and G depend on K alone, so a row's bits do not depend on M, on the instance or on the row's position.
//   Loads are clamped and unconditional, then masked (the rule at the top of mx_scaled_decode.cuh): a column past N reads column N - 1 and
//   is never stored; the unit loop runs over the units that exist.
// Prefill form (mx8_gemm_kernel): mx8_gemm_tile of mxfp8_common.cuh, a 128 x 128 tile GEMM on v_mfma_f32_32x32x16_{bf16,f16} with
// double-buffered LDS.  The weight tile is staged PACKED (64 bytes per row and 64-k stage in a swizzled, unpadded layout, plus two scale
// words) and converted after the LDS read, 16 converts per 32 weights.  Each column is rebiased by its largest scale code e_col[n]
// (bie_mxfp4_col_exp): fragments hold e4m3 * 2^(s - e_col[n]) <= 448 and the fp32 epilogue multiplies by 2^(e_col[n] - 127); e_col = 255
// makes the column NaN.
#include "mxfp8_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- decode form --------------------------------------------------------------------------------------------------------------------
// Workgroup: columns C * blockIdx.x .. + C - 1, C = CT * 256 / G (clamped reads past N, never stored), rows 0 .. M - 1 (M <= R).  Group
// g = t / G holds columns g CT .. + CT - 1 of those; its thread j = t % G takes the units j, j + G, ... of K.
template <int DT, int R, int CT, int G>
__global__ __launch_bounds__(256) void mx8_decode_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    typedef mx_pair<DT> P;
    typedef mx8_w16<DT> Cv;
    constexpr int C = CT * (256 / G), HPG = G / 32;  // columns per workgroup, half-waves per group
    constexpr int L = MX8_UNIT / 16;                 // 16-byte loads per unit
    __shared__ float red[8][CT][R];
    const int t = threadIdx.x, g = t / G, j = t % G;
    const int KB = K >> 5, U = K / MX8_UNIT;
    const int n0 = blockIdx.x * C + g * CT;
    const uint8_t* wrow[CT];
    const uint8_t* srow[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const long n = min(n0 + c, N - 1);
        wrow[c] = qw + n * (long)K;
        srow[c] = sc + n * KB;
    }
    float acc[CT][R];
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[c][r] = 0.0f;
    for (int u = j; u < U; u += G) {
        uint4_t wb[CT][L];
        uint32_t sb[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint4_t* p = reinterpret_cast<const uint4_t*>(wrow[c] + (long)u * MX8_UNIT);
#pragma unroll
            for (int i = 0; i < L; i++) wb[c][i] = __builtin_nontemporal_load(p + i);
            sb[c] = __builtin_nontemporal_load(srow[c] + (u * MX8_UNIT >> 5));
        }
        typename P::t wv[CT][8 * L];  // pair i: weights 2 i, 2 i + 1 of the unit
        float s[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
#pragma unroll
            for (int i = 0; i < L; i++) {
                const uint32_t d[4] = {wb[c][i].x, wb[c][i].y, wb[c][i].z, wb[c][i].w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    wv[c][8 * i + 2 * q] = Cv::template cvt<false>(d[q], 1.0f);
                    wv[c][8 * i + 2 * q + 1] = Cv::template cvt<true>(d[q], 1.0f);
                }
            }
            s[c] = e8m0_f32(sb[c]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {  // M is uniform
                const uint4_t* xp = reinterpret_cast<const uint4_t*>(x + (long)r * K + (long)u * MX8_UNIT);
                uint32_t xv[8 * L];
#pragma unroll
                for (int i = 0; i < 2 * L; i++) {
                    const uint4_t xq = xp[i];
                    xv[4 * i] = xq.x; xv[4 * i + 1] = xq.y; xv[4 * i + 2] = xq.z; xv[4 * i + 3] = xq.w;
                }
#pragma unroll
                for (int c = 0; c < CT; c++) {
                    float p = 0.0f;
#pragma unroll
                    for (int i = 0; i < 8 * L; i++) p = P::dot(wv[c][i], xv[i], p);
                    acc[c][r] += p * s[c];
                }
            }
        }
    }
    const int lane = t & 63;
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {
                const float v = mx6_half_sum_f32(acc[c][r]);
                if ((lane & 31) == 31) red[t >> 5][c][r] = v;
            }
        }
    __syncthreads();
    for (int o = t; o < C * R; o += 256) {
        const int cc = o / R, r = o % R, n = blockIdx.x * C + cc;
        if (n < N && r < M) {
            const int h0 = (cc / CT) * HPG, c = cc % CT;
            float v = red[h0][c][r];
#pragma unroll
            for (int h = 1; h < HPG; h++) v += red[h0 + h][c][r];
            if (bias) v += dt_traits<DT>::load(bias, n);
            dt_traits<DT>::store(y, (long)r * N + n, v);
        }
    }
}

// ---- prefill form -------------------------------------------------------------------------------------------------------------------
// A workgroup per 128 x 128 tile (mx8_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx8_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                       const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int M, int N,
                                                       int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx8_gemm_tile<DT>(mx_rows_dense{tile_m * MX_BM, M}, x, qw, sc, ecol, bias, y, 0L, tile_n * MX_BN, N, K);
}

// ---- plan and launchers -----------------------------------------------------------------------------------------------------------------
// The decode form exists for M <= MX8W_DECODE_ROWS (instances R = 1, 2, 4, 8, 16, 32 rows); larger M takes the MFMA GEMM.  The plan
// takes the decode form for M <= MX8W_PLAN_ROWS.  The bound was measured (tools/mxfp8_bench.py, profiles/mxfp8_bench.jsonl, the sweep
// rows: M = 1 .. 32, 40, 48, 56, 64 on both forms, medians of 7 graph replays over rotating weight sets; slowest - fastest replay
// under 8 % of the median on the sweep rows): the decode form was ahead at EVERY M <= 32 on 4096 x 4096, 4096 -> 11008, 11008 -> 4096
// and 2880 -> 5760, fp16 and bf16 alike (bf16 within 2.4 % of every figure), the GEMM having only ceil(N / 128) workgroups at such M and
// a time that does not depend on M below 128.  fp16, decode / prefill us:
//     M      4096 x 4096    4096 -> 11008   11008 -> 4096    2880 -> 5760
//     1     7.6 /  85.5    12.6 /  97.3    18.4 / 255.4     6.6 /  66.2
//     2     6.7 /  85.7    12.9 /  97.5    14.9 / 255.3     8.2 /  66.3
//     4     8.2 /  85.8    16.9 /  97.3    18.2 / 255.1    10.1 /  66.3
//     8    11.1 /  85.6    22.3 /  97.4    24.4 / 255.1    13.7 /  66.3
//    16    16.3 /  86.1    36.5 /  97.4    36.3 / 255.5    20.1 /  66.8
//    17    17.6 /  86.2    43.9 /  97.5    42.2 / 256.2    19.8 /  66.9    (the 32-row instance: CT = 2)
//    24    22.0 /  86.2    54.4 /  97.7    53.6 / 256.2    25.1 /  66.9
//    32    26.7 /  86.2    66.7 /  97.9    65.7 / 256.8    30.5 /  67.1
//    64       - /  86.9       - /  99.0       - / 257.8       - /  67.9
// At M = 32 the decode form is still 1.5 - 3.9 x ahead, growing by 0.6 - 1.6 us per row, so a 64-row instance might pay on three of
// the four shapes (on 4096 -> 11008 the extrapolation crosses near M = 52); with twice the accumulators it was NOT built or measured,
// and the bound stays at the largest instance that was.  Every instance up to 32 rows is used by the plan.  The one-row instance is
// slower than the two-row one at M = 2 on 4096 x 4096 and 11008 -> 4096 (7.6 against 6.7, 18.4 against 14.9): not explained; issuing
// the x and scale loads ahead of the converts did not change it and cost 5 - 10 % at 32 rows, so the loop is left to the compiler.
// The unit (the "unit" rows, fp16, decode us, half block / whole block, the half block measured before and after in the same call):
//     M      4096 x 4096    4096 -> 11008   11008 -> 4096    2880 -> 5760
//     1     7.6 /   5.7    12.5 /  12.2    18.7 /  13.6     6.6 /   8.1
//     4     8.2 /   7.9    16.7 /  16.4    18.4 /  17.6    10.1 /  10.8
//    16    16.1 /  15.8    36.7 /  42.0    36.3 /  35.3    19.8 /  22.0
//    17    17.3 /  28.7    44.0 /  64.0    42.4 /  73.2    19.4 /  30.1
//    32    26.7 /  47.0    66.7 / 105.9    65.9 / 119.2    30.3 /  49.7
// The whole block is ahead at M = 1 where K / 32 fills its 128-thread groups in one pass (by 25 % and 27 %) and 1.5 - 1.8 x behind from
// 17 rows on every shape, behind at every M on 2880 -> 5760: the half block ships, and the M = 1 figure on K = 4096 / 11008 is what it costs.
constexpr int MX8W_DECODE_ROWS = 32;
constexpr int MX8W_PLAN_ROWS = 32;

template <int DT, int R>
static void mx8_decode_launch_r(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
    mx6_decode_group(K / MX8_UNIT, [&](auto g) {
        constexpr int G = decltype(g)::value, CT = R >= 32 ? 2 : 4, C = CT * (256 / G);
        hipLaunchKernelGGL((mx8_decode_kernel<DT, R, CT, G>), dim3((unsigned)cdiv(N, C)), dim3(256), 0, st, x, qw, sc, bias, y, M, N, K);
    });
}

// the layer, for the host path of mx_w16_launch.cuh
struct mx8_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP8_FORM";
    static constexpr int decode_rows = MX8W_DECODE_ROWS, plan_rows = MX8W_PLAN_ROWS;
    static constexpr const char *decode_name = "mx8_decode_kernel", *gemm_name = "mx8_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
        if (M <= 1) mx8_decode_launch_r<DT, 1>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 2) mx8_decode_launch_r<DT, 2>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 4) mx8_decode_launch_r<DT, 4>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 8) mx8_decode_launch_r<DT, 8>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 16) mx8_decode_launch_r<DT, 16>(x, qw, sc, bias, y, M, N, K, st);
        else mx8_decode_launch_r<DT, 32>(x, qw, sc, bias, y, M, N, K, st);
    }
    template <int DT> static constexpr auto gemm() { return mx8_gemm_kernel<DT>; }
};

int mxfp8_form(long M, long, long, int) { return mx_w16_form<mx8_w16_layer>(M); }
bool mxfp8_decode_ok(long M) { return mx_w16_decode_ok<mx8_w16_layer>(M); }
int mxfp8_decode_rows() { return MX8W_DECODE_ROWS; }
int mxfp8_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, long M, long N, long K,
                         int dtype, int form, hipStream_t st) {
    return mx_w16_forward_launch<mx8_w16_layer>(x, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

}  // namespace bie
