// MXFP6 (OCP microscaling FP6, E2M3 elements) weight-only linear layer for gfx950: y = x . W^T (+ bias), x fp16 / bf16 (W6A16).  No
// reference implementation exists; the format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP6
// linear layer"), the contract MXFP4LinearCuda's with E2M3 elements:
//
//   qweight uint8 [N, 3K/4]: the mxfp6 w6a8 layout, per row K/32 blocks of 24 bytes, code j of a block in bits 6 j .. 6 j + 5
//   scales  uint8 [N, K/32]: E8M0, code s = 2^(s - 127) for s in 0..254, 255 = NaN
//   W[n, k] = e2m3(code) * 2^(s - 127)   (exact in fp32)
//   y[m, n] = dt( sum_k x[m, k] * W[n, k] + bias[n] ), products exact, the sum in fp32, one rounding to the dtype
//
// Decode form (mx6_decode_kernel, M <= MX6_DECODE_ROWS): one launch.  The unit of work is a whole block: its 24 bytes (three 8-byte
// non-temporal loads: a block is only 8-byte aligned) become 32 exact 16-bit values with ONE v_cvt_scalef32_pk32_{bf16,f16}_fp6 at scale
// 1.0, v_dot2_f32_{bf16,f16} sums the 32 products of a row into an fp32 partial, and the partial is multiplied by the block's fp32 scale
// (a power of two: exact).  No 16-bit image of W exists, so the fp16 form has the fp32 range of W.
//   The thread-to-unit map: a row of W has only K / 32 blocks (128 at K = 4096, 90 at K = 2880), fewer than the 256 threads, so the
//   workgroup is SPLIT OVER ITS COLUMNS: 256 / G groups of G threads (G = 128, 64 or 32, chosen on the host from K / 32 so that the
//   padded last pass wastes at most an eighth: 128 at K = 4096, 32 at K = 2880, where 3 passes of 32 cover the 90 blocks), each group
//   striding the blocks of its own CT columns, which share the x registers.  A thread holds one converted block per column: 16 VGPRs
//   each, so CT is 4 (2 for G = 32, which already has 8 groups, and for the 32-row instance, whose accumulators are CT * 32).
//   The K-split partials are summed on the DPP network per half-wave (mx6_half_sum_f32), then across the group's half-waves in LDS.
// Prefill form (mx6_gemm_kernel): mx6_gemm_tile of mxfp6_common.cuh, a 128 x 128 tile GEMM on v_mfma_f32_32x32x16_{bf16,f16} with
// double-buffered LDS.  The weight tile is staged PACKED (48 bytes per row and 64-k stage, plus two scale words) and converted after
// the LDS read, one pk32 convert per 32 weights.  Each column is rebiased by its largest scale code e_col[n] (bie_mxfp4_col_exp):
// fragments hold e2m3 * 2^(s - e_col[n]) <= 7.5 and the fp32 epilogue multiplies by 2^(e_col[n] - 127); e_col = 255 makes the column NaN.
#include "mxfp6_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- decode form --------------------------------------------------------------------------------------------------------------------
// Workgroup: columns C * blockIdx.x .. + C - 1, C = CT * 256 / G (clamped reads past N, never stored), rows 0 .. M - 1 (M <= R).  Group
// g = t / G holds columns g CT .. + CT - 1 of those; its thread j = t % G takes the blocks j, j + G, ... of K.
template <int DT, int R, int CT, int G>
__global__ __launch_bounds__(256) void mx6_decode_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    typedef mx_pair<DT> P;
    typedef mx6_w16<DT> Cv;
    constexpr int C = CT * (256 / G), HPG = G / 32;  // columns per workgroup, half-waves per group
    __shared__ float red[8][CT][R];
    const int t = threadIdx.x, g = t / G, j = t % G;
    const int KB = K >> 5;
    const int n0 = blockIdx.x * C + g * CT;
    const uint8_t* wrow[CT];
    const uint8_t* srow[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const long n = min(n0 + c, N - 1);
        wrow[c] = qw + n * ((long)KB * MX6_BLOCK_BYTES);
        srow[c] = sc + n * KB;
    }
    float acc[CT][R];
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[c][r] = 0.0f;
    for (int kb = j; kb < KB; kb += G) {
        uint2_t wb[CT][3];
        uint32_t sb[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint2_t* p = reinterpret_cast<const uint2_t*>(wrow[c] + (long)kb * MX6_BLOCK_BYTES);
#pragma unroll
            for (int i = 0; i < 3; i++) wb[c][i] = __builtin_nontemporal_load(p + i);
            sb[c] = __builtin_nontemporal_load(srow[c] + kb);
        }
        typename Cv::t wv[CT];
        float s[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            wv[c] = Cv::cvt(mx6_v6u{wb[c][0].x, wb[c][0].y, wb[c][1].x, wb[c][1].y, wb[c][2].x, wb[c][2].y}, 1.0f);
            s[c] = e8m0_f32(sb[c]);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {  // M is uniform
                const uint4_t* xp = reinterpret_cast<const uint4_t*>(x + (long)r * K) + 4 * kb;
                const uint4_t x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
                const uint32_t xv[16] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
#pragma unroll
                for (int c = 0; c < CT; c++) {
                    float p = 0.0f;
#pragma unroll
                    for (int i = 0; i < 16; i++) p = P::dot(Cv::pair(wv[c], i), xv[i], p);
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
// A workgroup per 128 x 128 tile (mx6_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx6_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                       const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int M, int N,
                                                       int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx6_gemm_tile<DT>(mx_rows_dense{tile_m * MX_BM, M}, x, qw, sc, ecol, bias, y, 0L, tile_n * MX_BN, N, K);
}

// ---- plan and launchers -----------------------------------------------------------------------------------------------------------------
// The decode form exists for M <= MX6_DECODE_ROWS (instances R = 1, 2, 4, 8, 16, 32 rows); larger M takes the MFMA GEMM.  The plan
// takes the decode form for M <= MX6_PLAN_ROWS.  The bound was measured (tools/mxfp6_bench.py, profiles/mxfp6_bench.jsonl, the sweep
// rows: M = 1 .. 32 on both forms, medians of 7 graph replays; slowest - fastest replay up to 12 % at M = 1, under 6 % elsewhere): the decode form was ahead at EVERY M <= 32 on
// 4096 x 4096, 4096 -> 11008, 11008 -> 4096 and 2880 -> 5760, fp16 and bf16 alike, the GEMM having only ceil(N / 128) workgroups at such
// M and a time that does not depend on M below 128.  fp16, decode / prefill us:
//     M      4096 x 4096    4096 -> 11008   11008 -> 4096    2880 -> 5760
//     1      5.3 / 103.4    10.5 / 109.0    12.2 / 277.5     6.2 / 73.4
//     8      9.9 / 103.2    22.4 / 108.9    20.6 / 276.9    16.4 / 73.4
//    16     15.8 / 103.5    41.0 / 109.3    32.6 / 277.2    27.1 / 73.7
//    17     28.3 / 103.9    62.6 / 109.6    68.1 / 277.8    29.4 / 74.0    (the 32-row instance: CT = 2)
//    24     36.8 / 103.7    82.3 / 109.6    89.7 / 278.0    38.4 / 74.1
//    32     46.6 / 103.9   103.9 / 109.8   114.6 / 278.5    48.9 / 74.0
// At M = 32 the margin on 4096 -> 11008 is down to 5 % and the decode time grows by 2.8 us per row there, so a 64-row instance (twice
// the accumulators) would already be behind at M = 35: the bound is 32, not MXFP4's 16, and no instance beyond 32 rows is built.
constexpr int MX6_DECODE_ROWS = 32;
constexpr int MX6_PLAN_ROWS = 32;

template <int DT, int R>
static void mx6_decode_launch_r(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
    mx6_decode_group(K >> 5, [&](auto g) {
        constexpr int G = decltype(g)::value, CT = (G == 32 || R >= 32) ? 2 : 4, C = CT * (256 / G);
        hipLaunchKernelGGL((mx6_decode_kernel<DT, R, CT, G>), dim3((unsigned)cdiv(N, C)), dim3(256), 0, st, x, qw, sc, bias, y, M, N, K);
    });
}

// the layer, for the host path of mx_w16_launch.cuh
struct mx6_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP6_FORM";
    static constexpr int decode_rows = MX6_DECODE_ROWS, plan_rows = MX6_PLAN_ROWS;
    static constexpr const char *decode_name = "mx6_decode_kernel", *gemm_name = "mx6_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
        if (M <= 1) mx6_decode_launch_r<DT, 1>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 2) mx6_decode_launch_r<DT, 2>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 4) mx6_decode_launch_r<DT, 4>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 8) mx6_decode_launch_r<DT, 8>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 16) mx6_decode_launch_r<DT, 16>(x, qw, sc, bias, y, M, N, K, st);
        else mx6_decode_launch_r<DT, 32>(x, qw, sc, bias, y, M, N, K, st);
    }
    template <int DT> static constexpr auto gemm() { return mx6_gemm_kernel<DT>; }
};

int mxfp6_form(long M, long, long, int) { return mx_w16_form<mx6_w16_layer>(M); }
bool mxfp6_decode_ok(long M) { return mx_w16_decode_ok<mx6_w16_layer>(M); }
int mxfp6_decode_rows() { return MX6_DECODE_ROWS; }
int mxfp6_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, long M, long N, long K,
                         int dtype, int form, hipStream_t st) {
    return mx_w16_forward_launch<mx6_w16_layer>(x, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

}  // namespace bie
