// MXFP4 (OCP microscaling FP4) weight-only linear layer for gfx950: y = x . W^T (+ bias), x fp16 / bf16.  No reference implementation
// exists; the format and the arithmetic are this library's own (include/bie_hip.h, INTEGRATION.md "MXFP4 linear layer").
//
//   qweight uint8 [N, K/2]: element 2j in the low nibble of byte j, 2j + 1 in the high nibble (the `blocks` of gpt-oss-style checkpoints)
//   scales  uint8 [N, K/32]: E8M0, code s = 2^(s - 127) for s in 0..254, 255 = NaN
//   W[n, k] = e2m1(code) * 2^(s - 127), e2m1 = sign bit 3, magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}[code & 7]   (exact in fp32)
//   y[m, n] = dt( sum_k x[m, k] * W[n, k] + bias[n] ), products exact, the sum in fp32, one rounding to the dtype
//
// Decode form (mx_decode_kernel, M <= 16): one launch, a workgroup per C output columns, its 256 threads striding K by 16 values
// (8 bytes of codes and the half-block's scale byte per column, non-temporal loads).  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns two codes
// into two exact 16-bit values (scale 1.0), v_dot2_f32_{bf16,f16} sums 16 products per row into fp32, and that partial is multiplied by
// the block's fp32 scale (a power of two: exact).  No 16-bit image of W exists, so the fp16 form has the fp32 range of W.  The K-split
// partials are summed on the DPP network, then across the 4 waves in LDS.
// Prefill form (mx_gemm_kernel): mx_gemm_tile of mxfp4_common.cuh, a 128 x 128 tile GEMM on v_mfma_f32_32x32x16_{bf16,f16} with
// double-buffered LDS, on the rows m0 .. of x.  The weight tile is staged PACKED (32 bytes per row and 64-k stage, plus two scale
// words) and converted to B fragments after the LDS read.  Each column is rebiased by its largest scale code e_col[n]
// (bie_mxfp4_col_exp, computed once at load time): fragments hold e2m1 * 2^(s - e_col[n]) <= 6 and the fp32 epilogue multiplies by
// 2^(e_col[n] - 127).  A column with a scale-255 block has e_col = 255, which makes the whole column NaN in the epilogue.
#include "mxfp4_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

__device__ __forceinline__ float mx_e2m1(uint32_t c) {  // the code's value as fp32 bits: 0, 0.5, then (1 + m / 2) * 2^(e - 1)
    const uint32_t i = c & 7u;
    const uint32_t mag = i < 2u ? (i ? 0x3f000000u : 0u) : ((126u + (i >> 1)) << 23) | ((i & 1u) << 22);
    return __uint_as_float(mag | ((c & 8u) << 28));
}

// ---- quantise / dequant / column exponent ---------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ float mx_load(const void* p, long i) { return dt_traits<DT>::load(p, i); }

// One thread per 32-value block: amax, the block's scale 2^e (mx_block_scale), codes of w * 2^-e.  An all-zero block: scale 0, codes 0.
template <int DT>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const void* __restrict__ w, uint8_t* __restrict__ qw, uint8_t* __restrict__ sc, long nblk) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    float v[32];
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        v[i] = mx_load<DT>(w, b * 32 + i);
        amax = fmaxf(amax, fabsf(v[i]));
    }
    uint4_t codes = {0u, 0u, 0u, 0u};
    uint32_t scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mx_block_scale(amax, inv);
#pragma unroll
        for (int i = 0; i < 32; i++) {
            const uint32_t c = mx_round_e2m1(fabsf(v[i] * inv)) | ((__float_as_uint(v[i]) >> 28) & 8u);
            codes[i >> 3] |= c << (4 * (i & 7));
        }
    }
    reinterpret_cast<uint4_t*>(qw)[b] = codes;
    sc[b] = (uint8_t)scode;
}

// One thread per 32-value block: W in fp32 (exact), rounded once to the output dtype
template <int DT>
__global__ __launch_bounds__(256) void mx_dequant_kernel(const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, void* __restrict__ w, long nblk) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const uint4_t codes = reinterpret_cast<const uint4_t*>(qw)[b];
    const float s = e8m0_f32(sc[b]);
#pragma unroll
    for (int i = 0; i < 32; i++) dt_traits<DT>::store(w, b * 32 + i, mx_e2m1(codes[i >> 3] >> (4 * (i & 7))) * s);
}

// e_col[n] = 255 if row n has a scale-255 block, else the largest scale code of the row.  One wave per row: the lanes read the row's
// scale bytes side by side, the maximum is taken across the wave.
__global__ __launch_bounds__(256) void mx_col_exp_kernel(const uint8_t* __restrict__ sc, uint8_t* __restrict__ ecol, int N, int KB) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;  // wave-uniform
    uint32_t e = 0u;
    for (int i = lane; i < KB; i += 64) e = max(e, (uint32_t)sc[(long)n * KB + i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) e = max(e, (uint32_t)__shfl_xor((int)e, o, 64));
    if (lane == 0) ecol[n] = (uint8_t)e;
}

// ---- decode form --------------------------------------------------------------------------------------------------------------------
// Workgroup: columns C * blockIdx.x .. + C - 1 (clamped reads past N, never stored), rows 0 .. M - 1 (M <= R).  Thread t takes the
// 16-value units u = t, t + 256, ... of K: per column 8 code bytes and the scale byte of block u / 2.
template <int DT, int R, int C>
__global__ __launch_bounds__(256) void mx_decode_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                        const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    typedef mx_pair<DT> P;
    __shared__ float red[4][C][R];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int U = K >> 4, KB = K >> 5;
    const int n0 = blockIdx.x * C;
    const uint8_t* wrow[C];
    const uint8_t* srow[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const long n = min(n0 + c, N - 1);
        wrow[c] = qw + n * (K >> 1);
        srow[c] = sc + n * KB;
    }
    float acc[C][R];
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
        for (int r = 0; r < R; r++) acc[c][r] = 0.0f;
    for (int u = threadIdx.x; u < U; u += 256) {
        uint2_t wb[C];
        uint32_t sb[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
            wb[c] = __builtin_nontemporal_load(reinterpret_cast<const uint2_t*>(wrow[c]) + u);
            sb[c] = __builtin_nontemporal_load(srow[c] + (u >> 1));
        }
        typename P::t wv[C][8];
#pragma unroll
        for (int c = 0; c < C; c++) mx_unpack16<DT>(wb[c], wv[c]);
        float s[C];
#pragma unroll
        for (int c = 0; c < C; c++) s[c] = e8m0_f32(sb[c]);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {  // M is uniform
                const uint4_t* xp = reinterpret_cast<const uint4_t*>(x + (long)r * K) + 2 * u;
                const uint4_t x0 = xp[0], x1 = xp[1];
                const uint32_t xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int c = 0; c < C; c++) {
                    float p = 0.0f;
#pragma unroll
                    for (int j = 0; j < 8; j++) p = P::dot(wv[c][j], xv[j], p);
                    acc[c][r] += p * s[c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {
                const float v = wave_sum_f32(acc[c][r]);
                if (lane == 0) red[wave][c][r] = v;
            }
        }
    __syncthreads();
    if (threadIdx.x < C * R) {
        const int c = threadIdx.x / R, r = threadIdx.x % R, n = n0 + c;
        if (n < N && r < M) {
            float v = ((red[0][c][r] + red[1][c][r]) + red[2][c][r]) + red[3][c][r];
            if (bias) v += dt_traits<DT>::load(bias, n);
            dt_traits<DT>::store(y, (long)r * N + n, v);
        }
    }
}

// ---- prefill form -------------------------------------------------------------------------------------------------------------------
// A workgroup per 128 x 128 tile (mx_gemm_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx_gemm_kernel(const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                      const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int M, int N,
                                                      int K, int tiles_n) {
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    mx_gemm_tile<DT>(mx_rows_dense{tile_m * MX_BM, M}, x, qw, sc, ecol, bias, y, 0L, tile_n * MX_BN, N, K);
}

// ---- plan and launchers -----------------------------------------------------------------------------------------------------------------
// The decode form serves M <= MX_DECODE_ROWS (instances R = 1, 2, 4, 8, 16 rows); larger M takes the MFMA GEMM.  The bound of the plan
// was measured (tools/mxfp4_bench.py, profiles/mxfp4_bench.jsonl, the M sweep): the decode form was ahead at every M <= 16 on
// 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 in fp16 and bf16 (at M = 16: 20.1 / 52.6 / 36.7 us against 84.9 / 91.6 / 241.0), the
// GEMM having only ceil(N / 128) workgroups at such M.
constexpr int MX_DECODE_ROWS = 16;
constexpr int MX_PLAN_ROWS = 16;

int mxfp4_quantize_launch(const void* w, uint8_t* qw, uint8_t* sc, long N, long K, int dtype, hipStream_t st) {
    const long nblk = N * (K / 32);
    const dim3 grid((unsigned)cdivl(nblk, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx_quantize_kernel<BIE_F16>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx_quantize_kernel<BIE_BF16>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    else hipLaunchKernelGGL(mx_quantize_kernel<BIE_F32>, grid, dim3(256), 0, st, w, qw, sc, nblk);
    return check_launch("mx_quantize_kernel");
}

int mxfp4_dequant_launch(const uint8_t* qw, const uint8_t* sc, void* w, long N, long K, int dtype, hipStream_t st) {
    const long nblk = N * (K / 32);
    const dim3 grid((unsigned)cdivl(nblk, 256));
    if (dtype == BIE_F16) hipLaunchKernelGGL(mx_dequant_kernel<BIE_F16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(mx_dequant_kernel<BIE_BF16>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    else hipLaunchKernelGGL(mx_dequant_kernel<BIE_F32>, grid, dim3(256), 0, st, qw, sc, w, nblk);
    return check_launch("mx_dequant_kernel");
}

int mxfp4_col_exp_launch(const uint8_t* sc, uint8_t* ecol, long N, long K, hipStream_t st) {
    hipLaunchKernelGGL(mx_col_exp_kernel, dim3((unsigned)cdivl(N, 4)), dim3(256), 0, st, sc, ecol, (int)N, (int)(K / 32));
    return check_launch("mx_col_exp_kernel");
}

template <int DT, int R>
static void mx_decode_launch_r(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
    constexpr int C = R >= 4 ? 8 : 4;  // columns per workgroup: x is read once per C columns
    hipLaunchKernelGGL((mx_decode_kernel<DT, R, C>), dim3((unsigned)cdiv(N, C)), dim3(256), 0, st, x, qw, sc, bias, y, M, N, K);
}

// the layer, for the host path of mx_w16_launch.cuh
struct mx4_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP4_FORM";
    static constexpr int decode_rows = MX_DECODE_ROWS, plan_rows = MX_PLAN_ROWS;
    static constexpr const char *decode_name = "mx_decode_kernel", *gemm_name = "mx_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int M, int N, int K, hipStream_t st) {
        if (M <= 1) mx_decode_launch_r<DT, 1>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 2) mx_decode_launch_r<DT, 2>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 4) mx_decode_launch_r<DT, 4>(x, qw, sc, bias, y, M, N, K, st);
        else if (M <= 8) mx_decode_launch_r<DT, 8>(x, qw, sc, bias, y, M, N, K, st);
        else mx_decode_launch_r<DT, 16>(x, qw, sc, bias, y, M, N, K, st);
    }
    template <int DT> static constexpr auto gemm() { return mx_gemm_kernel<DT>; }
};

int mxfp4_form(long M, long, long, int) { return mx_w16_form<mx4_w16_layer>(M); }
bool mxfp4_decode_ok(long M) { return mx_w16_decode_ok<mx4_w16_layer>(M); }
int mxfp4_decode_rows() { return MX_DECODE_ROWS; }
int mxfp4_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, long M, long N, long K,
                         int dtype, int form, hipStream_t st) {
    return mx_w16_forward_launch<mx4_w16_layer>(x, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

}  // namespace bie
