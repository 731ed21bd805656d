// MXFP8 weight-only (W8A16) mixture-of-experts expert GEMM for gfx950: the weights of mxfp8.hip stacked per expert, every (token, slot)
// pair contracted with the expert its index names (include/bie_hip.h, INTEGRATION.md "MXFP8 W8A16 mixture-of-experts layer").  It is
// mxfp6_moe.hip with the weight side of mxfp8.hip.  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]
//   qweight uint8 [E, N, K] (one e4m3fn byte per weight), scales uint8 [E, N, K/32] (E8M0), e_col uint8 [E, N], bias [E, N] or NULL:
//   mxfp8.hip's format on the [E * N, K] view
//   y[p, :] = dt( x_row(p) . W[idx[p]]^T + bias[idx[p]] ),  x_row(p) = x[p / S] (x_per_pair = 0, x is [T, K]) or x[p] (x_per_pair = 1, [P, K])
//   y[p, :] = +0 where idx[p] is outside [0, E): the index is compared before any address is formed from it
//
// Products are exact, the sum is in fp32, one rounding to the dtype.  A row of y is a function of its own pair only: in both forms a
// row's sum runs over K in an order fixed by K alone, whatever the other pairs are and wherever routing places the row.  Every expert
// and row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E, surplus workgroups leave after
// reading the tile count the routing kernel wrote.
//
// Routed decode form (mx8m_decode_kernel, one launch, P <= 1024): a workgroup per pair and C output columns, the arithmetic and the
// thread-to-unit map of mx8_decode_kernel (mxfp8.hip) for one row: the unit is half a block (MX8_UNIT = 16 bytes of mxfp8_common.cuh,
// one non-temporal 16-byte load), eight v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale 1.0, v_dot2_f32_* into an fp32 partial, the block
// scale on the partial; the workgroup split over its columns in groups of G threads (mx6_decode_group on the unit count), half-wave
// DPP sums, then the LDS sum over the group's half-waves in the same order.  So a live pair's row has the bits of the dense decode form
// at M = 1.  It reads idx[p] and offsets into that expert's rows.  Keeps the fp32 range of W, needs neither e_col nor a workspace.
//   Why the half block here too: the whole-block map (MX8_UNIT = 32) is ahead of the half block at one row on K = 4096 and K = 11008,
//   where K / 32 fills its 128-thread groups in one pass, and this kernel is the one-row instance.  But it is behind at one row on
//   K = 2880 (8.1 against 6.6 us on 2880 -> 5760, the plan comment of mxfp8.hip), the gpt-oss width the expert layers here are measured
//   and used on, and a second unit would give a pair's row other bits than the dense layer gives the same row of the same weights.
// Grouped prefill form (two launches): mxm_route_kernel (mxfp4_moe.hip; the same workspace), then mx8m_gemm_kernel: mxm_tile_begin
// (mxfp4_common.cuh) and mx8_gemm_tile (mxfp8_common.cuh), the 128 x 128 tile of the linear layer's prefill form.  A row tile belongs to
// one expert, gathers its x rows through the pair list and reads weights from (long)e * N; rows past the segment load as zero and are
// not stored; the epilogue scatters row r to y[pair r].  A row's K order is the dense tile's, so a pair's row has the bits of the dense
// prefill form.  The tiles of the skipped bin run no K loop and store zeros.
#include "mxfp8_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// Workgroup: pair blockIdx.y, columns C * blockIdx.x .. + C - 1 of its expert, C = CT * 256 / G (clamped reads past N, never stored).
// Group g = t / G holds columns g CT .. + CT - 1 of those; its thread j = t % G takes the units j, j + G, ... of K.
// It keeps a body of its own beside mx8_decode_kernel's (mxfp8.hip), as mx6m_decode_kernel does beside mx6_decode_kernel's: there the
// shared body measured slower (the comment in mxfp6_moe.hip).  tests/test_mxfp8_moe_gpu.py holds the two bodies to the same bits.
template <int DT, int CT, int G>
__global__ __launch_bounds__(256) void mx8m_decode_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw,
                                                          const uint8_t* __restrict__ sc, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                          int N, int K, int x_per_pair) {
    typedef mx_pair<DT> P;
    typedef mx8_w16<DT> Cv;
    constexpr int C = CT * (256 / G), HPG = G / 32;  // columns per workgroup, half-waves per group
    constexpr int L = MX8_UNIT / 16;                 // 16-byte loads per unit
    __shared__ float red[8][CT];
    const int t = threadIdx.x, g = t / G, j = t % G;
    const int p = blockIdx.y;
    const int e = idx[p];
    if ((unsigned)e >= (unsigned)E) {  // a skipped slot (uniform): zeros, and no address is formed from e
        const int n = blockIdx.x * C + t;
        if (t < C && n < N) dt_traits<DT>::store(y, (long)p * N + n, 0.0f);
        return;
    }
    const int KB = K >> 5, U = K / MX8_UNIT;
    const uint16_t* xr = x + (long)(x_per_pair ? p : p / S) * K;
    const long r0 = (long)e * N;  // the expert's first row of the [E * N, K] view
    const int n0 = blockIdx.x * C + g * CT;
    const uint8_t* wrow[CT];
    const uint8_t* srow[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const long n = r0 + min(n0 + c, N - 1);
        wrow[c] = qw + n * (long)K;
        srow[c] = sc + n * KB;
    }
    float acc[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) acc[c] = 0.0f;
    for (int u = j; u < U; u += G) {
        uint4_t wb[CT][L];
        uint32_t sb[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint4_t* q = reinterpret_cast<const uint4_t*>(wrow[c] + (long)u * MX8_UNIT);
#pragma unroll
            for (int i = 0; i < L; i++) wb[c][i] = __builtin_nontemporal_load(q + i);
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
        const uint4_t* xp = reinterpret_cast<const uint4_t*>(xr + (long)u * MX8_UNIT);
        uint32_t xv[8 * L];
#pragma unroll
        for (int i = 0; i < 2 * L; i++) {
            const uint4_t xq = xp[i];
            xv[4 * i] = xq.x; xv[4 * i + 1] = xq.y; xv[4 * i + 2] = xq.z; xv[4 * i + 3] = xq.w;
        }
#pragma unroll
        for (int c = 0; c < CT; c++) {
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < 8 * L; i++) d = P::dot(wv[c][i], xv[i], d);
            acc[c] += d * s[c];
        }
    }
    const int lane = t & 63;
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const float v = mx6_half_sum_f32(acc[c]);
        if ((lane & 31) == 31) red[t >> 5][c] = v;
    }
    __syncthreads();
    if (t < C) {
        const int n = blockIdx.x * C + t;
        if (n < N) {
            const int h0 = (t / CT) * HPG, c = t % CT;
            float v = red[h0][c];
#pragma unroll
            for (int h = 1; h < HPG; h++) v += red[h0 + h][c];
            if (bias) v += dt_traits<DT>::load(bias, r0 + n);
            dt_traits<DT>::store(y, (long)p * N + n, v);
        }
    }
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
// A workgroup per (row tile of the table, column tile): mx8_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
// Static LDS: the tile's two stages and prow.
static_assert(MXM_BM == MX_BM, "a row tile of the routing is a row tile of mx8_gemm_tile");
static_assert(2 * MX8_STAGE + MXM_BM * 4 <= 65536, "static LDS");

template <int DT>
__global__ __launch_bounds__(256) void mx8m_gemm_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                        const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                                        void* __restrict__ y, int S, int E, int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, MX_BN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx8_gemm_tile<DT>(mx_rows_listed{prow, S, x_per_pair}, x, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launcher --------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MX8M_DECODE_PAIRS (its grid's second dimension).  The plan's bounds were measured
// (tools/mxfp8_moe_bench.py, profiles/mxfp8_moe_bench.jsonl, the `sweep` rows: gpt-oss-20b's 2880 -> 5760 and 2880 -> 2880 at E = 32 and
// 2880 -> 5760 at E = 128, fp16 and bf16, P = 1 .. 1024 (every P the decode form exists for), medians of 7 graph replays, slowest -
// fastest replay under 5 % of the median) and came out where mxfp6_moe.hip's are, although the dense prefill tile is slow at few rows
// (the plan comment of mxfp8.hip): the grouped form pays that per expert with a pair, the decode form pays per pair.  fp16, decode /
// grouped us (bf16 within 5 % except the decode form at P = 2 on 2880 -> 2880, 6.9, and the grouped form at P = 32 there, 124.2):
//     P     2880 -> 5760, E = 32   2880 -> 2880, E = 32   2880 -> 5760, E = 128
//     1          6.9 /  70.6            5.6 /  69.6            7.2 /  70.6
//     4         14.8 /  74.0            9.1 /  71.7           15.3 /  74.1
//    16         45.5 / 154.4           25.3 /  81.6           48.3 / 160.9
//    32         86.8 / 207.2           45.5 / 112.5           92.4 / 251.0
//    64        170.7 / 239.9           87.2 / 154.3          173.1 / 402.4
//   128        341.3 / 246.7          173.5 / 158.2          347.3 / 623.7
//   256        685.7 / 249.7          345.5 / 158.8          701.5 / 871.4
//   512       1394.1 / 254.8          693.5 / 164.1         1423.7 / 970.7
//  1024       2816.1 / 272.6         1392.3 / 169.7         2871.0 / 993.8
// The decode form is ahead at every P <= 64 on every row (at P = 64 by 29 %, 43 % and 2.3 x).  Beyond that it depends on the pairs per
// expert: at E = 32 the grouped form leads from P = 128 on (by 28 % and 9 %, then by 2.7 x and 2.2 x at P = 256), at E = 128 the decode
// form still leads at P = 128 (1.8 x) and at P = 256 (by 19 %; bf16 by 16 %) and is behind at P = 512 = 4 E (1.47 x): the grouped form
// streams the whole weight of every expert that has a pair through a mostly empty row tile, the decode form the weight of every pair
// (its time is linear in P: 2.75 us per pair at 2880 -> 5760).  So the plan takes the decode form for P <= 64, and up to P = 256 while
// P <= 2 E.  Each bound is the largest measured P at which the decode form was ahead: no P between 64 and 128 was measured at E = 32,
// and P = 512 was measured only where P > 2 E, so neither bound goes further.
constexpr int MX8M_DECODE_PAIRS = 1024;
constexpr int MX8M_PLAN_PAIRS = 64, MX8M_PLAN_PAIRS_SPARSE = 256;

// the layer, for the host path of mx_w16_launch.cuh
struct mx8m_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP8_MOE_FORM";
    static constexpr int decode_pairs = MX8M_DECODE_PAIRS, plan_pairs = MX8M_PLAN_PAIRS, plan_pairs_sparse = MX8M_PLAN_PAIRS_SPARSE;
    static constexpr const char *decode_name = "mx8m_decode_kernel", *gemm_name = "mx8m_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int P, int S, int E, int N,
                       int K, int x_per_pair, hipStream_t st) {
        mx6_decode_group(K / MX8_UNIT, [&](auto g) {
            constexpr int G = decltype(g)::value, CT = 4, C = CT * (256 / G);  // mx8_decode_kernel's one-row instance
            hipLaunchKernelGGL((mx8m_decode_kernel<DT, CT, G>), dim3((unsigned)cdiv(N, C), (unsigned)P), dim3(256), 0, st, x, idx, qw, sc, bias, y, S, E, N,
                               K, x_per_pair);
        });
    }
    template <int DT> static constexpr auto gemm() { return mx8m_gemm_kernel<DT>; }
};

int mxfp8_moe_form(long P, long E, long, long, int) { return mx_w16_moe_form<mx8m_w16_layer>(P, E); }
bool mxfp8_moe_decode_ok(long P) { return mx_w16_moe_decode_ok<mx8m_w16_layer>(P); }
int mxfp8_moe_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                             void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_w16_moe_forward_launch<mx8m_w16_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
