// MXFP6 weight-only (W6A16) mixture-of-experts expert GEMM for gfx950: the weights of mxfp6.hip stacked per expert, every (token, slot)
// pair contracted with the expert its index names (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A16 mixture-of-experts layer").  It is
// mxfp4_moe.hip with the weight side of mxfp6.hip.  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]
//   qweight uint8 [E, N, 3K/4], scales uint8 [E, N, K/32], e_col uint8 [E, N], bias [E, N] or NULL: mxfp6.hip's format on the [E * N, K]
//   view (the bytes of the W6A8 expert layer)
//   y[p, :] = dt( x_row(p) . W[idx[p]]^T + bias[idx[p]] ),  x_row(p) = x[p / S] (x_per_pair = 0, x is [T, K]) or x[p] (x_per_pair = 1, [P, K])
//   y[p, :] = +0 where idx[p] is outside [0, E): the index is compared before any address is formed from it
//
// Products are exact, the sum is in fp32, one rounding to the dtype.  A row of y is a function of its own pair only: in both forms a
// row's sum runs over K in an order fixed by K alone, whatever the other pairs are and wherever routing places the row.  Every expert
// and row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E, surplus workgroups leave after
// reading the tile count the routing kernel wrote.
//
// Routed decode form (mx6m_decode_kernel, one launch, P <= 1024): a workgroup per pair and C output columns, the arithmetic and the
// thread-to-block map of mx6_decode_kernel (mxfp6.hip) for one row: per block three 8-byte non-temporal loads, one
// v_cvt_scalef32_pk32_*_fp6 at scale 1.0, v_dot2_f32_* into an fp32 partial, the block scale on the partial; the workgroup split over
// its columns in groups of G threads (mx6_decode_group), half-wave DPP sums, then the LDS sum over the group's half-waves in the same
// order.  So a live pair's row has the bits of the dense decode form at M = 1.  It reads idx[p] and offsets into that expert's rows.
// Keeps the fp32 range of W, needs neither e_col nor a workspace.
// Grouped prefill form (two launches): mxm_route_kernel (mxfp4_moe.hip; the same workspace), then mx6m_gemm_kernel: mxm_tile_begin
// (mxfp4_common.cuh) and mx6_gemm_tile (mxfp6_common.cuh), the 128 x 128 tile of the linear layer's prefill form.  A row tile belongs to
// one expert, gathers its x rows through the pair list and reads weights from (long)e * N; rows past the segment load as zero and are
// not stored; the epilogue scatters row r to y[pair r].  A row's K order is the dense tile's, so a pair's row has the bits of the dense
// prefill form.  The tiles of the skipped bin run no K loop and store zeros.
#include "mxfp6_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// Workgroup: pair blockIdx.y, columns C * blockIdx.x .. + C - 1 of its expert, C = CT * 256 / G (clamped reads past N, never stored).
// Group g = t / G holds columns g CT .. + CT - 1 of those; its thread j = t % G takes the blocks j, j + G, ... of K.
// It keeps a body of its own beside mx6_decode_kernel's (mxfp6.hip).  One body for both (the dense kernel's, called here with one row
// and the expert's row offset) kept registers, LDS and zero scratch but was slower at 64 pairs on 2880 -> 5760, E = 32: shared / own
// body, us by graph replay, medians of three rounds, in two runs of the comparison: fp16 186.54 / 185.75 and 186.35 / 185.64, bf16
// 187.68 / 187.12 and 187.29 / 186.49, against 0.4 - 0.6 us between two arms of the own body.  tests/test_mxfp6_moe_gpu.py holds the
// two bodies to the same bits.
template <int DT, int CT, int G>
__global__ __launch_bounds__(256) void mx6m_decode_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw,
                                                          const uint8_t* __restrict__ sc, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                          int N, int K, int x_per_pair) {
    typedef mx_pair<DT> P;
    typedef mx6_w16<DT> Cv;
    constexpr int C = CT * (256 / G), HPG = G / 32;  // columns per workgroup, half-waves per group
    __shared__ float red[8][CT];
    const int t = threadIdx.x, g = t / G, j = t % G;
    const int p = blockIdx.y;
    const int e = idx[p];
    if ((unsigned)e >= (unsigned)E) {  // a skipped slot (uniform): zeros, and no address is formed from e
        const int n = blockIdx.x * C + t;
        if (t < C && n < N) dt_traits<DT>::store(y, (long)p * N + n, 0.0f);
        return;
    }
    const int KB = K >> 5;
    const uint16_t* xr = x + (long)(x_per_pair ? p : p / S) * K;
    const long r0 = (long)e * N;  // the expert's first row of the [E * N, K] view
    const int n0 = blockIdx.x * C + g * CT;
    const uint8_t* wrow[CT];
    const uint8_t* srow[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const long n = r0 + min(n0 + c, N - 1);
        wrow[c] = qw + n * ((long)KB * MX6_BLOCK_BYTES);
        srow[c] = sc + n * KB;
    }
    float acc[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) acc[c] = 0.0f;
    for (int kb = j; kb < KB; kb += G) {
        uint2_t wb[CT][3];
        uint32_t sb[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint2_t* q = reinterpret_cast<const uint2_t*>(wrow[c] + (long)kb * MX6_BLOCK_BYTES);
#pragma unroll
            for (int i = 0; i < 3; i++) wb[c][i] = __builtin_nontemporal_load(q + i);
            sb[c] = __builtin_nontemporal_load(srow[c] + kb);
        }
        typename Cv::t wv[CT];
        float s[CT];
#pragma unroll
        for (int c = 0; c < CT; c++) {
            wv[c] = Cv::cvt(mx6_v6u{wb[c][0].x, wb[c][0].y, wb[c][1].x, wb[c][1].y, wb[c][2].x, wb[c][2].y}, 1.0f);
            s[c] = e8m0_f32(sb[c]);
        }
        const uint4_t* xp = reinterpret_cast<const uint4_t*>(xr) + 4 * kb;
        const uint4_t x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
        const uint32_t xv[16] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
#pragma unroll
        for (int c = 0; c < CT; c++) {
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; i++) d = P::dot(Cv::pair(wv[c], i), xv[i], d);
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
// A workgroup per (row tile of the table, column tile): mx6_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
// Static LDS: the tile's two stages and prow.
static_assert(MXM_BM == MX_BM, "a row tile of the routing is a row tile of mx6_gemm_tile");
static_assert(2 * MX6_STAGE + MXM_BM * 4 <= 65536, "static LDS");

// mx6_gemm_tile stays a body of its own beside mx_gemm_tile (mxfp4_common.cuh), with which it shares the x staging, the loop frame and
// the epilogue as text.  One frame over a weight-side type (slots, load / store, B fragments, the A fragment's 16 bytes) kept
// registers, LDS and zero scratch, and the MXFP4 GEMMs came out 2 - 5 % faster, but this kernel was slower at 512 pairs on 2880 -> 5760,
// E = 32: shared frame / own body, us by graph replay, medians of three rounds, in two runs of the comparison: fp16 285.65 / 283.36 and
// 284.70 / 283.22, bf16 285.56 / 283.72 and 285.11 / 282.98, against 0.4 - 1.2 us between two arms of the own body.  A frame that only
// some of its four kernels may use is more code than the two bodies, so all four keep theirs.
template <int DT>
__global__ __launch_bounds__(256) void mx6m_gemm_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                        const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                                        void* __restrict__ y, int S, int E, int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, MX_BN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx6_gemm_tile<DT>(mx_rows_listed{prow, S, x_per_pair}, x, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launcher --------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MX6M_DECODE_PAIRS (its grid's second dimension).  The plan's bounds were measured
// (tools/mxfp6_moe_bench.py, profiles/mxfp6_moe_bench.jsonl, the `sweep` rows: gpt-oss-20b's 2880 -> 5760 and 2880 -> 2880 at E = 32 and
// 2880 -> 5760 at E = 128, fp16 and bf16, P = 1 .. 256, medians of 7 graph replays, slowest - fastest replay under 4 %) and came out
// where mxfp4_moe.hip's are.  fp16, decode / grouped us (bf16 within 1 % except the grouped form at P = 32: 235 and 126 at E = 32):
//     P     2880 -> 5760, E = 32   2880 -> 2880, E = 32   2880 -> 5760, E = 128
//     1          6.3 /  76.7            5.6 /  75.2            6.9 /  77.1
//     4         14.8 /  82.0            8.4 /  79.2           16.0 /  81.9
//    16         49.9 / 172.2           27.4 /  90.6           49.3 / 177.4
//    32         96.3 / 223.9           50.8 / 152.9           95.2 / 271.9
//    64        189.3 / 271.5           97.9 / 174.4          187.1 / 460.5
//   128        378.1 / 278.8          193.6 / 177.6          372.7 / 748.1
//   256        763.4 / 280.7          390.3 / 178.9          751.6 / 960.1
// The decode form is ahead at every P <= 64 on every row.  Beyond that it depends on the pairs per expert: at E = 32 the grouped form
// leads from P = 128 on (by 26 % and 8 %, then by 2.7 x and 2.2 x at P = 256), at E = 128 the decode form still leads at P = 128 (2 x)
// and at P = 256 (by 22 %): the grouped form streams the whole weight of every expert that has a pair through a mostly empty row
// tile, the decode form the weight of every pair (its time is linear in P: 2.95 us per pair at 2880 -> 5760).  So the plan takes the
// decode form for P <= 64, and up to P = 256 (the end of the sweep) while P <= 2 E.  The crossover at E = 32 lies between P = 64 and
// P = 128 (by the linear decode time, near P = 94 at 2880 -> 5760 and P = 116 at 2880 -> 2880); no P between them was measured, so the
// bound stays at the last P where the decode form was measured ahead.
constexpr int MX6M_DECODE_PAIRS = 1024;
constexpr int MX6M_PLAN_PAIRS = 64, MX6M_PLAN_PAIRS_SPARSE = 256;

// the layer, for the host path of mx_w16_launch.cuh
struct mx6m_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP6_MOE_FORM";
    static constexpr int decode_pairs = MX6M_DECODE_PAIRS, plan_pairs = MX6M_PLAN_PAIRS, plan_pairs_sparse = MX6M_PLAN_PAIRS_SPARSE;
    static constexpr const char *decode_name = "mx6m_decode_kernel", *gemm_name = "mx6m_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int P, int S, int E, int N,
                       int K, int x_per_pair, hipStream_t st) {
        mx6_decode_group(K >> 5, [&](auto g) {
            constexpr int G = decltype(g)::value, CT = G == 32 ? 2 : 4, C = CT * (256 / G);  // mx6_decode_kernel's one-row instance
            hipLaunchKernelGGL((mx6m_decode_kernel<DT, CT, G>), dim3((unsigned)cdiv(N, C), (unsigned)P), dim3(256), 0, st, x, idx, qw, sc, bias, y, S, E, N,
                               K, x_per_pair);
        });
    }
    template <int DT> static constexpr auto gemm() { return mx6m_gemm_kernel<DT>; }
};

int mxfp6_moe_form(long P, long E, long, long, int) { return mx_w16_moe_form<mx6m_w16_layer>(P, E); }
bool mxfp6_moe_decode_ok(long P) { return mx_w16_moe_decode_ok<mx6m_w16_layer>(P); }
int mxfp6_moe_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                             void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_w16_moe_forward_launch<mx6m_w16_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
