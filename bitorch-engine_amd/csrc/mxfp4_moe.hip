// MXFP4 mixture-of-experts expert GEMM for gfx950: the weights of mxfp4.hip stacked per expert, every (token, slot) pair contracted with
// the expert its index names (include/bie_hip.h, INTEGRATION.md "MXFP4 mixture-of-experts layer").  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]
//   qweight uint8 [E, N, K/2], scales uint8 [E, N, K/32], e_col uint8 [E, N], bias [E, N] or NULL: mxfp4.hip's format on the [E * N, K] view
//   y[p, :] = dt( x_row(p) . W[idx[p]]^T + bias[idx[p]] ),  x_row(p) = x[p / S] (x_per_pair = 0, x is [T, K]) or x[p] (x_per_pair = 1, [P, K])
//   y[p, :] = 0 where idx[p] is outside [0, E): the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone, whatever the
// other pairs are and wherever routing places the row.  Every expert and row offset is 64-bit.  Nothing synchronises with the host: the
// grids are sized from P and E, surplus workgroups leave after reading the tile count the routing kernel wrote.
//
// Routed decode form (mxm_decode_kernel, one launch): a workgroup per pair and C output columns, the arithmetic of mxfp4.hip's decode
// form for one row (v_cvt_scalef32_pk_*_fp4 at scale 1, v_dot2_f32_*, the block scale on the fp32 partial, DPP sums).  It reads idx[p] and
// offsets into that expert's rows.  Keeps the fp32 range of W, needs neither e_col nor a workspace.
// Grouped prefill form (two launches):
//   mxm_route_kernel, one workgroup: an LDS histogram of the pairs over the experts (the skipped pairs in a bin of their own), an
//   exclusive scan, the tile table (expert, first entry, rows) with every expert's segment cut into row tiles of MXM_BM, and the pair
//   list ordered by expert.  The order of the pairs inside a segment is that of the LDS atomics' arrival; no row of y depends on it.
//   mxm_gemm_kernel: mxm_tile_begin and mx_gemm_tile of mxfp4_common.cuh, the 128 x 128 tile of the linear layer's prefill form (packed
//   codes staged in LDS, converted in registers, columns rebiased by e_col[e, n]).  A row tile belongs to one expert and gathers its x
//   rows through the pair list, each row in whole 16-byte pieces; rows past the segment load as zero and are not stored; the epilogue
//   scatters row r to y[pair r].  The tiles of the skipped bin run no K loop and store zeros.
#include "mxfp4_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// Workgroup: pair blockIdx.y, columns C * blockIdx.x .. + C - 1 of its expert (clamped reads past N, never stored).  Thread t takes the
// 16-value units u = t, t + 256, ... of K: per column 8 code bytes and the scale byte of block u / 2.
// It keeps a body of its own beside mx_decode_kernel's (mxfp4.hip), whose arithmetic it repeats for one row.  One body for both (the
// dense kernel's, called here with one row and the expert's row offset) kept registers, LDS and zero scratch but was slower at 64 pairs
// on 4096 x 4096, E = 32: shared / own body, us by graph replay, medians of three rounds, in two runs of the comparison: fp16
// 114.26 / 112.48 and 115.32 / 114.63, bf16 113.19 / 111.77 and 114.20 / 113.16, against 0.4 - 0.9 us between two arms of the own body.
// tests/test_mxfp4_moe_gpu.py holds the two bodies to the same bits.
template <int DT, int C>
__global__ __launch_bounds__(256) void mxm_decode_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw,
                                                         const uint8_t* __restrict__ sc, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                         int N, int K, int x_per_pair) {
    typedef mx_pair<DT> P;
    __shared__ float red[4][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.y, n0 = blockIdx.x * C;
    const int e = idx[p];
    if ((unsigned)e >= (unsigned)E) {  // a skipped slot (uniform): zeros, and no address is formed from e
        if (threadIdx.x < C && n0 + (int)threadIdx.x < N) dt_traits<DT>::store(y, (long)p * N + n0 + threadIdx.x, 0.0f);
        return;
    }
    const int U = K >> 4, KB = K >> 5;
    const uint16_t* xr = x + (long)(x_per_pair ? p : p / S) * K;
    const long r0 = (long)e * N;  // the expert's first row of the [E * N, K] view
    const uint8_t* wrow[C];
    const uint8_t* srow[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        const long n = r0 + min(n0 + c, N - 1);
        wrow[c] = qw + n * (K >> 1);
        srow[c] = sc + n * KB;
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.0f;
    for (int u = threadIdx.x; u < U; u += 256) {
        uint2_t wb[C];
        uint32_t sb[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
            wb[c] = __builtin_nontemporal_load(reinterpret_cast<const uint2_t*>(wrow[c]) + u);
            sb[c] = __builtin_nontemporal_load(srow[c] + (u >> 1));
        }
        const uint4_t* xp = reinterpret_cast<const uint4_t*>(xr) + 2 * u;
        const uint4_t x0 = xp[0], x1 = xp[1];
        const uint32_t xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int c = 0; c < C; c++) {
            typename P::t wv[8];
            mx_unpack16<DT>(wb[c], wv);
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; j++) s = P::dot(wv[j], xv[j], s);
            acc[c] += s * e8m0_f32(sb[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float v = wave_sum_f32(acc[c]);
        if (lane == 0) red[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int c = threadIdx.x, n = n0 + c;
        if (n < N) {
            float v = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
            if (bias) v += dt_traits<DT>::load(bias, r0 + n);
            dt_traits<DT>::store(y, (long)p * N + n, v);
        }
    }
}

// ---- grouped prefill form: routing --------------------------------------------------------------------------------------------------------
static_assert(MXM_BM == MX_BM, "a row tile of the routing is a row tile of mx_gemm_tile");  // both: mxfp4_common.cuh

// Workspace (int32): head [MXM_HEAD], tile_expert [max_tiles], tile_first [max_tiles], tile_rows [max_tiles], pair list [P].
// max_tiles bounds sum_e ceil(count_e / BM) + ceil(skipped / BM): every tile holds a pair, and at most one tile per bin is not full.
static long mxm_max_tiles(long P, long E) { return P < P / MXM_BM + E + 1 ? P : P / MXM_BM + E + 1; }

// One workgroup of 1024 threads, bin e of the scan on thread e.  Two passes over idx: count, then place.  One workgroup keeps the
// histogram and the cursors in LDS and needs no counters zeroed between calls; its cost is P / 1024 iterations per thread and pass on
// one CU before the GEMM can start: 16 at P = 16384 (15 us against the GEMM's 988 us at 2880 -> 5760: profiles/mxfp4_moe_kernel_stats.csv), 4096 at the largest
// admitted P = 2^22, where the routing is expected to take milliseconds.  That is a known limit: a multi-workgroup routing (per-workgroup
// LDS histograms merged with vector atomics) is the follow-up if calls of millions of pairs matter.
__global__ __launch_bounds__(1024) void mxm_route_kernel(const int32_t* __restrict__ idx, int32_t* __restrict__ ws, int P, int E, int max_tiles) {
    __shared__ int cnt[MXM_MAX_E], cur[MXM_MAX_E];
    __shared__ int poff[MXM_MAX_E + 1], toff[MXM_MAX_E + 1];  // exclusive pair / tile offsets of the bins; [E] = the skipped bin's
    __shared__ unsigned long long scan[2][MXM_MAX_E];
    __shared__ int nskip, curskip;
    const int t = threadIdx.x;
    cnt[t] = 0;
    cur[t] = 0;
    if (t == 0) nskip = 0, curskip = 0;
    __syncthreads();
    for (int p = t; p < P; p += 1024) {
        const int e = idx[p];
        atomicAdd((unsigned)e < (unsigned)E ? &cnt[e] : &nskip, 1);
    }
    __syncthreads();
    // inclusive scan of (tiles << 32 | pairs) over the 1024 bins (bins from E on are empty)
    const int c = cnt[t];
    const unsigned long long v = ((unsigned long long)((c + MXM_BM - 1) / MXM_BM) << 32) | (unsigned)c;
    scan[0][t] = v;
    __syncthreads();
    int b = 0;
    for (int d = 1; d < MXM_MAX_E; d <<= 1, b ^= 1) {
        unsigned long long a = scan[b][t];
        if (t >= d) a += scan[b][t - d];
        scan[b ^ 1][t] = a;
        __syncthreads();
    }
    const unsigned long long inc = scan[b][t];
    poff[t] = (int)(uint32_t)(inc - v);
    toff[t] = (int)((inc - v) >> 32);
    if (t == MXM_MAX_E - 1) {
        poff[MXM_MAX_E] = (int)(uint32_t)inc;
        toff[MXM_MAX_E] = (int)(inc >> 32);
    }
    __syncthreads();
    const int live_tiles = toff[E], live_pairs = poff[E];
    const int n_tiles = live_tiles + (nskip + MXM_BM - 1) / MXM_BM;  // <= max_tiles (see mxm_max_tiles)
    int32_t* tile_expert = ws + MXM_HEAD;
    int32_t* tile_first = tile_expert + max_tiles;
    int32_t* tile_rows = tile_first + max_tiles;
    int32_t* list = tile_rows + max_tiles;
    if (t == 0) ws[0] = n_tiles;
    for (int i = t; i < n_tiles; i += 1024) {
        int e, first, left;
        if (i >= live_tiles) {
            e = E;
            first = live_pairs + (i - live_tiles) * MXM_BM;
            left = live_pairs + nskip - first;
        } else {  // the last bin of [0, E) whose first tile is at or before i: the one that holds tile i (empty bins share an offset)
            int lo = 0, hi = E - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (toff[mid] <= i) lo = mid; else hi = mid - 1;
            }
            e = lo;
            first = poff[e] + (i - toff[e]) * MXM_BM;
            left = poff[e] + cnt[e] - first;
        }
        tile_expert[i] = e;
        tile_first[i] = first;
        tile_rows[i] = left < MXM_BM ? left : MXM_BM;
    }
    for (int p = t; p < P; p += 1024) {
        const int e = idx[p];
        const bool live = (unsigned)e < (unsigned)E;
        const int at = atomicAdd(live ? &cur[e] : &curskip, 1);
        list[(live ? poff[e] : live_pairs) + at] = p;
    }
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
// A workgroup per (row tile of the table, column tile): mx_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT>
__global__ __launch_bounds__(256) void mxm_gemm_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                       const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                                       void* __restrict__ y, int S, int E, int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, MX_BN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_gemm_tile<DT>(mx_rows_listed{prow, S, x_per_pair}, x, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launcher --------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MXM_DECODE_PAIRS (its grid's second dimension).  The plan's bound was measured
// (tools/mxfp4_moe_bench.py, profiles/mxfp4_moe_bench.jsonl, the `sweep` rows: gpt-oss-20b's 2880 -> 5760 and 2880 -> 2880 at E = 32
// and 2880 -> 5760 at E = 128, fp16 and bf16, P = 1 .. 256).  The decode form was ahead at every P <= 64 on every row (at P = 64:
// 138 / 69 us against 197 / 97 at E = 32, 139 against 385 - 398 at E = 128).  Beyond that it depends on the pairs per expert: at
// E = 32 the grouped form leads from P = 128 on (277 against 209 - 211 us at 5760, 132 against 102 - 103 at 2880; 560 against 215 at
// P = 256), at E = 128 the decode form still leads at P = 128 and 256 (279 against 569 - 592 us, 564 against 774 - 779): the grouped
// form streams the whole weight of every expert that has a pair through a mostly empty row tile, the decode form the weight of
// every pair.  So the plan takes the decode form for P <= 64, and up to P = 256 (the end of the sweep) while P <= 2 E.  (The rows' `plan`
// column is the plan of the build that measured them, P <= 64 alone; the E = 128 rows are what added the second clause.)
constexpr int MXM_DECODE_PAIRS = 1024;
constexpr int MXM_PLAN_PAIRS = 64, MXM_PLAN_PAIRS_SPARSE = 256;

size_t mxfp4_moe_workspace_bytes(long P, long E) {
    const size_t words = (size_t)MXM_HEAD + 3 * (size_t)mxm_max_tiles(P, E) + (size_t)P;
    return (words * 4 + 15) / 16 * 16;
}

// The routing launch, shared with the W4A4 expert GEMM (mxfp4_moe_a4.hip): the workspace layout above, row tiles of MXM_BM = 128.
long mxfp4_moe_max_tiles(long P, long E) { return mxm_max_tiles(P, E); }

int mxfp4_moe_route_launch(const int32_t* idx, void* workspace, long P, long E, hipStream_t st) {
    hipLaunchKernelGGL(mxm_route_kernel, dim3(1), dim3(1024), 0, st, idx, reinterpret_cast<int32_t*>(workspace), (int)P, (int)E, (int)mxm_max_tiles(P, E));
    return check_launch("mxm_route_kernel");
}

// the layer, for the host path of mx_w16_launch.cuh
struct mx4m_w16_layer {
    static constexpr const char* form_knob = "BIE_MXFP4_MOE_FORM";
    static constexpr int decode_pairs = MXM_DECODE_PAIRS, plan_pairs = MXM_PLAN_PAIRS, plan_pairs_sparse = MXM_PLAN_PAIRS_SPARSE;
    static constexpr const char *decode_name = "mxm_decode_kernel", *gemm_name = "mxm_gemm_kernel";
    template <int DT>
    static void decode(const uint16_t* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const void* bias, void* y, int P, int S, int E, int N,
                       int K, int x_per_pair, hipStream_t st) {
        constexpr int C = 4;  // mx_decode_kernel's one-row instance
        hipLaunchKernelGGL((mxm_decode_kernel<DT, C>), dim3((unsigned)cdiv(N, C), (unsigned)P), dim3(256), 0, st, x, idx, qw, sc, bias, y, S, E, N, K, x_per_pair);
    }
    template <int DT> static constexpr auto gemm() { return mxm_gemm_kernel<DT>; }
};

int mxfp4_moe_form(long P, long E, long, long, int) { return mx_w16_moe_form<mx4m_w16_layer>(P, E); }
bool mxfp4_moe_decode_ok(long P) { return mx_w16_moe_decode_ok<mx4m_w16_layer>(P); }
int mxfp4_moe_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                             void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_w16_moe_forward_launch<mx4m_w16_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
