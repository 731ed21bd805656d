// MXFP4 W4A4 expert GEMM for gfx950: the stacked expert weights of mxfp4_moe.hip against activations quantised to MXFP4 on the fly,
// contracted on the block-scaled matrix instructions (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A4 mixture-of-experts layer").  No
// reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]; row(p) = p / S (x_per_pair = 0) or p
//   xq / xs / row_flag: the stored rows of x (T or P of them) by the rule of mxa4_quantize_kernel (mxfp4_a4.hip)
//   y[p, n] = dt( sum_b 2^(xs[row(p), b] + scales[e, n, b] - 254) * (sum_{k in b} e2m1(xq) * e2m1(qweight)) + bias[e, n] ),  e = idx[p]
//   y[p, :] = NaN where row_flag[row(p)]; y[p, n] = NaN where e_col[e, n] == 255; y[p, :] = +0 where idx[p] is outside [0, E), whatever
//   the row's flag: the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone.  Every expert and
// row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E.
//
// Routed decode form (mxma4_decode_kernel, P <= 1024): a workgroup per pair and strip of 16 C16 columns of its expert, K split over the
// 4 waves in 128-k steps, on v_mfma_scale_f32_16x16x128_f8f6f4.  The pair's row is row 0 of the x operand,
// rows 1 .. 15 are zero codes under scale code 127; the four partial sums meet in LDS.  FUSED (one launch, K <= MXMA4_ONE_K): the
// workgroup quantises x_row(p) into LDS itself (a4_quantize_unit, the bits of mxa4_quantize_kernel; codes, scale bytes, and the
// non-finite flag through the barrier) and reads neither xq nor a workspace.  Not FUSED: it reads xq / xs / row_flag from memory.
// Grouped prefill form: mxa4_quantize_kernel over the stored rows, mxm_route_kernel (mxfp4_moe.hip; the same workspace), then
// mxma4_gemm_kernel: mxm_tile_begin (mxfp4_common.cuh) and mx_scaled_gemm_tile (mx_scaled_tile.cuh; FP4 x FP4) at 128 x 128, the tile of the W4A4 linear
// layer's prefill form.  A row tile belongs to one expert, gathers the xq / xs rows of its pairs through the pair list (whole 16-byte
// pieces of codes, whole scale bytes) and reads weights from (long)e * N; rows past the segment enter as zero codes under scale code
// 127 and are not stored; the epilogue scatters row r to y[pair r].  The tiles of the skipped bin run no K loop and store zeros.
#include "mxfp4_a4_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// The largest K of the one-launch form: a row's image in LDS is K / 2 bytes of codes and K / 32 scale bytes (17408 bytes at the bound).
constexpr int MXMA4_ONE_K = 32768;
constexpr int MXMA4_DECODE_PAIRS = 1024;  // the grid's second dimension

// Workgroup: pair blockIdx.y, columns 16 C16 blockIdx.x .. + 16 C16 - 1 of its expert (reads past N clamped, never stored).  Wave w takes
// the 128-k steps w, w + 4, ...; lane l holds column l & 15 of each of the C16 groups and block l >> 4 of the step.  xin is x (FUSED) or xq.
template <int DT, int C16, bool FUSED>
__global__ __launch_bounds__(256) void mxma4_decode_kernel(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                           const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                           int N, int K, int x_per_pair) {
    constexpr int C = 16 * C16;
    __shared__ float red[4][C];
    __shared__ __attribute__((aligned(16))) unsigned char img[FUSED ? MXMA4_ONE_K / 2 + MXMA4_ONE_K / 32 : 16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int p = blockIdx.y, n0 = blockIdx.x * C;
    const int e = idx[p];
    if ((unsigned)e >= (unsigned)E) {  // a skipped slot (uniform): zeros, and no address is formed from e
        if (t < C && n0 + t < N) dt_traits<DT>::store(y, (long)p * N + n0 + t, 0.0f);
        return;
    }
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const long xrow = x_per_pair ? p : p / S;
    const uint8_t* xqr = nullptr;
    const uint8_t* xsr = nullptr;
    int flagged;
    if constexpr (FUSED) {
        const uint16_t* xr = reinterpret_cast<const uint16_t*>(xin) + xrow * K;
        const int U = K >> 3;  // a multiple of 4: whole quads are in or out
        int bad = 0;
        for (int u = t; u < U; u += 256) {
            uint32_t codes, scode;
            a4_quantize_unit<DT>(*reinterpret_cast<const uint4_t*>(xr + (long)u * 8), bad, codes, scode);
            reinterpret_cast<uint32_t*>(img)[u] = codes;
            if ((u & 3) == 0) img[(K >> 1) + (u >> 2)] = (unsigned char)scode;
        }
        flagged = __syncthreads_or(bad);  // the barrier that publishes the image
    } else {
        xqr = reinterpret_cast<const uint8_t*>(xin) + xrow * (K >> 1);
        xsr = xs + xrow * KB;
        flagged = row_flag[xrow];
    }
    const long r0 = (long)e * N;  // the expert's first row of the [E * N, K] view
    const uint8_t* wrow[C16];
    const uint8_t* srow[C16];
#pragma unroll
    for (int c = 0; c < C16; c++) {
        const long n = r0 + min(n0 + c * 16 + r16, N - 1);
        wrow[c] = qw + n * (K >> 1);
        srow[c] = sc + n * KB;
    }
    mxa4_v4f acc[C16];
#pragma unroll
    for (int c = 0; c < C16; c++) acc[c] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);  // weight loads are clamped and unconditional, then masked
        const bool kin = kb < KB;
        uint4_t b[C16];
        int sb[C16];
#pragma unroll
        for (int c = 0; c < C16; c++) {
            b[c] = __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wrow[c]) + kc);
            sb[c] = __builtin_nontemporal_load(srow[c] + kc);
        }
        uint4_t a = uint4_t{0u, 0u, 0u, 0u};
        int sa = 127;
        if (r16 == 0 && kin) {
            if constexpr (FUSED) {
                a = *reinterpret_cast<const uint4_t*>(img + kb * 16);
                sa = img[(K >> 1) + kb];
            } else {
                a = reinterpret_cast<const uint4_t*>(xqr)[kb];
                sa = xsr[kb];
            }
        }
        if (!kin) {
#pragma unroll
            for (int c = 0; c < C16; c++) {
                b[c] = uint4_t{0u, 0u, 0u, 0u};
                sb[c] = 127;
            }
        }
#pragma unroll
        for (int c = 0; c < C16; c++) acc[c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a4_frag(a), a4_frag(b[c]), acc[c], 4, 4, 0, sa, 0, sb[c]);
    }
    // C/D: column n = lane & 15, row m = 4 (lane >> 4) + r: the pair's row is register 0 of lanes 0 .. 15
    if (lane < 16) {
#pragma unroll
        for (int c = 0; c < C16; c++) red[wave][c * 16 + lane] = acc[c][0];
    }
    __syncthreads();
    if (t < C) {
        const int n = n0 + t;
        if (n < N) {
            float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            if (flagged || ecol[r0 + n] == 255u) v = a4_nan();
            if (bias) v += dt_traits<DT>::load(bias, r0 + n);
            dt_traits<DT>::store(y, (long)p * N + n, v);
        }
    }
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
constexpr int MXMA4_W = 2;  // WM = WN of the tile: 128 x 128
static_assert(64 * MXMA4_W == MXM_BM, "a row tile of the routing is a row tile of the GEMM");

// A workgroup per (row tile of the table, column tile): mx_scaled_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT>
__global__ __launch_bounds__(256) void mxma4_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                         int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, 64 * MXMA4_W>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_scaled_gemm_tile<DT, MXMA4_W, MXMA4_W, mx_op_fp4, mx_op_fp4>(mx_rows_listed{prow, S, x_per_pair}, xq, xs, row_flag, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MXMA4_DECODE_PAIRS.  The plan's bound was measured (tools/mxfp4_moe_a4_bench.py,
// profiles/mxfp4_moe_a4_bench.jsonl, the `sweep` rows: both gpt-oss-20b projections at E = 32 and E = 128, fp16 and bf16, both forms
// forced at P = 1, 2, 4, ..., 1024, graph time, routings and weight stacks rotated; fp16 and bf16 agree within 1 %).  The decode form
// streams an expert's weights once per pair and grows linearly in P (9.4 / 16.8 / 51 / 96 / 184 / 363 us at P = 1 / 4 / 16 / 32 / 64 /
// 128 on 2880 -> 5760); the grouped form costs 37 us at P = 1 (three launches, one row tile walking K) and then grows with the number
// of experts that hold a pair.  At E = 32 the decode form led at every P <= 32 (P = 32: 96 against 134 us at 5760, 51 against 70 at
// 2880) and the grouped form from P = 64 on (184 against 139, 95 against 69; 723 against 145 at P = 256).  At E = 128, where nearly
// every pair of a small call has an expert of its own, the decode form still led at P = 64 (186 against 231 - 250 us, 97 against 131);
// P = 128 was a tie either way (367 against 345 - 352 at 5760, 187 against 196 at 2880) and the grouped form led from P = 256 on (734
// against 452, 371 against 261).  So the plan takes the decode form for P <= 32, and up to P = 64 while P <= E / 2.  E between 32 and
// 128 and beyond 128 was not measured: the second clause extends the E = 128 rows by the pairs-per-expert argument.  (The rows' `plan`
// column is the plan of the build that measured them, the weight-only plan's 64 / 256 / 2 E, which these rows replaced.)
// The strip width of the decode form: 16, 32 and 64 columns per workgroup measured at P = 1, 4, 16, 64 on both projections (the `strip`
// rows): 16 columns were ahead or level on every row (P = 1: 8.9 / 9.3 / 12.3 us at 5760; P = 64: 174 / 183 / 199), so the wider
// strips' saving of the per-workgroup quantisation does not pay for their fewer workgroups.
constexpr int MXMA4_PLAN_PAIRS = 32, MXMA4_PLAN_PAIRS_SPARSE = 64;
constexpr int MXMA4_STRIP = 1;  // C16 of the decode form: strips of 16 columns (BIE_MXFP4_MOE_A4_STRIP = 1 / 2 / 4 under BIE_TUNING)

// Workspace of bie_mxfp4_moe_a4_forward: xq [R, K/2], xs [R, K/32], row_flag [R], then the routing region (mx_scaled_launch.cuh)
struct mxma4_layer {
    using act = mx_act_fp4;
    static constexpr const char* form_knob = "BIE_MXFP4_MOE_A4_FORM";
    static constexpr const char* strip_knob = "BIE_MXFP4_MOE_A4_STRIP";
    static constexpr const char* wn_knob = nullptr;
    static constexpr int one_k = MXMA4_ONE_K, decode_pairs = MXMA4_DECODE_PAIRS;
    static constexpr int plan_pairs = MXMA4_PLAN_PAIRS, plan_pairs_sparse = MXMA4_PLAN_PAIRS_SPARSE, plan_sparse_mul = 2;
    static constexpr int strip = MXMA4_STRIP, wn = MXMA4_W;
    static constexpr const char* decode_name = "mxma4_decode_kernel";
    static constexpr const char* gemm_name = "mxma4_gemm_kernel";
    template <int DT, int C16, bool FUSED> static constexpr auto decode() { return mxma4_decode_kernel<DT, C16, FUSED>; }
    template <int DT, int WN> static constexpr auto gemm() { return mxma4_gemm_kernel<DT>; }
};

bool mxfp4_moe_a4_decode_ok(long P) { return mx_grouped_decode_ok<mxma4_layer>(P); }
bool mxfp4_moe_a4_one_launch_ok(long K) { return mx_grouped_one_launch_ok<mxma4_layer>(K); }
int mxfp4_moe_a4_form(long P, long E, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_grouped_form<mxma4_layer>(P, E); }
size_t mxfp4_moe_a4_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_workspace_bytes<mxma4_layer>(T, S, E, K, x_per_pair, form);
}

int mxfp4_moe_a4_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                             const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair,
                             int dtype, int form, hipStream_t st) {
    return mx_grouped_gemm_launch<mxma4_layer>(xq, xs, row_flag, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

int mxfp4_moe_a4_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                                void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_grouped_forward_launch<mxma4_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
