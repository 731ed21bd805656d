// MXFP4 W4A8 expert GEMM for gfx950: the stacked expert weights of mxfp4_moe.hip against activations quantised to MXFP8 (E4M3 elements,
// E8M0 block scales) on the fly, contracted on the block-scaled matrix instructions with an FP4 A operand and an E4M3 B operand
// (include/bie_hip.h, INTEGRATION.md "MXFP4 W4A8 mixture-of-experts layer").  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]; row(p) = p / S (x_per_pair = 0) or p
//   xq uint8 [R, K] (e4m3fn bytes) / xs uint8 [R, K/32] / row_flag uint8 [R]: the stored rows of x (R = T or P) by the rule of
//   mxa8_quantize_kernel (mxfp4_a8.hip)
//   y[p, n] = dt( sum_b 2^(xs[row(p), b] + scales[e, n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m1(qweight)) + bias[e, n] ),  e = idx[p]
//   y[p, :] = NaN where row_flag[row(p)]; y[p, n] = NaN where e_col[e, n] == 255; y[p, :] = +0 where idx[p] is outside [0, E), whatever
//   the row's flag: the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone.  Every expert and
// row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E.
//
// Routed decode form (mxma8_decode_kernel, P <= 1024): mx_scaled_decode_pair (FP4 x E4M3) of mx_scaled_decode.cuh, in the operand
// order of mxfp4_a8.hip (the only one profiles/mxfp4_a8_probe.txt pinned): the weight fragment is A (FP4, cbsz 4), the x fragment B
// (E4M3, blgp 0, the two halves of a8_frag), byte select 0; a pair's row has the bits of the dense W4A8 decode form.  FUSED (one
// launch, K <= MXMA8_ONE_K): the row image in LDS is written by mx_quantize_row, which mxa8_quantize_kernel calls too.
// Grouped prefill form: mxa8_quantize_kernel over the stored rows, mxm_route_kernel (mxfp4_moe.hip; the same workspace), then
// mxma8_gemm_kernel: mxm_tile_begin (mxfp4_common.cuh) and mx_scaled_gemm_tile (mx_scaled_tile.cuh; FP4 x E4M3) at 128 x 128.  A row tile belongs to one
// expert, gathers the xq / xs rows of its pairs through the pair list and reads weights from (long)e * N; rows past the segment enter
// as zero codes under scale code 127 and are not stored; the epilogue scatters row r to y[pair r].  The tiles of the skipped bin run no
// K loop and store zeros.
#include "mxfp4_a8_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// The largest K of the one-launch form: a row's image in LDS is K bytes of codes and K / 32 scale bytes (16896 bytes at the bound, the
// footprint class of the W4A4 kernel's 17408, whose occupancy is the measured one).
constexpr int MXMA8_ONE_K = 16384;
constexpr int MXMA8_DECODE_PAIRS = 1024;  // the grid's second dimension

// A workgroup per pair and strip of 16 C16 columns of its expert (mx_scaled_decode_pair).  xin is x (FUSED) or the quantised rows.
template <int DT, int C16, bool FUSED>
__global__ __launch_bounds__(256) void mxma8_decode_kernel(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                           const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                           int N, int K, int x_per_pair) {
    mx_scaled_decode_pair<DT, C16, FUSED, mx_op_fp4, mx_op_e4m3, MXMA8_ONE_K>(xin, xs, row_flag, idx, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair);
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
constexpr int MXMA8_W = 2;  // WM = WN of the tile: 128 x 128
static_assert(64 * MXMA8_W == MXM_BM, "a row tile of the routing is a row tile of the GEMM");

// A workgroup per (row tile of the table, column tile): mx_scaled_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT>
__global__ __launch_bounds__(256) void mxma8_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                         int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, 64 * MXMA8_W>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_scaled_gemm_tile<DT, MXMA8_W, MXMA8_W, mx_op_fp4, mx_op_e4m3>(mx_rows_listed{prow, S, x_per_pair}, xq, xs, row_flag, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MXMA8_DECODE_PAIRS.  The plan's bound was measured (tools/mxfp4_moe_a8_bench.py,
// profiles/mxfp4_moe_a8_bench.jsonl, the `sweep` rows: both gpt-oss-20b projections at E = 32 and E = 128, fp16 and bf16, both forms
// forced at P = 1, 2, 4, ..., 1024, graph time, routings and weight stacks rotated; fp16 and bf16 agree within 4 % but for the
// decode rows at E = 128, P <= 16 (5 - 11 %) and one grouped row (12 %): no verdict below turns on that).  The decode form streams an expert's weights once per pair and grows linearly in P (7.5 / 15.2 / 47 / 90 / 175 / 349 us at
// P = 1 / 4 / 16 / 32 / 64 / 128 on 2880 -> 5760); the grouped form costs 41 us at P = 1 (three launches, one row tile walking K) and
// then grows with the number of experts that hold a pair.  At E = 32 the decode form led at every P <= 32 (P = 32: 90 against 143 - 148
// us at 5760, 46 against 79 at 2880); P = 64 was split (175 against 165 at 5760, 88 against 99 - 101 at 2880) and the grouped form led
// from P = 128 on (349 against 168, 173 against 108 - 110).  At E = 128, where nearly every pair of a small call has an expert of its
// own, the decode form led through P = 128 (P = 64: 177 against 267, 91 against 158; P = 128: 355 against 426 - 432, 179 against 221)
// and the grouped form from P = 256 on (713 against 538 - 553, 352 against 312).  So the plan takes the decode form for P <= 32, and up
// to P = 128 while P <= E.  The second bound is wider than the W4A4 layer's (64 while 2 P <= E) because this layer's grouped form is the
// slower of the two (the `accept` rows: 1.07 - 1.48 x the W4A4 grouped form's time) while its decode form is the faster.  E between 32
// and 128 and beyond 128, and P between the powers of two, were not measured: the second clause extends the E = 128 rows by the
// pairs-per-expert argument.  (The rows' `plan` column is the plan of the build that measured them, the W4A4 constants 32 / 64 / 2 P <= E,
// which these rows replaced; the `accept` rows ran P = 4, 64, 1024 and 16384 at E = 32, where both plans choose alike.)
// The strip width of the decode form: 16, 32 and 64 columns per workgroup measured at P = 1, 4, 16, 64 on both projections (the `strip`
// rows): 16 columns were ahead or level (within 1 %) on every row (P = 1: 7.2 / 7.7 / 10.6 us at 5760; P = 64: 175 / 183 / 198).
constexpr int MXMA8_PLAN_PAIRS = 32, MXMA8_PLAN_PAIRS_SPARSE = 128;
constexpr int MXMA8_STRIP = 1;  // C16 of the decode form: strips of 16 columns (BIE_MXFP4_MOE_A8_STRIP = 1 / 2 / 4 under BIE_TUNING)

// Workspace of bie_mxfp4_moe_a8_forward: xq [R, K], xs [R, K/32], row_flag [R], then the routing region (mx_scaled_launch.cuh)
struct mxma8_layer {
    using act = mx_act_e4m3;
    static constexpr const char* form_knob = "BIE_MXFP4_MOE_A8_FORM";
    static constexpr const char* strip_knob = "BIE_MXFP4_MOE_A8_STRIP";
    static constexpr const char* wn_knob = nullptr;
    static constexpr int one_k = MXMA8_ONE_K, decode_pairs = MXMA8_DECODE_PAIRS;
    static constexpr int plan_pairs = MXMA8_PLAN_PAIRS, plan_pairs_sparse = MXMA8_PLAN_PAIRS_SPARSE, plan_sparse_mul = 1;
    static constexpr int strip = MXMA8_STRIP, wn = MXMA8_W;
    static constexpr const char* decode_name = "mxma8_decode_kernel";
    static constexpr const char* gemm_name = "mxma8_gemm_kernel";
    template <int DT, int C16, bool FUSED> static constexpr auto decode() { return mxma8_decode_kernel<DT, C16, FUSED>; }
    template <int DT, int WN> static constexpr auto gemm() { return mxma8_gemm_kernel<DT>; }
};

bool mxfp4_moe_a8_decode_ok(long P) { return mx_grouped_decode_ok<mxma8_layer>(P); }
bool mxfp4_moe_a8_one_launch_ok(long K) { return mx_grouped_one_launch_ok<mxma8_layer>(K); }
int mxfp4_moe_a8_form(long P, long E, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_grouped_form<mxma8_layer>(P, E); }
size_t mxfp4_moe_a8_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_workspace_bytes<mxma8_layer>(T, S, E, K, x_per_pair, form);
}

int mxfp4_moe_a8_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                             const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair,
                             int dtype, int form, hipStream_t st) {
    return mx_grouped_gemm_launch<mxma8_layer>(xq, xs, row_flag, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

int mxfp4_moe_a8_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                                void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_grouped_forward_launch<mxma8_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
