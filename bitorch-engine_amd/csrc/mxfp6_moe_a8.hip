// MXFP6 W6A8 expert GEMM for gfx950: stacked MXFP6 expert weights (E2M3 elements, E8M0 block scales; the format of mxfp6_a8.hip per
// expert) against activations quantised to MXFP8 (E4M3 elements, E8M0 block scales) on the fly, contracted on the block-scaled matrix
// instructions with an FP6 A operand and an E4M3 B operand (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A8 mixture-of-experts layer").
// It is mxfp4_moe_a8.hip with the weight side of mxfp6_a8.hip.  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]; row(p) = p / S (x_per_pair = 0) or p
//   qweight uint8 [E, N, 3K/4]: per row K/32 blocks of 24 bytes, code j of a block in bits 6 j .. 6 j + 5 (the dense layer's bit order)
//   scales uint8 [E, N, K/32]; e_col uint8 [E, N] = bie_mxfp4_col_exp on the [E * N, K/32] view
//   xq uint8 [R, K] (e4m3fn bytes) / xs uint8 [R, K/32] / row_flag uint8 [R]: the stored rows of x (R = T or P) by the rule of
//   mxa8_quantize_kernel (mxfp4_a8.hip)
//   y[p, n] = dt( sum_b 2^(xs[row(p), b] + scales[e, n, b] - 254) * (sum_{k in b} e4m3(xq) * e2m3(qweight)) + bias[e, n] ),  e = idx[p]
//   y[p, :] = NaN where row_flag[row(p)]; y[p, n] = NaN where e_col[e, n] == 255; y[p, :] = +0 where idx[p] is outside [0, E), whatever
//   the row's flag: the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone.  Every expert and
// row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E.
//
// Routed decode form (mx6m_decode_kernel, P <= 1024): mx_scaled_decode_pair (FP6 x E4M3) of mx_scaled_decode.cuh, in the operand order
// of mxfp6_a8.hip (profiles/mxfp6_a8_probe.txt): the weight fragment is A (FP6, cbsz 2; three non-temporal 8-byte pieces: a block is
// only 8-byte aligned), the x fragment B (E4M3, blgp 0, the two halves of a8_frag), byte select 0; a pair's row has the bits of the
// dense W6A8 decode form.  FUSED (one launch, K <= MX6M_ONE_K): the row image in LDS is written by mx_quantize_row, which
// mxa8_quantize_kernel calls too.
// Grouped prefill form: mxa8_quantize_kernel over the stored rows, mxm_route_kernel (mxfp4_moe.hip; the same workspace), then
// mx6m_gemm_kernel: mxm_tile_begin (mxfp4_common.cuh) and mx_scaled_gemm_tile (mx_scaled_tile.cuh; FP6 x E4M3) at 128 x 64.  A row tile belongs to one
// expert, gathers the xq / xs rows of its pairs through the pair list and reads weights from (long)e * N; rows past the segment enter
// as zero codes under scale code 127 and are not stored; the epilogue scatters row r to y[pair r].  The tiles of the skipped bin run no
// K loop and store zeros.
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// The largest K of the one-launch form: a row's image in LDS is the W4A8 expert kernel's (K bytes of codes and K / 32 scale bytes, 16896
// bytes at the bound), so its bound carries over.
constexpr int MX6M_ONE_K = 16384;
constexpr int MX6M_DECODE_PAIRS = 1024;  // the grid's second dimension

// A workgroup per pair and strip of 16 C16 columns of its expert (mx_scaled_decode_pair).  xin is x (FUSED) or the quantised rows.
template <int DT, int C16, bool FUSED>
__global__ __launch_bounds__(256) void mx6m_decode_kernel(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                          const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                          const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                          int N, int K, int x_per_pair) {
    mx_scaled_decode_pair<DT, C16, FUSED, mx_op_fp6, mx_op_e4m3, MX6M_ONE_K>(xin, xs, row_flag, idx, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair);
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
// 128 x 64: the routing's row tile fixes WM = 2; with WN = 1 the tile's two buffers and the pair list take 52224 bytes of LDS.  (The
// 128 x 128 instance's buffers alone are the 65536 bytes of static LDS; beside prow[] it would need 66048, which nothing in this
// library has launched.)
constexpr int MX6M_WM = 2, MX6M_WN = 1;
static_assert(64 * MX6M_WM == MXM_BM, "a row tile of the routing is a row tile of the GEMM");

// A workgroup per (row tile of the table, column tile): mx_scaled_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT>
__global__ __launch_bounds__(256) void mx6m_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                        const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                        const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                        int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, 64 * MX6M_WN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_scaled_gemm_tile<DT, MX6M_WM, MX6M_WN, mx_op_fp6, mx_op_e4m3>(mx_rows_listed{prow, S, x_per_pair}, xq, xs, row_flag, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MX6M_DECODE_PAIRS.  The plan started from the W4A8 expert layer's constants (decode for P <= 32,
// and up to 128 while P <= E) and was then measured (tools/mxfp6_moe_a8_bench.py, profiles/mxfp6_moe_a8_bench.jsonl, the `sweep` rows:
// both gpt-oss-20b projections at E = 32 and E = 128, fp16 and bf16, both forms forced at P = 1, 2, 4, ..., 1024, graph time, routings
// and weight stacks rotated; fp16 and bf16 agree within 2 % but for 12 of the 88 figures, all at P <= 8, up to 9 %: no verdict below turns on that).  The decode form streams an expert's
// weights once per pair, 1.5 x the W4A8 form's bytes, and grows linearly in P (9.8 / 23.3 / 81 / 157 / 311 / 619 us at
// P = 1 / 4 / 16 / 32 / 64 / 128 on 2880 -> 5760; the W4A8 form took 7.5 / 15.2 / 47 / 90 / 175 / 349); the grouped form costs 37 us at
// P = 1 (three launches, one row tile walking K) and then grows with the number of experts that hold a pair, on the narrower 128 x 64
// tile.  At E = 32 the decode form led at every P <= 16 (at most 0.75 x the grouped form's time); P = 32 was level on 2880 -> 5760
// (157.5 against 157.2 us in fp16, 157.9 against 158.3 in bf16) and ahead on 2880 -> 2880 (81 against 103 - 105); the grouped form led
// from P = 64 on (311 against 207, 158 against 109).  At E = 128, where nearly every pair of a small call has an expert of its own, the
// decode form led through P = 64 (308 against 341 - 348, 160 against 196 - 201) and the grouped form from P = 128 on (610 against
// 498 - 506, 315 - 317 against 282 - 295; 1.08 - 1.22 x).  So the plan takes the decode form for P <= 32, and up to P = 64 while
// 2 P <= E.  The second bound is narrower than the W4A8 layer's (128 while P <= E): the extra weight bytes are paid once per pair in
// the decode form and once per (expert, row tile) in the grouped one, so the crossover moved down; the W4A8 constants would lose
// 8 - 22 % at E = 128, P = 128.  E between 32 and 128 and beyond 128, and P between the powers of two, were not measured: the second
// clause extends the E = 128 rows by the pairs-per-expert argument (P = 64 at E = 128 is half a pair per expert; P = 32 at E = 32, one
// pair per expert, was level).  (The rows' `plan` column is the plan of the build that measured them, the W4A8 constants 32 / 128 /
// P <= E, which these rows replaced; the `accept` rows ran P = 4, 64, 1024 and 16384 at E = 32, where both plans choose alike.)
// The `accept` rows compare with the W4A8 expert layer on the same shapes, routings and activations (E = 32, S = 4, each arm one
// graph, alternated for 9 rounds, the W4A8 arm's spread 0.1 - 0.5 % but for one row at 6 %): T = 1 (decode) 1.52 - 1.56 x its time,
// above the 1.47 x of the weight bytes, as the dense W6A8 layer is at M = 1 (three 8-byte loads per lane and step); the grouped form
// 1.06 - 1.08 x on 2880 -> 2880 and 1.23 - 1.27 x on 2880 -> 5760 at T = 16 / 256, and 1.32 - 1.34 x at T = 4096 (450 / 377 against
// 602 / 499 TFLOP/s).  The expected cost was the weight bytes; the grouped form's rest is presumably the narrower tile (half the columns
// per staged x row) and the 24-byte fragment path that costs the dense layer 4 - 15 %.  Recorded, not gated; no counters were taken and
// the 128 x 128 tile was not launched.
// The strip width of the decode form: 16, 32 and 64 columns per workgroup measured at P = 1, 4, 16, 64 on both projections (the `strip`
// rows): 16 columns were ahead on every row (P = 1: 9.5 / 9.6 / 15.6 us at 5760 and 6.9 / 9.2 / 15.0 at 2880; P = 64: 311 / 327 / 336).
constexpr int MX6M_PLAN_PAIRS = 32, MX6M_PLAN_PAIRS_SPARSE = 64;
constexpr int MX6M_STRIP = 1;  // C16 of the decode form: strips of 16 columns (BIE_MXFP6_MOE_A8_STRIP = 1 / 2 / 4 under BIE_TUNING)

// Workspace of bie_mxfp6_moe_a8_forward, the W4A8 expert layer's: xq [R, K], xs [R, K/32], row_flag [R], then the routing region (mx_scaled_launch.cuh)
struct mx6m_layer {
    using act = mx_act_e4m3;
    static constexpr const char* form_knob = "BIE_MXFP6_MOE_A8_FORM";
    static constexpr const char* strip_knob = "BIE_MXFP6_MOE_A8_STRIP";
    static constexpr const char* wn_knob = nullptr;
    static constexpr int one_k = MX6M_ONE_K, decode_pairs = MX6M_DECODE_PAIRS;
    static constexpr int plan_pairs = MX6M_PLAN_PAIRS, plan_pairs_sparse = MX6M_PLAN_PAIRS_SPARSE, plan_sparse_mul = 2;
    static constexpr int strip = MX6M_STRIP, wn = MX6M_WN;
    static constexpr const char* decode_name = "mx6m_decode_kernel";
    static constexpr const char* gemm_name = "mx6m_gemm_kernel";
    template <int DT, int C16, bool FUSED> static constexpr auto decode() { return mx6m_decode_kernel<DT, C16, FUSED>; }
    template <int DT, int WN> static constexpr auto gemm() { return mx6m_gemm_kernel<DT>; }
};

bool mxfp6_moe_a8_decode_ok(long P) { return mx_grouped_decode_ok<mx6m_layer>(P); }
bool mxfp6_moe_a8_one_launch_ok(long K) { return mx_grouped_one_launch_ok<mx6m_layer>(K); }
int mxfp6_moe_a8_form(long P, long E, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_grouped_form<mx6m_layer>(P, E); }
size_t mxfp6_moe_a8_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_workspace_bytes<mx6m_layer>(T, S, E, K, x_per_pair, form);
}

int mxfp6_moe_a8_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                             const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair,
                             int dtype, int form, hipStream_t st) {
    return mx_grouped_gemm_launch<mx6m_layer>(xq, xs, row_flag, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

int mxfp6_moe_a8_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                                void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_grouped_forward_launch<mx6m_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
