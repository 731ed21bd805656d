// MXFP6 W6A6 expert GEMM for gfx950: stacked MXFP6 expert weights (E2M3 elements, E8M0 block scales; the format of mxfp6_a8.hip per
// expert) against activations quantised to the SAME format on the fly (mxfp6_a6.hip's xq6 / xs / row_flag), contracted on the
// block-scaled matrix instructions with two FP6 operands (include/bie_hip.h, INTEGRATION.md "MXFP6 W6A6 mixture-of-experts layer").
// It is mxfp6_moe_a8.hip with the activation side of mxfp6_a6.hip.  No reference implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]; row(p) = p / S (x_per_pair = 0) or p
//   qweight uint8 [E, N, 3K/4]: per row K/32 blocks of 24 bytes, code j of a block in bits 6 j .. 6 j + 5 (the dense layer's bit order)
//   scales uint8 [E, N, K/32]; e_col uint8 [E, N] = bie_mxfp4_col_exp on the [E * N, K/32] view
//   xq6 uint8 [R, 3K/4] / xs uint8 [R, K/32] / row_flag uint8 [R]: the stored rows of x (R = T or P) by the rule of
//   mx6a6_quantize_kernel (mxfp6_a6.hip), in the weight's byte format
//   y[p, n] = dt( sum_b 2^(xs[row(p), b] + scales[e, n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m3(qweight)) + bias[e, n] ),  e = idx[p]
//   y[p, :] = NaN where row_flag[row(p)]; y[p, n] = NaN where e_col[e, n] == 255; y[p, :] = +0 where idx[p] is outside [0, E), whatever
//   the row's flag: the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone.  Every expert and
// row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E.
//
// Routed decode form (mx6m6_decode_kernel, P <= 1024): mx_scaled_decode_pair (FP6 x FP6) of mx_scaled_decode.cuh, with two FP6
// operands (cbsz 2, blgp 2, byte select 0; profiles/mxfp6_a6_probe.txt): the weight fragment is three non-temporal 8-byte pieces, the x
// fragment the same 24-byte copy of its block; a pair's row has the bits of the dense W6A6 decode form.  FUSED (one launch,
// K <= MX6M6_ONE_K): the row image in LDS (3K/4 code bytes, K/32 scale bytes) is written by mx_quantize_row, which
// mx6a6_quantize_kernel calls too: the bits of bie_mxfp6_quantize_act.
// Grouped prefill form: mx6a6_quantize_kernel over the stored rows, mxm_route_kernel (mxfp4_moe.hip; the same workspace), then
// mx6m6_gemm_kernel: mxm_tile_begin (mxfp4_common.cuh) and mx_scaled_gemm_tile (mx_scaled_tile.cuh; FP6 x FP6) at 128 x 128 or 128 x 64.  A row tile
// belongs to one expert, gathers the xq6 / xs rows of its pairs through the pair list and reads weights from (long)e * N; rows past the
// segment enter as zero codes under scale code 127 and are not stored; the epilogue scatters row r to y[pair r].  The tiles of the
// skipped bin run no K loop and store zeros.
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// The largest K of the one-launch form, the sibling expert kernels' bound.  A row's image in LDS is 3K/4 code bytes and K/32 scale
// bytes: 12800 bytes at the bound (the W6A8 expert kernel's image is K + K/32 = 16896).
constexpr int MX6M6_ONE_K = 16384;
constexpr int MX6M6_DECODE_PAIRS = 1024;  // the grid's second dimension

// A workgroup per pair and strip of 16 C16 columns of its expert (mx_scaled_decode_pair).  xin is x (FUSED) or the quantised rows.
template <int DT, int C16, bool FUSED>
__global__ __launch_bounds__(256) void mx6m6_decode_kernel(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                           const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                           int N, int K, int x_per_pair) {
    mx_scaled_decode_pair<DT, C16, FUSED, mx_op_fp6, mx_op_fp6, MX6M6_ONE_K>(xin, xs, row_flag, idx, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair);
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
// The routing's row tile fixes WM = 2.  Unlike the W6A8 grouped GEMM (mxfp6_moe_a8.hip, MX6M_WM) the 128 x 128 instance fits: a stage of
// mx_scaled_gemm_tile is 27648 bytes at WM = WN = 2, 55296 for the two buffers, 55808 beside the pair list.  WN = 1 (128 x 64) takes 41984.
constexpr int MX6M6_WM = 2;
static_assert(64 * MX6M6_WM == MXM_BM, "a row tile of the routing is a row tile of the GEMM");
static_assert(2 * ((64 * MX6M6_WM + 128) * mx_op_fp6::pitch(128) + (64 * MX6M6_WM + 128) * 4) + MXM_BM * 4 == 55808, "static LDS of the 128 x 128 instance");
static_assert(55808 <= 65536, "static LDS");

// A workgroup per (row tile of the table, column tile): mx_scaled_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT, int WN>
__global__ __launch_bounds__(256) void mx6m6_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                         int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, 64 * WN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_scaled_gemm_tile<DT, MX6M6_WM, WN, mx_op_fp6, mx_op_fp6>(mx_rows_listed{prow, S, x_per_pair}, xq, xs, row_flag, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MX6M6_DECODE_PAIRS.  The plan started from the W6A8 expert layer's constants (decode for
// P <= 32, and up to P = 64 while 2 P <= E; mxfp6_moe_a8.hip) and was then measured (tools/mxfp6_moe_a6_bench.py,
// profiles/mxfp6_moe_a6_bench.jsonl, the `sweep` rows: both gpt-oss-20b projections at E = 32 and E = 128, fp16 and bf16, both forms
// forced at P = 1, 2, 4, ..., 1024, graph time, routings and weight stacks rotated, the grouped form on 128 x 128 tiles; fp16 and bf16
// agree within 2 % but for 8 of the 88 pairs of figures, up to 9 %: no verdict below turns on that).  The decode form grows linearly in P (10.6 /
// 24.5 / 82 / 158 / 311 / 618 us at P = 1 / 4 / 16 / 32 / 64 / 128 on 2880 -> 5760; the W6A8 form took 9.8 / 23.3 / 81 / 157 / 311 / 619);
// the grouped form costs 47 us at P = 1 and then grows with the number of experts that hold a pair.  At E = 32 the decode form led at
// every P <= 32 (0.93 x the grouped form's time at P = 32 on 2880 -> 5760, 158 against 170 - 171 us; 0.80 - 0.85 x on 2880 -> 2880, 82
// against 97 - 103) and the grouped form from P = 64 on (311 against 196, 159 against 132).  At E = 128 the decode form led through
// P = 32 (160 against 195, 83 against 129 - 130), was level or ahead at P = 64 (313 - 315 against 319, 161 against 193) and behind from
// P = 128 on (628 - 629 against 499 - 505, 317 against 257 - 276).  So the measured crossovers are where the W6A8 layer's are and the constants
// stay: the decode form for P <= 32, and up to P = 64 while 2 P <= E.  E between 32 and 128 and beyond 128, and P between the powers of
// two, were not measured.  The strip width of the decode form is the W6A8 layer's measured 16 columns; other widths were not measured here.
constexpr int MX6M6_PLAN_PAIRS = 32, MX6M6_PLAN_PAIRS_SPARSE = 64;
constexpr int MX6M6_STRIP = 1;  // C16 of the decode form
// The column tile of the grouped form, WN = 2 (128 x 128) or WN = 1 (128 x 64); BIE_MXFP6_MOE_A6_WN = 1 / 2 selects the instance and a
// row's bits do not depend on it.  Measured (the `tile` rows: T = 64, 256, 4096 at S = 4, both projections, E = 32 and E = 128, fp16 and
// bf16, the two widths captured as two graphs and alternated for 9 rounds, spread at most 0.7 %): 128 x 128 was ahead on 18 of the 24 rows
// (0.79 - 0.84 x the 128 x 64 time at T = 4096 on every shape; 0.92 - 0.95 x at T = 64 and 256 on 2880 -> 5760 and at T = 256 on
// 2880 -> 2880 with E = 128), level on 2 (2880 -> 2880, E = 128, T = 64: 1.00 / 1.01 x) and behind on 4 (2880 -> 2880, E = 32, T = 64
// and 256: 1.13 - 1.16 x, 136 / 156 against 117 / 138 us: 23 column tiles of 128 for about 32 live row tiles do not fill the card's second
// round of workgroups).  The majority ships: 128 x 128.  A width chosen per call from max_tiles and N was not tried.
constexpr int MX6M6_WN = 2;

// Workspace of bie_mxfp6_moe_a6_forward: xq6 [R, 3K/4], xs [R, K/32], row_flag [R], then the routing region (mx_scaled_launch.cuh)
struct mx6m6_layer {
    using act = mx_act_fp6;
    static constexpr const char* form_knob = "BIE_MXFP6_MOE_A6_FORM";
    static constexpr const char* strip_knob = nullptr;
    static constexpr const char* wn_knob = "BIE_MXFP6_MOE_A6_WN";
    static constexpr int one_k = MX6M6_ONE_K, decode_pairs = MX6M6_DECODE_PAIRS;
    static constexpr int plan_pairs = MX6M6_PLAN_PAIRS, plan_pairs_sparse = MX6M6_PLAN_PAIRS_SPARSE, plan_sparse_mul = 2;
    static constexpr int strip = MX6M6_STRIP, wn = MX6M6_WN;
    static constexpr const char* decode_name = "mx6m6_decode_kernel";
    static constexpr const char* gemm_name = "mx6m6_gemm_kernel";
    template <int DT, int C16, bool FUSED> static constexpr auto decode() { return mx6m6_decode_kernel<DT, C16, FUSED>; }
    template <int DT, int WN> static constexpr auto gemm() { return mx6m6_gemm_kernel<DT, WN>; }
};

bool mxfp6_moe_a6_decode_ok(long P) { return mx_grouped_decode_ok<mx6m6_layer>(P); }
bool mxfp6_moe_a6_one_launch_ok(long K) { return mx_grouped_one_launch_ok<mx6m6_layer>(K); }
int mxfp6_moe_a6_form(long P, long E, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_grouped_form<mx6m6_layer>(P, E); }
size_t mxfp6_moe_a6_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_workspace_bytes<mx6m6_layer>(T, S, E, K, x_per_pair, form);
}

int mxfp6_moe_a6_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                             const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair,
                             int dtype, int form, hipStream_t st) {
    return mx_grouped_gemm_launch<mx6m6_layer>(xq, xs, row_flag, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

int mxfp6_moe_a6_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                                void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_grouped_forward_launch<mx6m6_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
