// MXFP4 W4A6 expert GEMM for gfx950: stacked MXFP4 expert weights (E2M1 elements, E8M0 block scales; the format of mxfp4_moe.hip per
// expert) against activations quantised to MXFP6 (E2M3 elements, E8M0 block scales) on the fly (mxfp6_a6.hip's xq6 / xs / row_flag),
// contracted on the block-scaled matrix instructions with an FP4 and an FP6 operand, at the FP4 matrix rate (include/bie_hip.h,
// INTEGRATION.md "MXFP4 W4A6 mixture-of-experts layer").  It is mxfp6_moe_a6.hip with the weight side of mxfp4_a6.hip.  No reference
// implementation exists.
//
//   T tokens, S slots per token, P = T * S pairs; pair p = t * S + s uses expert idx[p]; row(p) = p / S (x_per_pair = 0) or p
//   qweight uint8 [E, N, K/2]: per row K/32 blocks of 16 bytes, code j of a block in bits 4 j .. 4 j + 3 (the dense layer's bit order)
//   scales uint8 [E, N, K/32]; e_col uint8 [E, N] = bie_mxfp4_col_exp on the [E * N, K/32] view
//   xq6 uint8 [R, 3K/4] / xs uint8 [R, K/32] / row_flag uint8 [R]: the stored rows of x (R = T or P) by the rule of
//   mx6a6_quantize_kernel (mxfp6_a6.hip): 24-byte blocks, code j in bits 6 j .. 6 j + 5
//   y[p, n] = dt( sum_b 2^(xs[row(p), b] + scales[e, n, b] - 254) * (sum_{k in b} e2m3(xq6) * e2m1(qweight)) + bias[e, n] ),  e = idx[p]
//   y[p, :] = NaN where row_flag[row(p)]; y[p, n] = NaN where e_col[e, n] == 255; y[p, :] = +0 where idx[p] is outside [0, E), whatever
//   the row's flag: the index is compared before any address is formed from it
//
// A row of y is a function of its own pair only: in both forms a row's sum runs over K in an order fixed by K alone.  Every expert and
// row offset is 64-bit.  Nothing synchronises with the host: the grids are sized from P and E.
//
// Routed decode form (mx4m6_decode_kernel, P <= 1024): mx_scaled_decode_pair (FP4 x FP6) of mx_scaled_decode.cuh, with an FP4 A and
// an FP6 B operand (cbsz 4, blgp 2, byte select 0; profiles/mxfp4_a6_probe.txt): the weight fragment is one non-temporal 16-byte load,
// the x fragment the 24 bytes of its block; a pair's row has the bits of the dense W4A6 decode form (mxfp4_a6.hip).  FUSED (one launch,
// K <= MX4M6_ONE_K): the row image in LDS (3K/4 code bytes, K/32 scale bytes) is written by mx_quantize_row, which
// mx6a6_quantize_kernel calls too: the bits of bie_mxfp6_quantize_act.
// Grouped prefill form: mx6a6_quantize_kernel over the stored rows, mxm_route_kernel (mxfp4_moe.hip; the same workspace), then
// mx4m6_gemm_kernel: mxm_tile_begin (mxfp4_common.cuh) and mx_scaled_gemm_tile (mx_scaled_tile.cuh; FP4 x FP6) at 128 x 128 or 128 x 64.  A row tile
// belongs to one expert, gathers the xq6 / xs rows of its pairs through the pair list and reads weights from (long)e * N; rows past the
// segment enter as zero codes under scale code 127 and are not stored; the epilogue scatters row r to y[pair r].  The tiles of the
// skipped bin run no K loop and store zeros.
#include "mxfp6_common.cuh"
#include "mx_scaled_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

// ---- routed decode form -------------------------------------------------------------------------------------------------------------------
// The largest K of the one-launch form, the sibling expert kernels' bound.  A row's image in LDS is 3K/4 code bytes and K/32 scale
// bytes: 12800 bytes at the bound (the W4A8 expert kernel's image is K + K/32 = 16896).
constexpr int MX4M6_ONE_K = 16384;
constexpr int MX4M6_DECODE_PAIRS = 1024;  // the grid's second dimension

// A workgroup per pair and strip of 16 C16 columns of its expert (mx_scaled_decode_pair).  xin is x (FUSED) or the quantised rows.
template <int DT, int C16, bool FUSED>
__global__ __launch_bounds__(256) void mx4m6_decode_kernel(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                           const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                           const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                           int N, int K, int x_per_pair) {
    mx_scaled_decode_pair<DT, C16, FUSED, mx_op_fp4, mx_op_fp6, MX4M6_ONE_K>(xin, xs, row_flag, idx, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair);
}

// ---- grouped prefill form: the GEMM -------------------------------------------------------------------------------------------------------
// The routing's row tile fixes WM = 2.  A stage of mx_scaled_gemm_tile at WM = WN = 2 is 13312 bytes of x codes, 10240 of weight codes and
// 1024 of scale dwords: 49152 for the two buffers, 49664 beside the pair list (the W4A8 grouped tile stages 59392 bytes, the W6A6 one
// 55296).  WN = 1 (128 x 64): 2 (13312 + 5120 + 768) + 512 = 38912.
constexpr int MX4M6_WM = 2;
static_assert(64 * MX4M6_WM == MXM_BM, "a row tile of the routing is a row tile of the GEMM");
static_assert(2 * (64 * MX4M6_WM * mx_op_fp6::pitch(128) + 128 * mx_op_fp4::pitch(128) + (64 * MX4M6_WM + 128) * 4) + MXM_BM * 4 == 49664, "static LDS of the 128 x 128 instance");
static_assert(2 * (64 * MX4M6_WM * mx_op_fp6::pitch(128) + 64 * mx_op_fp4::pitch(128) + (64 * MX4M6_WM + 64) * 4) + MXM_BM * 4 == 38912, "static LDS of the 128 x 64 instance");
static_assert(49664 <= 65536, "static LDS");

// A workgroup per (row tile of the table, column tile): mx_scaled_gemm_tile on the tile's pairs and the expert's rows of the [E * N, K] view.
template <int DT, int WN>
__global__ __launch_bounds__(256) void mx4m6_gemm_kernel(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                         const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                         const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                         int N, int K, int x_per_pair, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, n0;
    if (!mxm_tile_begin<DT, 64 * WN>(ws, max_tiles, E, N, y, prow, e, n0)) return;  // uniform
    mx_scaled_gemm_tile<DT, MX4M6_WM, WN, mx_op_fp4, mx_op_fp6>(mx_rows_listed{prow, S, x_per_pair}, xq, xs, row_flag, qw, sc, ecol, bias, y, (long)e * N, n0, N, K);
}

// ---- plan and launchers -------------------------------------------------------------------------------------------------------------------
// The routed decode form exists for P <= MX4M6_DECODE_PAIRS.  The plan started from the W4A8 expert layer's constants (decode for
// P <= 32, and up to P = 128 while P <= E; mxfp4_moe_a8.hip) and was then measured (tools/mxfp4_moe_a6_bench.py,
// profiles/mxfp4_moe_a6_bench.jsonl, the `sweep` rows: both gpt-oss-20b projections at E = 32 and E = 128, fp16 and bf16, both forms
// forced at P = 1, 2, 4, ..., 1024, graph time, routings and weight stacks rotated, the grouped form on 128 x 128 tiles; fp16 and bf16
// agree within 2 % but for 9 of the 88 pairs of figures, up to 12 %: no verdict below turns on that).  The decode form grows linearly
// in P (8.7 / 15.8 / 47 / 88 / 170 / 337 us at P = 1 / 4 / 16 / 32 / 64 / 128 on 2880 -> 5760); the grouped form costs 42 us at P = 1
// and then grows with the number of experts that hold a pair.  At E = 32 the decode form led at every P <= 32 (P = 32: 88 against
// 140 - 147 us at 5760, 47 against 81 - 82 at 2880); P = 64 was split (170 against 168 at 5760: level; 88 - 89 against 103 at 2880:
// decode ahead) and the grouped form led from P = 128 on (337 against 170, 172 - 173 against 112 - 113).  At E = 128 the decode form
// led through P = 128 (P = 64: 169 against 270 - 272, 89 - 90 against 160 - 162; P = 128: 332 against 428 - 433, 173 - 174 against
// 225 - 226) and the grouped form from P = 256 on (657 - 658 against 542 - 556, 340 against 313 - 316).  Those are the W4A8 layer's
// crossovers, so the constants stay: they take the faster form on 86 of the 88 rows; the other two are 2880 -> 2880 at E = 32, P = 64
// (the grouped form taken, 103 us against the decode form's 88 - 89), where 2880 -> 5760 is level.  A first bound of 64 would take
// those two and lose 1 % on the level pair, but it would also hold for E < 32, which was not measured and where the grouped form has
// fewer experts to visit.  E between 32 and 128 and beyond 128, and P between the powers of two, were not measured.  The strip width
// of the decode form is the W4A8 layer's measured 16 columns; other widths were not measured here.
constexpr int MX4M6_PLAN_PAIRS = 32, MX4M6_PLAN_PAIRS_SPARSE = 128;
constexpr int MX4M6_STRIP = 1;  // C16 of the decode form
// The column tile of the grouped form, WN = 2 (128 x 128) or WN = 1 (128 x 64); BIE_MXFP4_MOE_A6_WN = 1 / 2 selects the instance and a
// row's bits do not depend on it.  Measured (the `tile` rows: T = 64, 256, 4096 at S = 4, both projections, E = 32 and E = 128, fp16 and
// bf16, the two widths captured as two graphs and alternated for 9 rounds, spread at most 0.9 %): 128 x 128 was ahead on 20 of the 24 rows
// (0.78 - 0.83 x the 128 x 64 time at T = 4096 on every shape; 0.89 - 0.95 x at T = 64 and 256 on 2880 -> 5760 and on 2880 -> 2880 with
// E = 128) and behind on 4 (2880 -> 2880, E = 32, T = 64 and 256: 1.10 - 1.14 x, 113 / 133 against 99 / 120 us, the rows on which the
// W6A6 expert layer's wide tile is behind as well).  The majority ships: 128 x 128.  A width chosen per call from max_tiles and N was
// not tried.
constexpr int MX4M6_WN = 2;

// Workspace of bie_mx4a6_moe_forward, the W6A6 expert layer's layout: xq6 [R, 3K/4], xs [R, K/32], row_flag [R], then the routing region (mx_scaled_launch.cuh)
struct mx4m6_layer {
    using act = mx_act_fp6;
    static constexpr const char* form_knob = "BIE_MXFP4_MOE_A6_FORM";
    static constexpr const char* strip_knob = nullptr;
    static constexpr const char* wn_knob = "BIE_MXFP4_MOE_A6_WN";
    static constexpr int one_k = MX4M6_ONE_K, decode_pairs = MX4M6_DECODE_PAIRS;
    static constexpr int plan_pairs = MX4M6_PLAN_PAIRS, plan_pairs_sparse = MX4M6_PLAN_PAIRS_SPARSE, plan_sparse_mul = 1;
    static constexpr int strip = MX4M6_STRIP, wn = MX4M6_WN;
    static constexpr const char* decode_name = "mx4m6_decode_kernel";
    static constexpr const char* gemm_name = "mx4m6_gemm_kernel";
    template <int DT, int C16, bool FUSED> static constexpr auto decode() { return mx4m6_decode_kernel<DT, C16, FUSED>; }
    template <int DT, int WN> static constexpr auto gemm() { return mx4m6_gemm_kernel<DT, WN>; }
};

bool mxfp4_moe_a6_decode_ok(long P) { return mx_grouped_decode_ok<mx4m6_layer>(P); }
bool mxfp4_moe_a6_one_launch_ok(long K) { return mx_grouped_one_launch_ok<mx4m6_layer>(K); }
int mxfp4_moe_a6_form(long P, long E, long N, long K, int dtype) { (void)N; (void)K; (void)dtype; return mx_grouped_form<mx4m6_layer>(P, E); }
size_t mxfp4_moe_a6_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_workspace_bytes<mx4m6_layer>(T, S, E, K, x_per_pair, form);
}

int mxfp4_moe_a6_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* row_flag, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                             const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair,
                             int dtype, int form, hipStream_t st) {
    return mx_grouped_gemm_launch<mx4m6_layer>(xq, xs, row_flag, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

int mxfp4_moe_a6_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                                void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    return mx_grouped_forward_launch<mx4m6_layer>(x, idx, qw, sc, ecol, bias, y, workspace, T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
