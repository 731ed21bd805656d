// MXFP8 input gradient for gfx950: gx = gy . W straight from the packed E4M3 weights of mxfp8.hip / mxfp8_moe.hip (and mxfp8_a8.hip: the
// same bytes), for the backward of the MXFP8 weight-only layers (include/bie_hip.h, INTEGRATION.md "MXFP8 input gradient").  No
// reference implementation exists.
//
//   gx[m, k] = odt( sum_n gy[m, n] * W[n, k] ),  W[n, k] = e4m3(qweight[n, k]) * 2^(scales[n, k/32] - 127);  gy [M, N] fp16 / bf16, N arbitrary
//   products exact (a 16-bit significand times the 4 significant bits of E4M3), the sum in fp32 in an order fixed by N alone, one
//   rounding to odt (the dtype, or fp32 for the grouped form)
//
// This is the contract of mxfp4_grad.hip, and the rebias is that file's: e_blk[kb] = max_n scales[n, kb] (mx_blk_exp_kernel serves
// unchanged, the scale bytes are the same), fragments hold e4m3 * 2^(s[n, kb] - e_blk[kb]) <= 448, the fp32 epilogue multiplies column k
// by 2^(e_blk[k / 32] - 127), and a block-column with e_blk = 255 is NaN in every row of gx.  An E4M3 NaN code (0x7F / 0xFF) in W[n, k]
// converts to a NaN fragment element and makes column k NaN in every row, as a float product does.
//
// Neither sibling tile can be relabelled.  mx_dgrad_tile transposes single code BYTES and converts each byte (two k of one row) at that
// row's scale; an E4M3 byte is one k, and v_cvt_scalef32_pk_{f16,bf16}_fp8 converts two ADJACENT bytes under one scale, so a byte
// transpose would put two rows, with two scales, into one convert.  mx6_dgrad_tile leans on the one-instruction-per-block FP6 convert
// and pays for a 16-bit image in LDS.  The ways weighed for the weight operand (v_mfma_f32_32x32x16 wants a lane to hold 8 consecutive n
// of one output column k):
//   (a) the row-major packed tile in LDS, read with ds_read_b64_tr_b8: a lane then holds 8 rows of ONE k, which is 8 scales against a
//       two-bytes-one-scale convert: a scale-1.0 convert of four dwords plus 8 multiplies by the rows' scales, and bf16 has no packed
//       multiply (8 unpack / multiply / repack sequences per fragment);
//   (b) a 16-bit image [n][k] converted at staging time and read with ds_read_b64_tr_b16, the MXFP6 way: twice the LDS bytes of the
//       packed tile (16 KiB per 64 n x 128 k), which holds a stage to 32 n, and the image is rounded at the block-column's scale before
//       it is stored;
//   (c) transposing 16-bit UNITS of codes at staging time: the unit (p, n) = the two code bytes W[n, 2 p], W[n, 2 p + 1] is what one
//       convert takes under one scale, so LDS holds [k pair][n] and a lane's 8 rows of one k pair are one 16-byte read.
// mx8_dgrad_tile (mxfp8_common.cuh) takes (c): a staging thread loads one dword (two units) from each of eight consecutive rows,
// regroups them with eight v_perm_b32 and writes two ds_write_b128; the rebiased scales are staged as fp32 [block-column][n], so a
// lane's 8 scales are two 16-byte reads.  A dword of the fragment read holds rows 2 i (low half) and 2 i + 1 (high half); each half is
// one convert at its own row's scale, picked by op_sel.  Per 16-n step a lane issues 2 + 1 + 2 ds_read_b128 for 4 MFMAs, the tile stays
// packed in LDS (9 KiB per stage with the pad), no 16-bit image of W exists anywhere, and every code is converted by exactly one
// instruction at its own scale: the 8 first values and the 8 second values are the B fragments of two MFMAs (output columns 2 r and
// 2 r + 1), and the epilogue stores two adjacent columns per lane.
//
// The stage is 64 n: 18 KiB of gy, 9 KiB of codes and 1 KiB of scales per buffer, 56.1 KiB for the two buffers, which fits the 64 KiB of
// static LDS with the grouped kernel's prow[] (static_assert in mxfp8_common.cuh).  A 32-n stage would double the barriers per n (what
// mx6_dgrad_tile pays for its image) and leave a staging thread four rows per dword column, i.e. ds_write_b64 pairs whose bank pattern
// the 144-byte pitch does not spread; since 64 n fits, 32 n was not built.
//
// Precision range (the rebias is exact while the fragment is a normal number): the smallest E4M3 magnitude is 2^-9, so in fp16 a block
// whose scale code is up to 5 below its block-column's largest is held in normal numbers (2^-9 * 2^-5 = 2^-14, the smallest normal).
// From 6 to 15 below, the values are fp16 subnormals that are still exact (multiples of 2^-24); they are exact only as far as the
// convert returns them (profiles/mxfp8_cvt_probe.txt part (c)) and v_mfma_f32_32x32x16_f16 keeps them (profiles/mxfp6_grad_probe.txt).
// From 16 below bits are rounded away, and far enough below the block is zero.  In bf16 the normal range ends at 2^-9 * 2^-117 = 2^-126;
// mx_rebias gives scale 0 past 2^-126.  The tests stay inside e_blk - s <= 5.
//
// One form only (mx8_dgrad_kernel dense, mx8m_dgrad_kernel grouped): a backward call carries a whole batch, so there is no decode form;
// a small M is correct on the tile, not efficient.  The grouped kernel uses the routing workspace and launch of mxfp4_moe.hip as they
// are: a row tile belongs to one expert, gathers its gy rows by the pair list and scatters gx[pair]; the tiles of the skipped bin store
// +0 and run no loop.  Nothing synchronises with the host.
//
// Measured on an MI355X (tools/mxfp8_grad_bench.py, profiles/mxfp8_grad_bench.jsonl; graph time, medians, weight sets rotated past
// the Infinity Cache; fp16 and bf16 agree within 4 %), kernel time over (i) the layers' torch path (an fp32 image of W and mm, the only
// backward before this file) and (ii) mx6_dgrad_kernel on an FP6 weight of the same shape:
//   K -> N           M      kernel us   / torch   / mxfp6
//   4096 -> 4096      128     103         1.08      0.79      the kernel LOSES to the torch path at M = 128 on every dense shape:
//   4096 -> 4096     1024     110         0.41      0.82      one row tile is K / 128 = 23 or 32 workgroups for 256 CUs
//   4096 -> 4096     4096     238         0.25      0.89      (576 TFLOP/s)
//   4096 -> 11008     128     321         1.72      0.83
//   4096 -> 11008    1024     285         0.41      0.82
//   4096 -> 11008    4096     700         0.28      0.97
//   2880 -> 5760      128     146         1.25      0.81
//   2880 -> 5760     1024     151         0.53      0.82
//   2880 -> 5760     4096     305         0.29      1.44      it loses to the MXFP6 kernel here, and in the grouped form:
//   E = 32, top-4, T = 1024, 2880 -> 5760:   616   0.13 (eager torch loop)   1.14
//   E = 32, top-4, T = 1024, 2880 -> 2880:   325   0.10 (eager torch loop)   1.17
// Peak bytes of the backward at 4096 -> 11008, M = 1024: 8.4 MB against the torch path's 243 MB.  The 64-n choice rested on the LDS
// budget above, not on a 32-n measurement.  A first build formed every code load's 64-bit address from min(n, N - 1) * K per row and
// stage and was 1.3 .. 1.5 x slower than the figures above (VALU-bound beside the 32 converts per stage and lane); the whole stages now
// load through eight loop-invariant 32-bit offsets from a uniform row pointer, and only the last partial stage clamps.  Resources:
// profiles/mxfp8_grad_resources.txt (122 VGPRs + 64 AGPRs, no scratch, two waves per SIMD, 57472 / 57984 bytes of LDS).
#include "mxfp8_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

static_assert(MXM_BM == MX8_DG_BM, "a row tile of the routing is a row tile of mx8_dgrad_tile");

// ---- dense ------------------------------------------------------------------------------------------------------------------------------
// A workgroup per 128 x 128 tile of gx (mx8_dgrad_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx8_dgrad_kernel(const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                        const uint8_t* __restrict__ eblk, void* __restrict__ gx, int M, int N, int K, int tiles_k, int vec) {
    int tile_m, tile_k;
    pipe_tile(blockIdx.x, gridDim.x, tiles_k, BIE_PIPE_GM, tile_m, tile_k);
    mx8_dgrad_tile<DT, DT>(mx_rows_dense{tile_m * MX8_DG_BM, M}, gy, qw, sc, eblk, gx, 0L, tile_k * MX8_DG_BK, N, K, vec != 0);
}

// ---- grouped ----------------------------------------------------------------------------------------------------------------------------
// A workgroup per (row tile of the table, column tile of gx): mx8_dgrad_tile on the tile's pairs (gy [P, N], one row per pair) and the
// expert's rows of the [E * N, K] view, rebiased by the expert's K / 32 codes of e_blk.  The exit of mxm_tile_begin is
// workgroup-uniform: a workgroup that goes on has every lane of every wave in the tile body.
template <int DT, int ODT>
__global__ __launch_bounds__(256) void mx8m_dgrad_kernel(const uint16_t* __restrict__ gy, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                         const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, int E,
                                                         int N, int K, int vec, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, k0;
    if (!mxm_tile_begin<ODT, MX8_DG_BK>(ws, max_tiles, E, K, gx, prow, e, k0)) return;  // uniform
    mx8_dgrad_tile<DT, ODT>(mx_rows_listed{prow, 1, 1}, gy, qw, sc, eblk + (long)e * (K >> 5), gx, (long)e * N, k0, N, K, vec != 0);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
// the unit, for the host path of mx_w16_launch.cuh (the routing launch and its workspace layout are mxfp4_moe.hip's, shared as they are)
struct mx8_dgrad_unit {
    static constexpr int BM = MX8_DG_BM, BK = MX8_DG_BK;
    static constexpr const char *dense_name = "mx8_dgrad_kernel", *grouped_name = "mx8m_dgrad_kernel";
    template <int DT> static constexpr auto dense() { return mx8_dgrad_kernel<DT>; }
    template <int DT, int ODT> static constexpr auto grouped() { return mx8m_dgrad_kernel<DT, ODT>; }
};

int mxfp8_grad_input_launch(const void* gy, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, long M, long N, long K, int dtype,
                            hipStream_t st) {
    return mx_w16_grad_input_launch<mx8_dgrad_unit>(gy, qw, sc, eblk, gx, M, N, K, dtype, st);
}
int mxfp8_moe_grad_input_launch(const void* gy, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, void* workspace,
                                long P, long E, long N, long K, int dtype, int out_fp32, hipStream_t st) {
    return mx_w16_moe_grad_input_launch<mx8_dgrad_unit>(gy, idx, qw, sc, eblk, gx, workspace, P, E, N, K, dtype, out_fp32, st);
}

}  // namespace bie
