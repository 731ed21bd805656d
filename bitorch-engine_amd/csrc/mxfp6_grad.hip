// MXFP6 input gradient for gfx950: gx = gy . W straight from the packed weights of mxfp6_a8.hip / mxfp6_moe_a8.hip, for the backward of
// the MXFP6 layers (include/bie_hip.h, INTEGRATION.md "MXFP6 input gradient").  No reference implementation exists.
//
//   gx[m, k] = odt( sum_n gy[m, n] * W[n, k] ),  W[n, k] = e2m3(code) * 2^(scales[n, k/32] - 127);  gy [M, N] fp16 / bf16, N arbitrary
//   products exact (a 16-bit significand times the 4 bits of E2M3), the sum in fp32 in an order fixed by N alone, one rounding to odt
//   (the dtype, or fp32 for the grouped form)
//
// This is the contract of mxfp4_grad.hip, and the rebias is that file's: e_blk[kb] = max_n scales[n, kb] (mx_blk_exp_kernel serves
// unchanged, the scale bytes are the same), fragments hold e2m3 * 2^(s[n, kb] - e_blk[kb]) <= 7.5, the fp32 epilogue multiplies column k
// by 2^(e_blk[k / 32] - 127), and a block-column with e_blk = 255 is NaN in every row of gx.
//
// It is not mx_dgrad_tile with another convert.  That tile transposes code BYTES (a byte holds two codes of one row) and converts a byte
// at a time at its own row's scale.  E2M3 codes straddle bytes (four codes in three bytes), and the only FP6 converts of gfx950 are
// v_cvt_scalef32_pk32_{bf16,f16}_fp6: six registers, the 32 codes of one block ALONG k, to 32 values under one scale.  So the convert has
// to run before the transpose.  The ways weighed for the weight operand (v_mfma_f32_32x32x16 wants a lane to hold 8 consecutive n of one
// output column k):
//   (a) the packed tile in LDS as the forward stages it, every lane of a 16-n step unpacking 8 six-bit codes of 8 rows with shifts and a
//       table or integer arithmetic instead of the convert: 8 unaligned bit-field reads and 8 scale reads per fragment, and the convert
//       instruction unused;
//   (b) converting a block per lane after the LDS read and transposing 32 x 32 values between lanes (permutes or a second LDS round
//       trip): the converted data crosses lanes anyway, at 16-bit width, and every wave of a column repeats the converts;
//   (c) converting at staging time, ONE convert per block at the block's own rebiased scale, writing a 16-bit image [n][k] to LDS and
//       reading the B fragments back with ds_read_b64_tr_b16, the hardware's transposed read.
// mx6_dgrad_tile (mxfp6_common.cuh) takes (c): every block of qweight is converted exactly once per tile by exactly one instruction,
// the transpose costs no VALU work, and a fragment is two 8-byte LDS reads (4 per 16-n step and wave beside the 2 ds_read_b128 of gy,
// for 4 MFMAs).  The price is LDS: the image is 4 x the packed codes' bytes (8 KiB per 32 n x 128 k), which with the gy tile holds a
// stage to 32 n where mx_dgrad_tile has 64 (two buffers of a 64-n stage would pass the 64 KiB of static LDS); a stage is 18 KiB and the
// two buffers 36 KiB.  So there are twice the barriers per n of mx_dgrad_tile, and the 16-bit image is written and read where that tile
// moves packed bytes.
//
// Precision range (the rebias is exact while the fragment is a normal number): the smallest E2M3 magnitude is 2^-3, so in fp16 a block
// whose scale code is up to 11 below its block-column's largest is held in normal numbers (2^-3 * 2^-11 = 2^-14, the smallest normal).
// From 12 to 21 below, the values are fp16 subnormals that are still exact (multiples of 2^-24); the convert returns them and
// v_mfma_f32_32x32x16_f16 keeps them (tools/probe/probe_fp6_cvt.hip parts (c), (d), profiles/mxfp6_grad_probe.txt).  From 22 below the
// convert rounds bits away (to nearest even), from 28 below the block is zero.  In bf16 the normal range ends at 2^-3 * 2^-123 = 2^-126;
// the convert keeps bf16 subnormals too, the bf16 MFMA was not probed (124 .. 126 below: unspecified), and mx_rebias gives scale 0
// past 2^-126.  The tests stay inside e_blk - s <= 11.
//
// One form only (mx6_dgrad_kernel dense, mx6m_dgrad_kernel grouped): a small M is correct on the tile, not efficient.  The grouped
// kernel uses the routing workspace and launch of mxfp4_moe.hip as they are: a row tile belongs to one expert, gathers its gy rows by
// the pair list and scatters gx[pair]; the tiles of the skipped bin store zeros and run no loop.  Nothing synchronises with the host.
#include "mxfp6_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

static_assert(MXM_BM == MX6_DG_BM, "a row tile of the routing is a row tile of mx6_dgrad_tile");

// ---- dense ------------------------------------------------------------------------------------------------------------------------------
// A workgroup per 128 x 128 tile of gx (mx6_dgrad_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx6_dgrad_kernel(const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                        const uint8_t* __restrict__ eblk, void* __restrict__ gx, int M, int N, int K, int tiles_k, int vec) {
    int tile_m, tile_k;
    pipe_tile(blockIdx.x, gridDim.x, tiles_k, BIE_PIPE_GM, tile_m, tile_k);
    mx6_dgrad_tile<DT, DT>(mx_rows_dense{tile_m * MX6_DG_BM, M}, gy, qw, sc, eblk, gx, 0L, tile_k * MX6_DG_BK, N, K, vec != 0);
}

// ---- grouped ----------------------------------------------------------------------------------------------------------------------------
// A workgroup per (row tile of the table, column tile of gx): mx6_dgrad_tile on the tile's pairs (gy [P, N], one row per pair) and the
// expert's rows of the [E * N, 3K/4] view, rebiased by the expert's K / 32 codes of e_blk.  The exit of mxm_tile_begin is
// workgroup-uniform: a workgroup that goes on has every lane of every wave in the tile body.
template <int DT, int ODT>
__global__ __launch_bounds__(256) void mx6m_dgrad_kernel(const uint16_t* __restrict__ gy, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                         const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, int E,
                                                         int N, int K, int vec, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, k0;
    if (!mxm_tile_begin<ODT, MX6_DG_BK>(ws, max_tiles, E, K, gx, prow, e, k0)) return;  // uniform
    mx6_dgrad_tile<DT, ODT>(mx_rows_listed{prow, 1, 1}, gy, qw, sc, eblk + (long)e * (K >> 5), gx, (long)e * N, k0, N, K, vec != 0);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
// the unit, for the host path of mx_w16_launch.cuh (the routing launch and its workspace layout are mxfp4_moe.hip's, shared as they are)
struct mx6_dgrad_unit {
    static constexpr int BM = MX6_DG_BM, BK = MX6_DG_BK;
    static constexpr const char *dense_name = "mx6_dgrad_kernel", *grouped_name = "mx6m_dgrad_kernel";
    template <int DT> static constexpr auto dense() { return mx6_dgrad_kernel<DT>; }
    template <int DT, int ODT> static constexpr auto grouped() { return mx6m_dgrad_kernel<DT, ODT>; }
};

int mxfp6_grad_input_launch(const void* gy, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, long M, long N, long K, int dtype,
                            hipStream_t st) {
    return mx_w16_grad_input_launch<mx6_dgrad_unit>(gy, qw, sc, eblk, gx, M, N, K, dtype, st);
}
int mxfp6_moe_grad_input_launch(const void* gy, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, void* workspace,
                                long P, long E, long N, long K, int dtype, int out_fp32, hipStream_t st) {
    return mx_w16_moe_grad_input_launch<mx6_dgrad_unit>(gy, idx, qw, sc, eblk, gx, workspace, P, E, N, K, dtype, out_fp32, st);
}

}  // namespace bie
