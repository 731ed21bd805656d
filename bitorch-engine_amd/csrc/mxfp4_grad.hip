// MXFP4 input gradient for gfx950: gx = gy . W straight from the packed weights of mxfp4.hip / mxfp4_moe.hip, for the backward of the
// MXFP4 layers (include/bie_hip.h, INTEGRATION.md "MXFP4 input gradient").  No reference implementation exists.
//
//   gx[m, k] = odt( sum_n gy[m, n] * W[n, k] ),  W[n, k] = e2m1(code) * 2^(scales[n, k/32] - 127);  gy [M, N] fp16 / bf16, N arbitrary
//   products exact, the sum in fp32 in an order fixed by N alone, one rounding to odt (the dtype, or fp32 for the grouped form)
//
// This is not the forward with its arguments swapped: the contraction runs over n, while qweight is packed along k (two k per byte)
// and scales[n, k/32] varies along the contraction and the output column together.
//
// The weight operand's transpose.  v_mfma_f32_32x32x16_{bf16,f16} wants a lane to hold 8 consecutive contraction values of one output
// column; here those are 8 nibbles from 8 rows of qweight.  Three ways were weighed:
//   (a) stage the packed tile as the forward does ([n][32 code bytes]) and let lane (r, h) read the 8 bytes at byte column r of rows
//       8 h .. + 7: 8 one-byte LDS reads and 8 one-dword scale reads per 16-n step and lane, 64 per stage against 16 MFMAs;
//   (b) write a converted 16-bit image to LDS and read it with ds_read_b64_tr_b16: 4 x the LDS bytes of the packed tile, the converts
//       before the LDS write, and the image is rounded at a scale that must already be the block-column's;
//   (c) transpose the bytes at staging time, so that LDS holds [byte column][n] and a lane's 8 rows are one 8-byte read.
// mx_dgrad_tile (mxfp4_common.cuh) takes (c): the staging thread loads one dword from each of four consecutive rows, transposes the
// 4 x 4 bytes in registers and writes four dwords; the rebiased scales are staged as fp32 [block-column][n], so a lane's 8 scales are
// two 16-byte reads.  Per 16-n step a lane then issues 2 + 1 + 2 LDS reads for 4 MFMAs, the tile stays packed in LDS (4.5 KiB per stage),
// and every byte still takes exactly one v_cvt_scalef32_pk_{bf16,f16}_fp4 at its own row's scale: a byte is the two adjacent output
// columns 2 r, 2 r + 1, the 8 low halves and the 8 high halves are the B fragments of two MFMAs, and the epilogue stores two adjacent
// columns per lane.
//
// The rebias is per block-column: e_blk[kb] = max_n scales[n, kb] (255 where a block of the block-column has scale code 255;
// mx_blk_exp_kernel, one pass over N * K / 32 bytes).  Fragments hold e2m1 * 2^(s[n, kb] - e_blk[kb]) <= 6 and the fp32 epilogue
// multiplies column k by 2^(e_blk[k / 32] - 127).  A block-column with e_blk = 255 is NaN in every row of gx, as a float product with a
// NaN weight is.  In fp16 a block more than 2^14 below its block-column's largest scale loses bits and one more than 2^24 below it
// flushes to zero; in bf16 the flush is at 2^126 below.
//
// One form only (mx_dgrad_kernel dense, mxm_dgrad_kernel grouped): a backward call carries a whole batch, so there is no decode form;
// a small M is correct on the tile, just not efficient.  The grouped kernel uses the routing workspace and launch of mxfp4_moe.hip as
// they are: a row tile belongs to one expert, gathers its gy rows by the pair list and scatters gx[pair]; the tiles of the skipped bin
// store zeros and run no loop.  Nothing synchronises with the host.
#include "mxfp4_common.cuh"
#include "mx_w16_launch.cuh"

#pragma clang fp contract(off)

namespace bie {

static_assert(MXM_BM == MX_DG_BM, "a row tile of the routing is a row tile of mx_dgrad_tile");

// ---- block-column exponent --------------------------------------------------------------------------------------------------------------
// e_blk[g, kb] = the largest scale code of block-column kb over the `rows` rows of group g (255 is the largest code, so a NaN block
// gives 255).  Workgroup: 4 block-columns (blockIdx.x) of one group (blockIdx.y), 64 threads per block-column striding the rows.
__global__ __launch_bounds__(256) void mx_blk_exp_kernel(const uint8_t* __restrict__ sc, uint8_t* __restrict__ eblk, int rows, int KB) {
    __shared__ uint32_t red[4][64];
    const int c = threadIdx.x & 3, q = threadIdx.x >> 2, kb = blockIdx.x * 4 + c;
    const uint8_t* src = sc + (long)blockIdx.y * rows * KB;
    uint32_t e = 0u;
    if (kb < KB)
        for (int n = q; n < rows; n += 64) e = max(e, (uint32_t)src[(long)n * KB + kb]);
    red[c][q] = e;
    __syncthreads();
    if (threadIdx.x < 4 && blockIdx.x * 4 + (int)threadIdx.x < KB) {
        uint32_t m = 0u;
        for (int i = 0; i < 64; i++) m = max(m, red[threadIdx.x][i]);
        eblk[(long)blockIdx.y * KB + blockIdx.x * 4 + threadIdx.x] = (uint8_t)m;
    }
}

// ---- dense ------------------------------------------------------------------------------------------------------------------------------
// A workgroup per 128 x 128 tile of gx (mx_dgrad_tile), the tiles walked in pipe_tile's order.
template <int DT>
__global__ __launch_bounds__(256) void mx_dgrad_kernel(const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                       const uint8_t* __restrict__ eblk, void* __restrict__ gx, int M, int N, int K, int tiles_k, int vec) {
    int tile_m, tile_k;
    pipe_tile(blockIdx.x, gridDim.x, tiles_k, BIE_PIPE_GM, tile_m, tile_k);
    mx_dgrad_tile<DT, DT>(mx_rows_dense{tile_m * MX_DG_BM, M}, gy, qw, sc, eblk, gx, 0L, tile_k * MX_DG_BK, N, K, vec != 0);
}

// ---- grouped ----------------------------------------------------------------------------------------------------------------------------
// A workgroup per (row tile of the table, column tile of gx): mx_dgrad_tile on the tile's pairs (gy [P, N], one row per pair) and the
// expert's rows of the [E * N, K] view, rebiased by the expert's K / 32 codes of e_blk.
template <int DT, int ODT>
__global__ __launch_bounds__(256) void mxm_dgrad_kernel(const uint16_t* __restrict__ gy, const int32_t* __restrict__ ws, const uint8_t* __restrict__ qw,
                                                        const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, int E,
                                                        int N, int K, int vec, int max_tiles) {
    __shared__ int prow[MXM_BM];
    int e, k0;
    if (!mxm_tile_begin<ODT, MX_DG_BK>(ws, max_tiles, E, K, gx, prow, e, k0)) return;  // uniform
    mx_dgrad_tile<DT, ODT>(mx_rows_listed{prow, 1, 1}, gy, qw, sc, eblk + (long)e * (K >> 5), gx, (long)e * N, k0, N, K, vec != 0);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
int mxfp4_blk_exp_launch(const uint8_t* sc, uint8_t* eblk, long rows, long K, long groups, hipStream_t st) {
    const long KB = K / 32;
    hipLaunchKernelGGL(mx_blk_exp_kernel, dim3((unsigned)cdivl(KB, 4), (unsigned)groups), dim3(256), 0, st, sc, eblk, (int)rows, (int)KB);
    return check_launch("mx_blk_exp_kernel");
}

// the unit, for the host path of mx_w16_launch.cuh (the routing launch and its workspace layout are mxfp4_moe.hip's, shared as they are)
struct mx4_dgrad_unit {
    static constexpr int BM = MX_DG_BM, BK = MX_DG_BK;
    static constexpr const char *dense_name = "mx_dgrad_kernel", *grouped_name = "mxm_dgrad_kernel";
    template <int DT> static constexpr auto dense() { return mx_dgrad_kernel<DT>; }
    template <int DT, int ODT> static constexpr auto grouped() { return mxm_dgrad_kernel<DT, ODT>; }
};

int mxfp4_grad_input_launch(const void* gy, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, long M, long N, long K, int dtype,
                            hipStream_t st) {
    return mx_w16_grad_input_launch<mx4_dgrad_unit>(gy, qw, sc, eblk, gx, M, N, K, dtype, st);
}
int mxfp4_moe_grad_input_launch(const void* gy, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, void* workspace,
                                long P, long E, long N, long K, int dtype, int out_fp32, hipStream_t st) {
    return mx_w16_moe_grad_input_launch<mx4_dgrad_unit>(gy, idx, qw, sc, eblk, gx, workspace, P, E, N, K, dtype, out_fp32, st);
}

}  // namespace bie
