// The MXFP6 (OCP microscaling FP6, E2M3 elements) format's device-side rules (gfx950): the quantiser's rounding rule, code <-> fp32,
// a block's 24 bytes <-> its 32 codes, the input-gradient 128 x 128 tile body (mx6_dgrad_tile: the kernels of mxfp6_grad.hip), the
// weight-only (W6A16) 128 x 128 tile body (mx6_gemm_tile: mx6_gemm_kernel of mxfp6.hip) and the MXFP6 activation quantiser's unit and
// row (a6_quantize_unit, mx_quantize_row: the kernels of mxfp6_a6.hip, mxfp6_moe_a6.hip and mxfp4_moe_a6.hip).  The E8M0 block scales, the block-scale rule (mx_block_scale:
// emax = 2 for E2M3 as for E2M1), the row sources and the MXFP8 activations are those of mxfp4_common.cuh / mxfp4_a8_common.cuh; the
// FP6 operand of the block-scaled matrix instructions (a6_frag, mx_op_fp6) and the prefill tile body of the W6A8, W6A6 and W4A6 units
// are those of mx_scaled_tile.cuh.
//
// A block of 32 codes is 24 bytes: code j in bits 6 j .. 6 j + 5 of the block's little-endian 192-bit integer, which is the order in
// which the instructions read a lane's six operand registers (tools/probe/probe_mx_fp6.hip part (a2), profiles/mxfp6_a8_probe.txt), so
// a lane's fragment is a plain 24-byte copy.  Code bits: bit 5 sign, bits 4:3 exponent (bias 1), bits 2:0 mantissa; no Inf / NaN code.
#pragma once
#include <type_traits>
#include "mxfp4_a8_common.cuh"

namespace bie {

constexpr int MX6_BLOCK_BYTES = mx_op_fp6::BLOCK;  // 24

// |a| <= 7.5 -> E2M3 magnitude code 0 .. 31, round to nearest, ties to the even code.  The codes are linear in each of three ranges:
// 0 .. 16 = a * 8 on [0, 2] (subnormals and the first binade share the step 0.125), 16 .. 24 = a * 4 + 8 on [2, 4], 24 .. 31 = a * 2 + 16
// on [4, 7.5]; the offsets are even, so rint's ties-to-even on the scaled value is ties-to-even on the code, and a tie at the top of a
// range lands on the next range's first (even) code (1.9375 -> 2.0).  The multiplies are by powers of two: exact.
__device__ __forceinline__ uint32_t mx6_round_e2m3(float a) {
    return a < 2.0f ? (uint32_t)__builtin_rintf(a * 8.0f) : a < 4.0f ? (uint32_t)__builtin_rintf(a * 4.0f) + 8u : (uint32_t)__builtin_rintf(a * 2.0f) + 16u;
}

// code (6 bits; higher bits ignored) -> fp32, exact; the sign bit is kept on zero
__device__ __forceinline__ float mx6_e2m3(uint32_t c) {
    const uint32_t m = c & 31u;
    const float mag = m < 16u ? (float)m * 0.125f : m < 24u ? (float)(m - 8u) * 0.25f : (float)(m - 16u) * 0.5f;
    return __uint_as_float(__float_as_uint(mag) | ((c & 32u) << 26));
}

// a block's 24 bytes as three little-endian 64-bit words <-> its 32 codes
__device__ __forceinline__ void mx6_pack(const uint32_t (&c)[32], uint64_t (&w)[3]) {
    w[0] = w[1] = w[2] = 0ull;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int bit = 6 * j, i = bit >> 6, o = bit & 63;
        w[i] |= (uint64_t)c[j] << o;
        if (o > 58) w[i + 1] |= (uint64_t)c[j] >> (64 - o);
    }
}
__device__ __forceinline__ uint32_t mx6_code(const uint64_t (&w)[3], int j) {
    const int bit = 6 * j, i = bit >> 6, o = bit & 63;
    uint64_t v = w[i] >> o;
    if (o > 58) v |= w[i + 1] << (64 - o);
    return (uint32_t)v & 63u;
}

// ---- the MXFP6 activation quantiser's unit ----------------------------------------------------------------------------------------------------
// One 8-value unit (16 bytes of x) of a block of 32 whose four units sit on the four lanes of a quad, for the MXFP6 activation quantiser
// (mx6a6_quantize_kernel of mxfp6_a6.hip): the block maximum over the quad on the DPP network, the block's E8M0 code (mx_block_scale, the
// weight quantiser's) and this lane's eight E2M3 codes by exactly mx6_quantize_kernel's expression, code i in bits 6 i .. 6 i + 5 of the
// 48-bit result.  An all-zero block: scale code 0, codes 0.  `bad` collects a NaN or +-inf.  All lanes of the quad must call it together.
template <int DT>
__device__ __forceinline__ void a6_quantize_unit(const uint4_t& raw, int& bad, uint64_t& codes, uint32_t& scode) {
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if constexpr (DT == BIE_F16) {
            v[2 * i] = f16_bits_to_f32(w[i] & 0xffffu);
            v[2 * i + 1] = f16_bits_to_f32(w[i] >> 16);
        } else {
            v[2 * i] = bf16_bits_to_f32(w[i] & 0xffffu);
            v[2 * i + 1] = bf16_bits_to_f32(w[i] >> 16);
        }
    }
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        amax = fmaxf(amax, fabsf(v[i]));
        bad |= (__float_as_uint(v[i]) & 0x7f800000u) == 0x7f800000u;
    }
    amax = a4_dpp_max<0xB1>(amax);  // quad_perm [1, 0, 3, 2]
    amax = a4_dpp_max<0x4E>(amax);  // quad_perm [2, 3, 0, 1]
    codes = 0ull;
    scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mx_block_scale(amax, inv);
#pragma unroll
        for (int i = 0; i < 8; i++)
            codes |= (uint64_t)(mx6_round_e2m3(fminf(fabsf(v[i] * inv), 7.5f)) | ((__float_as_uint(v[i]) >> 26) & 32u)) << (6 * i);
    }
}

// A row of x to MXFP6 (mx_quantize_row of mx_scaled_decode.cuh).  Lane q of a quad holds bits 48 q .. 48 q + 47 of its block's 192; the
// block's 8-byte word i is (c_i >> 16 i) | (c_(i+1) << (48 - 16 i)): lane i < 3 takes its right neighbour's 48 bits over the DPP network
// and stores word i, 24 contiguous bytes per quad; lane 0 stores the scale byte.  U = K / 8 is a multiple of 4 and the stride is 256:
// whole quads are in or out, so the quad's exchanges are complete.
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_fp6, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad) {
    const int U = K >> 3;
    for (int u = threadIdx.x; u < U; u += 256) {
        uint64_t c;
        uint32_t scode;
        a6_quantize_unit<DT>(*reinterpret_cast<const uint4_t*>(xr + (long)u * 8), bad, c, scode);
        // the right neighbour's codes: quad_perm [1, 2, 3, 0]
        const uint32_t nlo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)c, 0x39, 0xf, 0xf, false);
        const uint32_t nhi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(c >> 32), 0x39, 0xf, 0xf, false);
        const uint64_t nb = (uint64_t)nlo | ((uint64_t)nhi << 32);
        const int q = u & 3;
        if (q < 3) {
            const uint64_t word = (c >> (16 * q)) | (nb << (48 - 16 * q));
            *reinterpret_cast<uint2_t*>(codes + (long)(u >> 2) * MX6_BLOCK_BYTES + q * 8) = uint2_t{(uint32_t)word, (uint32_t)(word >> 32)};
        }
        if (q == 0) scales[u >> 2] = (uint8_t)scode;
    }
}

// ---- the input-gradient tile -----------------------------------------------------------------------------------------------------------------
constexpr int MX6_DG_BM = 128, MX6_DG_BK = 128, MX6_DG_BN = 32;  // rows of gy, columns k of gx, contraction rows n of a stage
constexpr int MX6_DG_APITCH = MX6_DG_BN * 2 + 16;                // bytes per gy row in LDS (MX_APITCH's pad)
constexpr int MX6_DG_WPITCH = MX6_DG_BK * 2;                     // bytes per weight row n of the 16-bit image [n][k]
constexpr int MX6_DG_STAGE = MX6_DG_BM * MX6_DG_APITCH + MX6_DG_BN * MX6_DG_WPITCH;  // 10240 + 8192

// The 16-bit weight image of a stage: [32 n][128 k], 256-byte rows, the 16-byte chunk ch (8 k) of row n stored at chunk
// ch ^ (((n & 3) << 2) | ((n >> 2) & 3)).  Every chunk stays whole and 16-byte aligned, so a lane's 8-byte transposed read (4 contiguous
// k of one row) is 8-byte aligned and inside one chunk.  Banks, by the (a / 4) mod 64 rule (a row is 64 dwords, so the bank is 4 * the
// stored chunk + the dword in it):
//   transposed read (ds_read_b64_tr_b16, served per 32 lanes): a half-wave reads rows n = 4 c + q (q = 0 .. 3, c = (n >> 2) fixed) and the
//     four chunks ch = 4 a + b (b = 0 .. 3, a fixed: 32 k of one block-column); stored chunk = ((a ^ q) << 2) | (b ^ (c & 3)): 16 distinct
//     chunks for the 16 (q, b), two lanes (the 8-byte halves) in each: all 64 banks, no conflict.
//   write (ds_write_b128, served per 8 consecutive lanes, bank mod 32 = the stored chunk mod 8): the 8 lanes hold the blocks
//     kb = 2 a1 + a0 with a0 = lane bit 0 and rows n with (n >> 2) & 3 = lane bits 1, 2, n & 3 fixed; chunk 4 kb + c is stored at
//     ((a0 ^ (n & 1)) << 2 | (c ^ ((n >> 2) & 3))) mod 8: 8 distinct values, no conflict.
__device__ __forceinline__ int mx6_dg_woff(int n, int ch) { return n * MX6_DG_WPITCH + ((ch ^ (((n & 3) << 2) | ((n >> 2) & 3))) << 4); }

// one block's 32 codes -> 32 16-bit values at one scale (v_cvt_scalef32_pk32_{bf16,f16}_fp6: element j of the result is code j,
// tools/probe/probe_fp6_cvt.hip part (a)), as four 16-byte chunks of 8 k; and the transposed LDS read of 4 rows of one column
typedef uint32_t mx6_v6u __attribute__((ext_vector_type(6)));
typedef uint32_t mx6_v16u __attribute__((ext_vector_type(16)));
typedef short mx6_short4_t __attribute__((ext_vector_type(4)));
typedef short mx6_short8_t __attribute__((ext_vector_type(8)));
typedef __bf16 mx6_bf16x32_t __attribute__((ext_vector_type(32)));
typedef _Float16 mx6_half32_t __attribute__((ext_vector_type(32)));
__device__ __forceinline__ mx6_short8_t mx6_tr2(const unsigned char* p0, const unsigned char* p1) {  // two ds_read_b64_tr_b16
    typedef __attribute__((address_space(3))) mx6_short4_t* lp;
    const mx6_short4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)p0), b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)p1);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <int DT> struct mx6_dg;
template <> struct mx6_dg<BIE_BF16> {
    static __device__ __forceinline__ mx6_v16u cvt(const mx6_v6u& w, float s) {
        return __builtin_bit_cast(mx6_v16u, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(w, s));
    }
    static __device__ __forceinline__ mx_bf16x8_t tr2(const unsigned char* p0, const unsigned char* p1) { return __builtin_bit_cast(mx_bf16x8_t, mx6_tr2(p0, p1)); }
};
template <> struct mx6_dg<BIE_F16> {
    static __device__ __forceinline__ mx6_v16u cvt(const mx6_v6u& w, float s) {
        return __builtin_bit_cast(mx6_v16u, __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(w, s));
    }
    static __device__ __forceinline__ mx_half8_t tr2(const unsigned char* p0, const unsigned char* p1) { return __builtin_bit_cast(mx_half8_t, mx6_tr2(p0, p1)); }
};

// One 128 x 128 tile of gx = gy . W on v_mfma_f32_32x32x16_{bf16,f16}, contracted over the N MXFP6 weight rows that start at row r0 of
// qw / sc (0, or (long)e * N for expert e): mx_dgrad_tile's contract (mxfp4_common.cuh) with E2M3 elements.  Tile rows from `rows` (a
// live row reads gy[src] and writes gx[dst]), columns k0 .. of K, rebiased by eblk[k / 32] (the caller's pointer already at the
// expert's K / 32 codes).  ODT, the element type of gx, is DT or BIE_F32.  4 waves as 2 x 2, wave tile 64 x 64.
// Per stage of 32 n a thread loads 2 x 16 bytes of gy, and the lower half of every wave one block (n, kb) of the stage's 32 x 4: its
// 24 bytes in three 8-byte pieces (a block is only 8-byte aligned) and its scale byte, into registers while the MFMAs run on the other
// LDS buffer.  It then converts the block with ONE v_cvt_scalef32_pk32 at 2^(s[n, kb] - e_blk[kb]) and writes the 64 bytes as four
// chunks of the 16-bit image (mx6_dg_woff).  Lane (r = lane & 31, h = lane >> 5) of a 16-n step reads its B fragment, rows 8 h .. + 7
// of column r of a 32-column block, with two ds_read_b64_tr_b16 (rows .. + 3 and + 4 .. + 7): lane 4 q + p of a 16-lane group gives the
// address of row q, columns 4 p .. + 3, of the group's 4 x 16 block and receives column (lane & 15).  Every lane of every wave gives an
// in-bounds address (the image is always whole: rows past N and blocks past K are written as zeros), the loops are uniform and there
// is no return before them, so EXEC is all ones at the transposed reads.  The accumulators acc[.][j] hold column 32 j + r in lane r;
// before the epilogue the lanes of a pair (r even, r + 1) swap one value each, so that lane r even holds columns r, r + 1 and lane r
// odd 32 + r - 1, 32 + r, and the epilogue is mx_dgrad_tile's: two adjacent columns in one store.  gy rows have any length N: whole
// 16-byte pieces where `vec` (N % 8 == 0 and gy 16-byte aligned), else 16-bit loads, each guarded by n < N.  Dead rows and whatever
// lies past N / K: gy and codes load as zero, the scale as 1.0, so the padding adds exact zeros.  gy rows in LDS: 80-byte pitch, the
// 16-byte slot of row r is 5 r mod 16, distinct over each 16-lane group of the ds_read_b128 fragment reads ({0-3, 12-15, 20-27} and
// {4-11, 16-19, 28-31} of a half-wave).  The gy WRITES are 2-way on one bank quad: the 8 lanes of a ds_write_b128 group hold the four
// pieces of two rows, banks 20 r + 4 c mod 32, and piece 3 of the odd row meets piece 0 of the even one.  Counters show exactly that
// and nothing else (profiles/mxfp6_grad_pmc.txt: 16 conflict cycles per wave and stage, none with the write order changed to 8 rows
// of one piece per group); that order was measured slower all the same (its global loads put neighbouring lanes on different rows),
// so the staging order of mx_dgrad_tile stays.  All 256 threads of the workgroup must call it together.
template <int DT, int ODT, class Rows>
__device__ __forceinline__ void mx6_dgrad_tile(const Rows& rows, const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw,
                                               const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, long r0,
                                               int k0, int N, int K, bool vec) {
    typedef mx_frag<DT> F;
    typedef mx6_dg<DT> G;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX6_DG_STAGE];
    constexpr int W_OFF = MX6_DG_BM * MX6_DG_APITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int NT = (N + MX6_DG_BN - 1) / MX6_DG_BN, KB = K >> 5;

    // this thread's load slots.  Weight block: w = 32 wave + lane (lane < 32); block-column wkb = w bits 0 and 3, row wn = w bits 4, 5
    // (n & 3), bits 1, 2 ((n >> 2) & 3) and bit 6 (n >> 4): the order the image's write banks want (mx6_dg_woff)
    const bool wt = lane < 32;
    const int w = wave * 32 + (lane & 31);
    const int wkb = (w & 1) | ((w >> 2) & 2), wn = ((w >> 4) & 3) | (((w >> 1) & 3) << 2) | (((w >> 6) & 1) << 4);
    const bool wk_ok = wt && (k0 >> 5) + wkb < KB;
    const uint8_t* wsrc = qw + r0 * ((long)KB * MX6_BLOCK_BYTES) + (long)((k0 >> 5) + wkb) * MX6_BLOCK_BYTES;
    const uint8_t* ssrc = sc + r0 * KB + (k0 >> 5) + wkb;
    const uint32_t eb = wk_ok ? eblk[(k0 >> 5) + wkb] : 0u;
    const uint16_t* grow[2];  // the gy rows of this thread's two 16-byte pieces per stage: tile row (t + 256 i) / 4, piece t & 3
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (t + 256 * i) >> 2;
        grow[i] = rows.live(row) ? gy + rows.src(row) * N : nullptr;
    }
    uint4_t ra[2];
    uint2_t rw[3];
    float rs;
    auto load = [&](int nt) {
        const int na = nt * MX6_DG_BN + (t & 3) * 8;  // the first n of this thread's pieces
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (!grow[i] || na >= N) {
                ra[i] = uint4_t{0u, 0u, 0u, 0u};
            } else if (vec) {  // uniform; N % 8 == 0: the piece lies inside the row
                ra[i] = *reinterpret_cast<const uint4_t*>(grow[i] + na);
            } else {
                uint32_t h[8];
#pragma unroll
                for (int j = 0; j < 8; j++) h[j] = na + j < N ? (uint32_t)grow[i][na + j] : 0u;
                ra[i] = uint4_t{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            }
        }
        const int n = nt * MX6_DG_BN + wn;
        const bool ok = wk_ok && n < N;
        const uint2_t* src = reinterpret_cast<const uint2_t*>(wsrc + (long)n * ((long)KB * MX6_BLOCK_BYTES));
#pragma unroll
        for (int i = 0; i < 3; i++) rw[i] = ok ? src[i] : uint2_t{0u, 0u};
        rs = ok ? mx_rebias(ssrc[(long)n * KB], eb) : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX6_DG_STAGE;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int q = t + 256 * i, row = q >> 2, c16 = q & 3;
            *reinterpret_cast<uint4_t*>(st + row * MX6_DG_APITCH + c16 * 16) = ra[i];
        }
        const mx6_v16u v = G::cvt(mx6_v6u{rw[0].x, rw[0].y, rw[1].x, rw[1].y, rw[2].x, rw[2].y}, rs);
        if (wt) {
#pragma unroll
            for (int c = 0; c < 4; c++)
                *reinterpret_cast<uint4_t*>(st + W_OFF + mx6_dg_woff(wn, wkb * 4 + c)) = uint4_t{v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]};
        }
    };

    float16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int rl = lane & 31, hh = lane >> 5;
    // the transposed reads of this lane: row tq of its group's 4-row block, the 8-byte half tp & 1 of chunk tch (+ 4 j + 8 wx)
    const int tq = (lane >> 2) & 3, tp = lane & 3, tch = wx * 8 + ((lane >> 4) & 1) * 2 + (tp >> 1);
    load(0);
    store(0);
    __syncthreads();
    for (int nt = 0; nt < NT; nt++) {
        const int buf = nt & 1;
        if (nt + 1 < NT) load(nt + 1);
        const unsigned char* st = lds + buf * MX6_DG_STAGE;
#pragma unroll
        for (int ns = 0; ns < MX6_DG_BN / 16; ns++) {
            typename F::t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX6_DG_APITCH + ns * 32 + hh * 16));
            const int n0 = ns * 16 + hh * 8 + tq;
#pragma unroll
            for (int j = 0; j < 2; j++)
                b[j] = G::tr2(st + W_OFF + mx6_dg_woff(n0, tch + 4 * j) + (tp & 1) * 8, st + W_OFF + mx6_dg_woff(n0 + 4, tch + 4 * j) + (tp & 1) * 8);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = F::mfma(a[i], b[j], acc[i][j]);
        }
        if (nt + 1 < NT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: acc[i][j][r] is column 32 j + rl of the wave's 64, tile row (r & 3) + 8 (r >> 2) + 4 hh.  The lanes of a pair swap: the even
    // lane gives its column 32 + rl and takes the odd lane's column rl + 1, so v0, v1 are two adjacent columns from kc on
    const bool odd = (rl & 1) != 0;
    const int k = k0 + wx * 64 + (odd ? 32 + rl - 1 : rl);
    const bool k_ok = k < K;  // K % 32 == 0 and k is even: the pair lies inside K or outside
    const float cs = e8m0_f32(eblk[k_ok ? k >> 5 : 0]);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float give = odd ? acc[i][0][r] : acc[i][1][r];
            const float take = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(give), 0xB1, 0xf, 0xf, false));  // quad_perm [1, 0, 3, 2]
            const float v0 = odd ? take : acc[i][0][r], v1 = odd ? acc[i][1][r] : take;
            const int row = wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (k_ok && rows.live(row)) mx_store2<ODT>(gx, rows.dst(row) * K + k, v0 * cs, v1 * cs);
        }
}

// The pk32 convert's native result (32 16-bit values) and its pieces, for the forms that keep it in registers.  The pieces are taken
// element by element from the native vector: taking dwords out of a bit cast to mx6_v16u is folded by the compiler (ROCm 7 clang) to
// dword 0 for every index where the dwords feed arithmetic directly (mx6_dg::cvt, whose result is stored whole, is not affected).
template <int DT> struct mx6_w16;
template <> struct mx6_w16<BIE_BF16> {
    typedef mx6_bf16x32_t t;
    static __device__ __forceinline__ t cvt(const mx6_v6u& w, float s) { return __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(w, s); }
    static __device__ __forceinline__ bf16x2_t pair(const t& v, int i) { return bf16x2_t{v[2 * i], v[2 * i + 1]}; }
    static __device__ __forceinline__ mx_bf16x8_t chunk(const t& v, int c) {
        return mx_bf16x8_t{v[8 * c], v[8 * c + 1], v[8 * c + 2], v[8 * c + 3], v[8 * c + 4], v[8 * c + 5], v[8 * c + 6], v[8 * c + 7]};
    }
};
template <> struct mx6_w16<BIE_F16> {
    typedef mx6_half32_t t;
    static __device__ __forceinline__ t cvt(const mx6_v6u& w, float s) { return __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(w, s); }
    static __device__ __forceinline__ half2_t pair(const t& v, int i) { return half2_t{v[2 * i], v[2 * i + 1]}; }
    static __device__ __forceinline__ mx_half8_t chunk(const t& v, int c) {
        return mx_half8_t{v[8 * c], v[8 * c + 1], v[8 * c + 2], v[8 * c + 3], v[8 * c + 4], v[8 * c + 5], v[8 * c + 6], v[8 * c + 7]};
    }
};

// ---- the weight-only (W6A16) prefill tile ----------------------------------------------------------------------------------------------------
constexpr int MX6_BK = 64;                             // k per stage: two blocks, 48 code bytes per weight row
constexpr int MX6_WROW = MX6_BK / 32 * MX6_BLOCK_BYTES;  // 48
// 56 bytes per weight row in LDS (14 dwords).  A lane's block is the 24 bytes at row * 56 + 24 * block, three 8-byte reads.  The lanes
// of a half-wave read the same block of rows r = 0 .. 31: per piece the dwords 14 r + c and 14 r + c + 1.  By the rule above: as
// ds_read_b64 (per 32 lanes, bank = dword mod 64), 14 r mod 64 = 2 (7 r mod 32) takes 32 distinct even values, so the 32 dword pairs
// tile all 64 banks; as ds_read2_b64 (per 16 lanes, bank = dword mod 32), 14 r mod 32 = 2 (7 r mod 16) takes 16 distinct even values.
// Counters (profiles/mxfp6_pmc.txt): 16 bank-conflict cycles per wave and stage against 8 for mx_gemm_tile in the same run; the 8 more are
// what the packed WRITES predict (a half-wave's 32 consecutive 8-byte pieces span 74 or 76 dwords), 3 % of a stage's matrix time.
constexpr int MX6_WPITCH = MX6_WROW + 8;
constexpr int MX6_STAGE = MX_BM * MX_APITCH + MX_BN * MX6_WPITCH + MX_BN * 2 * 4;  // x (mx_gemm_tile's rows), codes, two fp32 rebiased scales per row

// One 128 x 128 tile of y = x . W^T (+ bias) on v_mfma_f32_32x32x16_{bf16,f16}: mx_gemm_tile's contract and structure (mxfp4_common.cuh)
// with MXFP6 weights.  Tile rows from `rows`, columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or
// (long)e * N for an expert e).  4 waves as 2 x 2, wave tile 64 x 64.  Per 64-k stage a thread loads 4 x 16 bytes of x, three 8-byte
// pieces of codes (a weight row's pitch is 24 K / 32 bytes: nothing wider is aligned) and one scale byte into registers while the
// MFMAs run on the other LDS buffer, then writes them (the scale already rebiased to fp32 by e_col).  The weight tile is staged
// PACKED.  The contraction order inside a stage is free, so lane (n = lane & 31, h = lane >> 5) reads block h of weight row n, turns
// its 32 codes into 32 16-bit values with ONE v_cvt_scalef32_pk32 at 2^(s - e_col[n]) (element j = code j, probe_fp6_cvt.hip part (a)),
// and uses the four 8-k chunks as the B fragments of four MFMAs; the A fragment of MFMA i is then x at k = 32 h + 8 i .. + 7 of the
// stage.  No transposed read and no 16-bit image of W in LDS.  The x reads are 16 bytes at row * 144 + 64 h + 16 i: a 16-lane group of
// the ds_read_b128 reads 16 consecutive rows at one offset, and the 16-byte slot of row r is 9 r + c mod 16: 16 distinct slots (mx_gemm_tile's
// pad, unchanged).  Dead rows and whatever lies past N / K: x and
// codes load as zero, scales as 1.0, so the padding adds exact zeros.  All 256 threads of the workgroup must call it together.
template <int DT, class Rows>
__device__ __forceinline__ void mx6_gemm_tile(const Rows& rows, const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw,
                                              const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                              void* __restrict__ y, long r0, int n0, int N, int K) {
    typedef mx_frag<DT> F;
    typedef mx6_w16<DT> G;
    static_assert(2 * MX6_STAGE <= 65536, "static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX6_STAGE];
    constexpr int W_OFF = MX_BM * MX_APITCH, S_OFF = W_OFF + MX_BN * MX6_WPITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KT = (K + MX6_BK - 1) / MX6_BK, KB = K >> 5;

    // this thread's load slots: code pieces t, t + 256, t + 512 of the tile's 128 x 6 (row = piece / 6, 8-byte piece % 6 of the row's 48
    // bytes: block (piece % 6) / 3 of the stage); the scale of row t >> 1, block t & 1
    const uint8_t* wsrc[3];
    bool wok[3];
    int wblk[3], wdst[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int p = t + 256 * i, row = p / 6, part = p - row * 6;
        wblk[i] = part / 3;
        wdst[i] = W_OFF + row * MX6_WPITCH + part * 8;
        wok[i] = n0 + row < N;
        wsrc[i] = qw + (r0 + min(n0 + row, N - 1)) * ((long)KB * MX6_BLOCK_BYTES) + part * 8;
    }
    const int bn = t >> 1, bh = t & 1;
    const int nb = n0 + bn;
    const bool nb_ok = nb < N;
    const uint8_t* ssrc = sc + (r0 + min(nb, N - 1)) * KB + bh;
    const uint32_t e = nb_ok ? ecol[r0 + nb] : 0u;
    const uint16_t* xrow[4];  // the x rows of this thread's four 16-byte pieces per stage: tile row (t + 256 i) / 8, piece t & 7
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = (t + 256 * i) >> 3;
        xrow[i] = rows.live(row) ? x + rows.src(row) * K + (t & 7) * 8 : nullptr;
    }
    uint4_t ra[4];
    uint2_t rw[3];
    float rs;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            ra[i] = (xrow[i] && kt * MX6_BK + (t & 7) * 8 < K) ? *reinterpret_cast<const uint4_t*>(xrow[i] + kt * MX6_BK) : uint4_t{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 3; i++)
            rw[i] = (wok[i] && kt * 2 + wblk[i] < KB) ? __builtin_nontemporal_load(reinterpret_cast<const uint2_t*>(wsrc[i] + (long)kt * MX6_WROW))
                                                      : uint2_t{0u, 0u};
        rs = (nb_ok && kt * 2 + bh < KB) ? mx_rebias(__builtin_nontemporal_load(ssrc + kt * 2), e) : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX6_STAGE;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 256 * i, row = q >> 3, c16 = q & 7;
            *reinterpret_cast<uint4_t*>(st + row * MX_APITCH + c16 * 16) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) *reinterpret_cast<uint2_t*>(st + wdst[i]) = rw[i];
        reinterpret_cast<float*>(st + S_OFF)[bn * 2 + bh] = rs;
    };

    float16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int rl = lane & 31, hh = lane >> 5;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load(kt + 1);
        const unsigned char* st = lds + buf * MX6_STAGE;
        const float* ss = reinterpret_cast<const float*>(st + S_OFF);
        typename G::t bv[2];  // block hh of the wave's weight rows 32 j + rl: 32 values, k 32 hh .. + 31 of the stage
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = wx * 64 + j * 32 + rl;
            const uint2_t* p = reinterpret_cast<const uint2_t*>(st + W_OFF + n * MX6_WPITCH + hh * MX6_BLOCK_BYTES);
            const uint2_t p0 = p[0], p1 = p[1], p2 = p[2];
            bv[j] = G::cvt(mx6_v6u{p0.x, p0.y, p1.x, p1.y, p2.x, p2.y}, ss[n * 2 + hh]);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            typename F::t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX_APITCH + hh * 64 + ks * 16));
#pragma unroll
            for (int j = 0; j < 2; j++) b[j] = G::chunk(bv[j], ks);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = F::mfma(a[i], b[j], acc[i][j]);
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: column n = lane & 31, tile row (r & 3) + 8 (r >> 2) + 4 hh.  e_col = 255 (a NaN block in the column) makes cs NaN
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int n = n0 + wx * 64 + j * 32 + rl;
        if (n >= N) continue;
        const float cs = e8m0_f32(ecol[r0 + n]);
        const float bv0 = bias ? dt_traits<DT>::load(bias, r0 + n) : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (rows.live(row)) {
                    float v = acc[i][j][r] * cs;
                    if (bias) v += bv0;
                    dt_traits<DT>::store(y, rows.dst(row) * N + n, v);
                }
            }
    }
}

// the sums of a wave's two halves on the DPP network (wave_sum_f32's first five steps): lane 31 holds lanes 0 .. 31, lane 63 lanes 32 .. 63
__device__ __forceinline__ float mx6_half_sum_f32(float v) {
    v = dpp_add<0xB1, 0xf>(v);
    v = dpp_add<0x4E, 0xf>(v);
    v = dpp_add<0x141, 0xf>(v);
    v = dpp_add<0x140, 0xf>(v);
    return dpp_add<0x142, 0xa>(v);
}

// (host) The decode forms' dispatch over the group width, for mxfp6.hip and mxfp6_moe.hip: f(std::integral_constant<int, G>) with G the
// threads per column group, the largest of 128, 64, 32 whose padded last pass wastes at most an eighth of the passes' slots, else 32.
template <class F>
static void mx6_decode_group(int KB, F&& f) {
    if ((long)cdiv(KB, 128) * 128 * 8 <= (long)KB * 9) f(std::integral_constant<int, 128>{});
    else if ((long)cdiv(KB, 64) * 64 * 8 <= (long)KB * 9) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 32>{});
}

}  // namespace bie
