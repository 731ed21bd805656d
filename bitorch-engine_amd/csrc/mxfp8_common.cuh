// The MXFP8 (OCP microscaling FP8, E4M3 elements) weight-only (W8A16) device-side rules (gfx950): the two-at-a-time convert of code bytes
// to exact 16-bit values, the 128 x 128 prefill tile body (mx8_gemm_tile: mx8_gemm_kernel of mxfp8.hip) and the input-gradient 128 x 128
// tile body (mx8_dgrad_tile: the kernels of mxfp8_grad.hip).  The E8M0 block scales, the
// rebias, the row sources, the x side of the tile and the 16-bit MFMA are those of mxfp4_common.cuh; the half-wave sum and the decode
// forms' group dispatch are those of mxfp6_common.cuh.
//
// A block of 32 codes is 32 bytes, code j in byte j, and a weight row is K bytes: every block is 32-byte aligned under a 16-byte aligned
// qweight.  Code bits: bit 7 sign, bits 6:3 exponent (bias 7), bits 2:0 mantissa; 0x7f / 0xff are NaN, there is no Inf.
// v_cvt_scalef32_pk_{f16,bf16}_fp8 turns two bytes of a dword into two 16-bit values at an fp32 scale; op_sel picks the low (bytes 0, 1)
// or the high (bytes 2, 3) half of the dword, the lower byte in the lower half of the result (tools/probe/probe_fp8_cvt.hip part (a),
// profiles/mxfp8_cvt_probe.txt).  Every E4M3 value is exact in fp16 and in bf16 at scale 1.0 (part (b)); a NaN code gives a NaN (part (d)).
#pragma once
#include "mxfp6_common.cuh"

namespace bie {

// one dword (four codes, k .. k + 3) -> two pairs of 16-bit values at scale s
template <int DT> struct mx8_w16;
template <> struct mx8_w16<BIE_BF16> {
    typedef bf16x2_t t;
    template <bool HI>
    static __device__ __forceinline__ t cvt(uint32_t w, float s) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, HI); }
};
template <> struct mx8_w16<BIE_F16> {
    typedef half2_t t;
    template <bool HI>
    static __device__ __forceinline__ t cvt(uint32_t w, float s) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, HI); }
};

// two dwords (eight codes, k .. k + 7) -> one 8-k MFMA fragment at scale s: four converts
template <int DT>
__device__ __forceinline__ typename mx_frag<DT>::t mx8_frag(uint32_t w0, uint32_t w1, float s) {
    typedef mx8_w16<DT> C;
    const typename C::t a = C::template cvt<false>(w0, s), b = C::template cvt<true>(w0, s);
    const typename C::t c = C::template cvt<false>(w1, s), d = C::template cvt<true>(w1, s);
    return typename mx_frag<DT>::t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// the decode forms (mx8_decode_kernel of mxfp8.hip, mx8m_decode_kernel of mxfp8_moe.hip)
constexpr int MX8_UNIT = 16;  // bytes (= weights) per unit of work: 16 (half a block) or 32 (a block)

// ---- the weight-only (W8A16) prefill tile ----------------------------------------------------------------------------------------------------
constexpr int MX8_BK = 64;  // k per stage: two blocks, 64 code bytes per weight row
// 64 bytes per weight row in LDS, NO pad: the 16-byte piece c (0 .. 3) of tile row n is stored at piece c ^ ((n >> 2) & 3) of the row, so
// the 16-byte slot of a piece (its address / 16) is 4 n + (c ^ ((n >> 2) & 3)).  By the bank rule of mxfp6_common.cuh (bank = dword mod
// 64; a ds_read_b128 is served per 16 lanes, a ds_write_b128 per 8 consecutive lanes on bank mod 32):
//   fragment reads (ds_read_b128): the lanes of a half-wave read ONE piece c of the rows n = 0 .. 31 of a 32-row block.  The slot mod 16
//     is 4 (n & 3) + (c ^ ((n >> 2) & 3)), a function of n mod 16 alone and one-to-one on it (n & 3 picks the group of four slots,
//     (n >> 2) & 3 the slot in it), so any 16 lanes whose rows differ mod 16 (each of the two 16-lane groups of a half-wave, whichever
//     lanes they are) cover all 16 slots = all 64 banks once: no conflict.
//   staging writes (ds_write_b128): the 8 lanes hold the four pieces of rows n (even) and n + 1; slot mod 8 = 4 (n & 1) + (c ^ f) with one
//     f for both rows (they share n >> 2): the even row takes slots 0 .. 3 and the odd row 4 .. 7, each once: no conflict.
//   scales (ds_read_b32 of fp32 [128 rows][2 blocks]): the 64 lanes read dword 2 n + h for n = 0 .. 31, h = 0, 1: 64 banks once.
// A padded pitch cannot do both: the reads want pitch / 16 odd, and then the pieces 0 .. 3 of row n meet those of row n + 1 on the
// write (the gy rows of mx6_dgrad_tile have that 2-way write).
constexpr int MX8_WPITCH = MX8_BK;
__device__ __forceinline__ int mx8_woff(int n, int c) { return n * MX8_WPITCH + ((c ^ ((n >> 2) & 3)) << 4); }
constexpr int MX8_STAGE = MX_BM * MX_APITCH + MX_BN * MX8_WPITCH + MX_BN * 2 * 4;  // x (mx_gemm_tile's rows), codes, two fp32 rebiased scales per row

// One 128 x 128 tile of y = x . W^T (+ bias) on v_mfma_f32_32x32x16_{bf16,f16}: mx_gemm_tile's contract and structure (mxfp4_common.cuh)
// with MXFP8 weights.  Tile rows from `rows`, columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or
// (long)e * N for an expert e).  4 waves as 2 x 2, wave tile 64 x 64.  Per 64-k stage a thread loads 4 x 16 bytes of x, 2 x 16 bytes of
// codes (the four lanes of a quad read the 64 contiguous bytes of one weight row; piece p = t + 256 i is row p / 4, piece p % 4) and one
// scale byte into registers while the MFMAs run on the other LDS buffer, then writes them (the scale already rebiased to fp32 by
// e_col).  The weight tile is staged PACKED, one byte per weight.  The contraction order inside a stage is free, so lane (n = lane & 31,
// h = lane >> 5) reads block h of weight row n (two ds_read_b128), and turns its 32 codes into four 8-k B fragments with 16 converts at
// 2^(s - e_col[n]): a fragment holds at most 448 in magnitude, and what falls below the fp16 normal range is rounded to an fp16
// subnormal (probe_fp8_cvt.hip part (c)).  The A fragment of MFMA i is then x at k = 32 h + 8 i .. + 7 of the stage (mx6_gemm_tile's x
// reads).  No 16-bit image of W, in LDS or anywhere.  Dead rows and whatever lies past N / K: x and codes load as zero, scales as 1.0, so
// the padding adds exact zeros.  All 256 threads of the workgroup must call it together.
template <int DT, class Rows>
__device__ __forceinline__ void mx8_gemm_tile(const Rows& rows, const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw,
                                              const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                              void* __restrict__ y, long r0, int n0, int N, int K) {
    typedef mx_frag<DT> F;
    static_assert(2 * MX8_STAGE <= 65536, "static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX8_STAGE];
    constexpr int W_OFF = MX_BM * MX_APITCH, S_OFF = W_OFF + MX_BN * MX8_WPITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KT = (K + MX8_BK - 1) / MX8_BK, KB = K >> 5;

    // this thread's load slots: code pieces t and t + 256 of the tile's 128 x 4 (rows t / 4 and 64 + t / 4, piece t & 3: block (t & 3) / 2
    // of the stage); the scale of row t >> 1, block t & 1
    const int wc = t & 3;
    const uint8_t* wsrc[2];
    bool wok[2];
    int wdst[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (t >> 2) + 64 * i;
        wdst[i] = W_OFF + mx8_woff(row, wc);
        wok[i] = n0 + row < N;
        wsrc[i] = qw + (r0 + min(n0 + row, N - 1)) * (long)K + wc * 16;
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
    uint4_t ra[4], rw[2];
    float rs;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            ra[i] = (xrow[i] && kt * MX8_BK + (t & 7) * 8 < K) ? *reinterpret_cast<const uint4_t*>(xrow[i] + kt * MX8_BK) : uint4_t{0u, 0u, 0u, 0u};
        const bool kin = kt * 2 + (wc >> 1) < KB;
#pragma unroll
        for (int i = 0; i < 2; i++)
            rw[i] = (wok[i] && kin) ? __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wsrc[i] + (long)kt * MX8_BK)) : uint4_t{0u, 0u, 0u, 0u};
        rs = (nb_ok && kt * 2 + bh < KB) ? mx_rebias(__builtin_nontemporal_load(ssrc + kt * 2), e) : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX8_STAGE;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 256 * i, row = q >> 3, c16 = q & 7;
            *reinterpret_cast<uint4_t*>(st + row * MX_APITCH + c16 * 16) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) *reinterpret_cast<uint4_t*>(st + wdst[i]) = rw[i];
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
        const unsigned char* st = lds + buf * MX8_STAGE;
        const float* ss = reinterpret_cast<const float*>(st + S_OFF);
        uint4_t bw[2][2];  // block hh of the wave's weight rows 32 j + rl: 32 codes, k 32 hh .. + 31 of the stage
        float bs[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = wx * 64 + j * 32 + rl;
            bw[j][0] = *reinterpret_cast<const uint4_t*>(st + W_OFF + mx8_woff(n, 2 * hh));
            bw[j][1] = *reinterpret_cast<const uint4_t*>(st + W_OFF + mx8_woff(n, 2 * hh + 1));
            bs[j] = ss[n * 2 + hh];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
            typename F::t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX_APITCH + hh * 64 + ks * 16));
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint4_t& w = bw[j][ks >> 1];
                b[j] = (ks & 1) ? mx8_frag<DT>(w.z, w.w, bs[j]) : mx8_frag<DT>(w.x, w.y, bs[j]);
            }
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

// ---- the input-gradient tile -----------------------------------------------------------------------------------------------------------------
constexpr int MX8_DG_BM = 128, MX8_DG_BK = 128, MX8_DG_BN = 64;  // rows of gy, columns k of gx, contraction rows n of a stage
constexpr int MX8_DG_APITCH = MX8_DG_BN * 2 + 16;                // bytes per gy row in LDS (MX_APITCH's pad)
// The codes of a stage in LDS: [64 k pairs][64 n] of 16-bit units (unit (p, n) = the code bytes of W[n, 2 p] and W[n, 2 p + 1]), 128
// bytes per k pair + 16: the 16-byte slot (address / 16) of the chunk of rows 8 c .. + 7 of k pair p is 9 p + c.  By the bank rule of
// mxfp6_common.cuh (bank = dword mod 64; a ds_read_b128 is served per 16 lanes, a ds_write_b128 per 8 consecutive lanes on bank mod 32):
//   fragment reads (ds_read_b128): the lanes of a half-wave read ONE chunk c of the k pairs p = p0 + r, r = 0 .. 31.  The slot mod 16 is
//     (9 r + const) mod 16, one-to-one on r mod 16 (9 is odd), so any 16 lanes whose r differ mod 16 (each of the two 16-lane groups of a
//     half-wave, whichever lanes they are) cover all 16 slots = all 64 banks once: no conflict.
//   staging writes (ds_write_b128): the 8 lanes hold the dword columns d = 4 a + i (i = 0 .. 3: k pairs p = 2 d + j in write j) of the
//     chunks c = 2 b and 2 b + 1; slot mod 8 = (9 (8 a + 2 i + j) + c) mod 8 = (2 i + (c & 1) + j + 2 b) mod 8: 8 distinct values for
//     the 8 (i, c & 1), no conflict.
// A pitch of 128 cannot do the reads (slot = 8 p + c: two values mod 16), and 128 + 8 is not 16-byte aligned.
constexpr int MX8_DG_WPITCH = MX8_DG_BN * 2 + 16;
constexpr int MX8_DG_SPITCH = MX8_DG_BN + 4;  // fp32 per block-column of rebiased scales (MX_DG_SPITCH's pad)
constexpr int MX8_DG_STAGE = MX8_DG_BM * MX8_DG_APITCH + (MX8_DG_BK / 2) * MX8_DG_WPITCH + (MX8_DG_BK / 32) * MX8_DG_SPITCH * 4;  // 18432 + 9216 + 1088
static_assert(2 * MX8_DG_STAGE + MXM_BM * 4 <= 65536, "two buffers and the grouped kernel's prow[] in the 64 KiB of static LDS");

// Four dwords of one k pair (dword i: the unit of row n + 2 i in the low half, of row n + 2 i + 1 in the high half) at their rows' rebiased
// scales -> the 8-n fragments of the units' first bytes (column 2 p) and second bytes (column 2 p + 1): one convert per unit, each half
// of a dword under its own row's scale (op_sel), the halves of the results regrouped.
template <int DT>
__device__ __forceinline__ void mx8_frag_columns(const uint4_t& w, const float4_t& s0, const float4_t& s1, typename mx_frag<DT>::t& lo,
                                                 typename mx_frag<DT>::t& hi) {
    typedef mx8_w16<DT> C;
    const typename C::t v0 = C::template cvt<false>(w.x, s0[0]), v1 = C::template cvt<true>(w.x, s0[1]);
    const typename C::t v2 = C::template cvt<false>(w.y, s0[2]), v3 = C::template cvt<true>(w.y, s0[3]);
    const typename C::t v4 = C::template cvt<false>(w.z, s1[0]), v5 = C::template cvt<true>(w.z, s1[1]);
    const typename C::t v6 = C::template cvt<false>(w.w, s1[2]), v7 = C::template cvt<true>(w.w, s1[3]);
    lo = typename mx_frag<DT>::t{v0[0], v1[0], v2[0], v3[0], v4[0], v5[0], v6[0], v7[0]};
    hi = typename mx_frag<DT>::t{v0[1], v1[1], v2[1], v3[1], v4[1], v5[1], v6[1], v7[1]};
}

// One 128 x 128 tile of gx = gy . W on v_mfma_f32_32x32x16_{bf16,f16}, contracted over the N MXFP8 weight rows that start at row r0 of
// qw / sc (0, or (long)e * N for expert e): mx_dgrad_tile's contract (mxfp4_common.cuh) with E4M3 elements.  Tile rows from `rows` (a
// live row reads gy[src] and writes gx[dst]), columns k0 .. of K, rebiased by eblk[k / 32] (the caller's pointer already at the
// expert's K / 32 codes).  ODT, the element type of gx, is DT or BIE_F32.  4 waves as 2 x 2, wave tile 64 x 64.
// Per stage of 64 n a thread loads 4 x 16 bytes of gy, eight dwords of codes (dword column d of the tile's 32: k pairs 2 d, 2 d + 1; rows
// 8 c .. + 7 of the stage) and one scale byte into registers while the MFMAs run on the other LDS buffer.  A wave's code load touches
// four rows, the 128 contiguous bytes of each (lane bits 0, 1, 3, 4, 5 are d; bit 2 and the wave are c).  It then regroups the eight
// dwords with eight v_perm_b32 (the low 16-bit units of two rows into one dword, the high units into another) and writes two
// ds_write_b128: LDS holds [k pair][n], unit (p, n) next to (p, n + 1).  The scale is rebiased to fp32 and staged as [block-column][n]
// (mx_dgrad_tile's).  Lane (r = lane & 31, h = lane >> 5) of a 16-n step reads the 8 units of k pair r, rows 8 h .. + 7, in one
// ds_read_b128 and their 8 scales in two; each unit is one v_cvt_scalef32_pk_{f16,bf16}_fp8 at its own row's scale; the 8 first values
// and the 8 second values are the B fragments of two MFMAs whose output column for lane r is k0 + 2 r and k0 + 2 r + 1, so the epilogue
// stores two adjacent columns per lane.  No 16-bit image of W, in LDS or anywhere.  gy rows have any length N: whole 16-byte pieces
// where `vec` (N % 8 == 0 and gy 16-byte aligned), else 16-bit loads, each guarded by n < N.  Dead rows and whatever lies past N / K:
// gy and codes count as zero and scales as 1.0, so the padding adds exact zeros; the code and scale loads are clamped to the last row /
// column and their values replaced, not skipped.  All 256 threads of the workgroup must call it together.
template <int DT, int ODT, class Rows>
__device__ __forceinline__ void mx8_dgrad_tile(const Rows& rows, const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw,
                                               const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, long r0,
                                               int k0, int N, int K, bool vec) {
    typedef mx_frag<DT> F;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX8_DG_STAGE];
    constexpr int B_OFF = MX8_DG_BM * MX8_DG_APITCH, S_OFF = B_OFF + (MX8_DG_BK / 2) * MX8_DG_WPITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int NT = (N + MX8_DG_BN - 1) / MX8_DG_BN, KB = K >> 5;

    // this thread's load slots
    const int bd = (t & 3) | (((t >> 3) & 7) << 2), bc = ((t >> 2) & 1) | (wave << 1);  // codes: dword column bd, rows 8 bc .. + 7 of the stage
    const bool bk_ok = k0 + bd * 4 < K;
    const uint32_t wcol = (uint32_t)min(k0 + bd * 4, K - 4);
    uint32_t woff[8];  // the eight rows' byte offsets from the stage's first row (below 64 K <= 2^26): loop-invariant in a whole stage
#pragma unroll
    for (int i = 0; i < 8; i++) woff[i] = (uint32_t)(bc * 8 + i) * (uint32_t)K + wcol;
    const int sn = t >> 2, sb = t & 3;  // scale: row sn of the stage, block-column sb of the tile
    const bool sb_ok = (k0 >> 5) + sb < KB;
    const uint8_t* ssrc = sc + r0 * KB + min((k0 >> 5) + sb, KB - 1);
    const uint32_t eb = eblk[min((k0 >> 5) + sb, KB - 1)];
    const uint16_t* grow[4];  // the gy rows of this thread's four 16-byte pieces per stage: tile row (t + 256 i) / 8, piece t & 7
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = (t + 256 * i) >> 3;
        grow[i] = rows.live(row) ? gy + rows.src(row) * N : nullptr;
    }
    uint4_t ra[4];
    uint32_t rb[8];
    float rs;
    auto load = [&](int nt) {
        const int na = nt * MX8_DG_BN + (t & 7) * 8;  // the first n of this thread's pieces
#pragma unroll
        for (int i = 0; i < 4; i++) {
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
        const uint8_t* wrow = qw + (r0 + (long)nt * MX8_DG_BN) * K;  // uniform: the stage's first row
        const int left = N - nt * MX8_DG_BN;                         // rows of the stage inside N, >= 1
        if (left >= MX8_DG_BN) {                                     // uniform
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(wrow + woff[i]);
                rb[i] = bk_ok ? w : 0u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int r = bc * 8 + i;
                const uint32_t w = *reinterpret_cast<const uint32_t*>(wrow + ((uint32_t)min(r, left - 1) * (uint32_t)K + wcol));
                rb[i] = (bk_ok && r < left) ? w : 0u;
            }
        }
        const int n = nt * MX8_DG_BN + sn;
        const float s = mx_rebias(ssrc[(long)min(n, N - 1) * KB], eb);
        rs = (sb_ok && n < N) ? s : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX8_DG_STAGE;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 256 * i, row = q >> 3, c16 = q & 7;
            *reinterpret_cast<uint4_t*>(st + row * MX8_DG_APITCH + c16 * 16) = ra[i];
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {  // k pair 2 bd + j of rows 8 bc .. + 7: bytes 2 j, 2 j + 1 of every row's dword
            const uint32_t sel = j ? 0x07060302u : 0x05040100u;
            const uint4_t w = {__builtin_amdgcn_perm(rb[1], rb[0], sel), __builtin_amdgcn_perm(rb[3], rb[2], sel),
                               __builtin_amdgcn_perm(rb[5], rb[4], sel), __builtin_amdgcn_perm(rb[7], rb[6], sel)};
            *reinterpret_cast<uint4_t*>(st + B_OFF + (bd * 2 + j) * MX8_DG_WPITCH + bc * 16) = w;
        }
        reinterpret_cast<float*>(st + S_OFF)[sb * MX8_DG_SPITCH + sn] = rs;
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
    for (int nt = 0; nt < NT; nt++) {
        const int buf = nt & 1;
        if (nt + 1 < NT) load(nt + 1);
        const unsigned char* st = lds + buf * MX8_DG_STAGE;
        const unsigned char* bcol = st + B_OFF + (wx * 32 + rl) * MX8_DG_WPITCH + hh * 16;
        const float* scol = reinterpret_cast<const float*>(st + S_OFF) + (wx * 2 + (rl >> 4)) * MX8_DG_SPITCH + hh * 8;
#pragma unroll
        for (int ns = 0; ns < MX8_DG_BN / 16; ns++) {
            typename F::t a[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX8_DG_APITCH + ns * 32 + hh * 16));
            const uint4_t w = *reinterpret_cast<const uint4_t*>(bcol + ns * 32);
            const float4_t s0 = *reinterpret_cast<const float4_t*>(scol + ns * 16), s1 = *reinterpret_cast<const float4_t*>(scol + ns * 16 + 4);
            typename F::t b0, b1;  // output columns 2 rl and 2 rl + 1 of the wave's 64
            mx8_frag_columns<DT>(w, s0, s1, b0, b1);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                acc[i][0] = F::mfma(a[i], b0, acc[i][0]);
                acc[i][1] = F::mfma(a[i], b1, acc[i][1]);
            }
        }
        if (nt + 1 < NT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: lane column rl = output columns k0 + wx 64 + 2 rl (acc[.][0]) and + 1 (acc[.][1]), tile row (r & 3) + 8 (r >> 2) + 4 hh
    const int k = k0 + wx * 64 + 2 * rl;
    if (k >= K) return;  // K % 32 == 0 and k is even: the pair lies inside K or outside
    const float cs = e8m0_f32(eblk[k >> 5]);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (rows.live(row)) mx_store2<ODT>(gx, rows.dst(row) * K + k, acc[i][0][r] * cs, acc[i][1][r] * cs);
        }
}

}  // namespace bie
