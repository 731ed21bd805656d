// The MXFP8 (OCP microscaling FP8, E4M3 elements) weight-only (W8A16) device-side rules (gfx950): the two-at-a-time convert of code bytes
// to exact 16-bit values and the 128 x 128 prefill tile body (mx8_gemm_tile: mx8_gemm_kernel of mxfp8.hip).  The E8M0 block scales, the
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

}  // namespace bie
