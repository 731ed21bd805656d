// The MXFP4 format's device-side rules and everything the MXFP4 translation units share (gfx950): E8M0 scale codes to fp32, the
// quantiser's rounding and block-scale rules, the fp4 -> fp16 / bf16 converts with their dot2 and MFMA, the fp32 wave sum on the DPP
// network, the row sources of the tile GEMMs, the weight-only 128 x 128 tile body (mx_gemm_tile: mx_gemm_kernel of mxfp4.hip and
// mxm_gemm_kernel of mxfp4_moe.hip), the input-gradient 128 x 128 tile body (mx_dgrad_tile: the kernels of mxfp4_grad.hip), and the
// routing workspace of the grouped expert GEMMs with their common prologue (mxm_tile_begin).
#pragma once
#include "mfma_pipe.cuh"

namespace bie {

typedef __bf16 mx_bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 mx_half8_t __attribute__((ext_vector_type(8)));

// E8M0 -> fp32: 2^(s - 127), code 0 the subnormal 2^-127 (not 0.0), code 255 NaN (not +inf, which the plain s << 23 would give)
__device__ __forceinline__ float e8m0_f32(uint32_t s) { return __uint_as_float(s == 0u ? 0x00400000u : s == 255u ? 0x7fc00000u : s << 23); }

// 2^d for d <= 0 as the convert's scale: 0 below 2^-126 (e2m1 * 2^d then lies below every fp16 / bf16 normal the fragments keep)
__device__ __forceinline__ float mx_rebias(uint32_t s, uint32_t e) {
    const int d = (int)s - (int)e;
    return __uint_as_float(d < -126 ? 0u : (uint32_t)(d + 127) << 23);
}

// |a| -> E2M1 magnitude index, round to nearest, ties to the even index (0.25 -> 0, 0.75 -> 2, 1.25 -> 2, 1.75 -> 4, 2.5 -> 4, 3.5 -> 6,
// 5 -> 6), saturating at 6
__device__ __forceinline__ uint32_t mx_round_e2m1(float a) {
    return a <= 0.25f ? 0u : a < 0.75f ? 1u : a <= 1.25f ? 2u : a < 1.75f ? 3u : a <= 2.5f ? 4u : a < 3.5f ? 5u : a <= 5.0f ? 6u : 7u;
}

// A block's scale from its largest magnitude amax > 0: e = floor(log2 amax) - 2 clamped to [-127, 127] (from the fp32 exponent bits,
// a subnormal amax by its leading bit).  Returns the E8M0 code e + 127 and sets inv = 2^-e (normal: e <= 125 for any finite amax), so
// that w * inv is exact: a power-of-two multiply of a normal result.
__device__ __forceinline__ uint32_t mx_block_scale(float amax, float& inv) {
    const uint32_t bits = __float_as_uint(amax);
    const int ex = (int)(bits >> 23);
    const int fl = ex ? ex - 127 : (31 - __builtin_clz(bits & 0x7fffffu)) - 149;  // floor(log2(amax))
    const int e = min(max(fl - 2, -127), 127);
    inv = __uint_as_float((uint32_t)(127 - e) << 23);
    return (uint32_t)(e + 127);
}

// ---- decode forms: two codes -> two exact 16-bit values (scale 1.0), dot2 into fp32 -----------------------------------------------------
template <int DT> struct mx_pair;
template <> struct mx_pair<BIE_BF16> {
    typedef bf16x2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, SEL); }
    static __device__ __forceinline__ float dot(t a, uint32_t b, float c) { return __builtin_amdgcn_fdot2_f32_bf16(a, __builtin_bit_cast(t, b), c, false); }
};
template <> struct mx_pair<BIE_F16> {
    typedef half2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, SEL); }
    static __device__ __forceinline__ float dot(t a, uint32_t b, float c) { return __builtin_amdgcn_fdot2(a, __builtin_bit_cast(t, b), c, false); }
};

// 16 codes (two dwords) -> eight pairs of exact 16-bit values
template <int DT>
__device__ __forceinline__ void mx_unpack16(const uint2_t& w, typename mx_pair<DT>::t (&v)[8]) {
    typedef mx_pair<DT> P;
    v[0] = P::template cvt<0>(w.x); v[1] = P::template cvt<1>(w.x);
    v[2] = P::template cvt<2>(w.x); v[3] = P::template cvt<3>(w.x);
    v[4] = P::template cvt<0>(w.y); v[5] = P::template cvt<1>(w.y);
    v[6] = P::template cvt<2>(w.y); v[7] = P::template cvt<3>(w.y);
}

template <int CTRL, int RMASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, RMASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_f32(float v) {  // wave_sum_dpp's network (bie_common.h) on fp32; the total of lane 63
    v = dpp_add<0xB1, 0xf>(v);
    v = dpp_add<0x4E, 0xf>(v);
    v = dpp_add<0x141, 0xf>(v);
    v = dpp_add<0x140, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- prefill forms: four code bytes -> one 8-k MFMA fragment at the block's rebiased scale ---------------------------------------------
template <int DT> struct mx_frag;
template <> struct mx_frag<BIE_BF16> {
    typedef mx_bf16x8_t t;
    static __device__ __forceinline__ t cvt(uint32_t w, float s) {
        const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
        const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
        return t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ float16_t mfma(const t& a, const t& b, const float16_t& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct mx_frag<BIE_F16> {
    typedef mx_half8_t t;
    static __device__ __forceinline__ t cvt(uint32_t w, float s) {
        const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 1);
        const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 3);
        return t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ float16_t mfma(const t& a, const t& b, const float16_t& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// ---- where the rows of a tile come from ------------------------------------------------------------------------------------------------
// A tile GEMM body asks its row source, for tile row r: whether the row is live (a dead row loads as zero and is not stored), which
// stored row of x (or of xq / xs / row_flag) it reads, and which row of y it writes.  src and dst are asked of live rows only.
struct mx_rows_dense {  // rows m0 .. of an [M, K] x, written to the same rows of y
    int m0, M;
    __device__ __forceinline__ bool live(int r) const { return m0 + r < M; }
    __device__ __forceinline__ long src(int r) const { return m0 + r; }
    __device__ __forceinline__ long dst(int r) const { return m0 + r; }
};
struct mx_rows_listed {  // the pairs of a row tile of the grouped expert GEMMs: prow[] in LDS (-1 past the segment), pair p writes y[p]
    const int* prow;
    int S, x_per_pair;
    __device__ __forceinline__ bool live(int r) const { return prow[r] >= 0; }
    __device__ __forceinline__ long src(int r) const { return x_per_pair ? prow[r] : prow[r] / S; }
    __device__ __forceinline__ long dst(int r) const { return prow[r]; }
};

// ---- the weight-only prefill tile ----------------------------------------------------------------------------------------------------------
constexpr int MX_BM = 128, MX_BN = 128, MX_BK = 64;
constexpr int MX_APITCH = MX_BK * 2 + 16;  // bytes per x row in LDS (16-byte pad: the fragment reads of 32 rows spread over the banks)
constexpr int MX_BPITCH = 36;              // bytes per weight row: 32 code bytes + 4 (9 dwords, the 32 rows of a read on distinct banks)
constexpr int MX_STAGE = MX_BM * MX_APITCH + MX_BN * MX_BPITCH + MX_BN * 2 * 4;  // x, codes, the two fp32 rebiased scales per row

// One 128 x 128 tile of y = x . W^T (+ bias) on v_mfma_f32_32x32x16_{bf16,f16}: tile rows from `rows`, columns n0 .. of the N weight
// rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for expert e).  4 waves as 2 x 2, wave tile 64 x 64 (2 x 2 MFMA
// tiles).  Per 64-k stage a thread loads 4 x 16 bytes of x, 16 code bytes and one scale byte into registers while the MFMAs run on the
// other LDS buffer, then writes them (the scale already rebiased to fp32).  The weight tile is staged packed and converted to B
// fragments after the LDS read: a lane's 8-k fragment is 4 code bytes = 4 converts.  Dead rows and whatever lies past N / K: x and
// codes load as zero, scales as 1.0, so the padding adds exact zeros.  All 256 threads of the workgroup must call it together.
template <int DT, class Rows>
__device__ __forceinline__ void mx_gemm_tile(const Rows& rows, const uint16_t* __restrict__ x, const uint8_t* __restrict__ qw,
                                             const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol, const void* __restrict__ bias,
                                             void* __restrict__ y, long r0, int n0, int N, int K) {
    typedef mx_frag<DT> F;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX_STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KT = (K + MX_BK - 1) / MX_BK, KB = K >> 5;

    // this thread's load slots
    const int bn = t >> 1, bh = t & 1;  // weight row bn of the tile, 16-byte half bh; scale block bh of the stage
    const int nb = n0 + bn;
    const bool nb_ok = nb < N;
    const uint8_t* wsrc = qw + (r0 + min(nb, N - 1)) * (K >> 1) + bh * 16;
    const uint8_t* ssrc = sc + (r0 + min(nb, N - 1)) * KB + bh;
    const uint32_t e = nb_ok ? ecol[r0 + nb] : 0u;
    const uint16_t* xrow[4];  // the x rows of this thread's four 16-byte pieces per stage: tile row (t + 256 i) / 8, piece t & 7
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = (t + 256 * i) >> 3;
        xrow[i] = rows.live(row) ? x + rows.src(row) * K + (t & 7) * 8 : nullptr;
    }
    uint4_t ra[4], rb;
    float rs;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            ra[i] = (xrow[i] && kt * MX_BK + (t & 7) * 8 < K) ? *reinterpret_cast<const uint4_t*>(xrow[i] + kt * MX_BK) : uint4_t{0u, 0u, 0u, 0u};
        const bool kin = kt * MX_BK + bh * 32 < K;
        rb = (nb_ok && kin) ? __builtin_nontemporal_load(reinterpret_cast<const uint4_t*>(wsrc + kt * 32)) : uint4_t{0u, 0u, 0u, 0u};
        rs = (nb_ok && kin) ? mx_rebias(__builtin_nontemporal_load(ssrc + kt * 2), e) : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX_STAGE;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 256 * i, row = q >> 3, c16 = q & 7;
            *reinterpret_cast<uint4_t*>(st + row * MX_APITCH + c16 * 16) = ra[i];
        }
        uint32_t* wb = reinterpret_cast<uint32_t*>(st + MX_BM * MX_APITCH + bn * MX_BPITCH + bh * 16);
        wb[0] = rb.x; wb[1] = rb.y; wb[2] = rb.z; wb[3] = rb.w;
        reinterpret_cast<float*>(st + MX_BM * MX_APITCH + MX_BN * MX_BPITCH)[bn * 2 + bh] = rs;
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
        const unsigned char* st = lds + buf * MX_STAGE;
        const float* ss = reinterpret_cast<const float*>(st + MX_BM * MX_APITCH + MX_BN * MX_BPITCH);
#pragma unroll
        for (int ks = 0; ks < MX_BK / 16; ks++) {
            typename F::t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX_APITCH + ks * 32 + hh * 16));
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int n = wx * 64 + j * 32 + rl;
                const uint32_t w = *reinterpret_cast<const uint32_t*>(st + MX_BM * MX_APITCH + n * MX_BPITCH + ks * 8 + hh * 4);
                b[j] = F::cvt(w, ss[n * 2 + (ks >> 1)]);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = F::mfma(a[i], b[j], acc[i][j]);
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: column n = lane & 31, tile row (r & 3) + 8 (r >> 2) + 4 hh
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int n = n0 + wx * 64 + j * 32 + rl;
        if (n >= N) continue;
        const float cs = e8m0_f32(ecol[r0 + n]);
        const float bv = bias ? dt_traits<DT>::load(bias, r0 + n) : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (rows.live(row)) {
                    float v = acc[i][j][r] * cs;
                    if (bias) v += bv;
                    dt_traits<DT>::store(y, rows.dst(row) * N + n, v);
                }
            }
    }
}

// ---- the input-gradient tile -----------------------------------------------------------------------------------------------------------------
constexpr int MX_DG_BM = 128, MX_DG_BK = 128, MX_DG_BN = 64;  // rows of gy, columns k of gx, contraction rows n of a stage
constexpr int MX_DG_APITCH = MX_DG_BN * 2 + 16;               // bytes per gy row in LDS (MX_APITCH's pad)
constexpr int MX_DG_BPITCH = MX_DG_BN + 8;  // bytes per byte-column of codes: 64 n + 8 (18 dwords: the 8-byte reads of 32 lanes on distinct bank pairs)
constexpr int MX_DG_SPITCH = MX_DG_BN + 4;  // fp32 per block-column of rebiased scales: 64 n + 4 (the two block-columns a half-wave reads on distinct banks)
constexpr int MX_DG_STAGE = MX_DG_BM * MX_DG_APITCH + (MX_DG_BK / 2) * MX_DG_BPITCH + (MX_DG_BK / 32) * MX_DG_SPITCH * 4;

// Eight code bytes of one byte column (rows n .. n + 7, byte j of w0 / w1) at their rows' rebiased scales -> the 8-n fragments of the
// bytes' low nibbles (column 2 c) and high nibbles (column 2 c + 1): one convert per byte, the halves regrouped.
template <int DT> struct mx_cvt2;
template <> struct mx_cvt2<BIE_BF16> {
    typedef bf16x2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w, float s) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, SEL); }
};
template <> struct mx_cvt2<BIE_F16> {
    typedef half2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w, float s) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, SEL); }
};
template <int DT>
__device__ __forceinline__ void mx_frag_columns(uint32_t w0, uint32_t w1, const float4_t& s0, const float4_t& s1, typename mx_frag<DT>::t& lo,
                                                typename mx_frag<DT>::t& hi) {
    typedef mx_cvt2<DT> C;
    const typename C::t v0 = C::template cvt<0>(w0, s0[0]), v1 = C::template cvt<1>(w0, s0[1]);
    const typename C::t v2 = C::template cvt<2>(w0, s0[2]), v3 = C::template cvt<3>(w0, s0[3]);
    const typename C::t v4 = C::template cvt<0>(w1, s1[0]), v5 = C::template cvt<1>(w1, s1[1]);
    const typename C::t v6 = C::template cvt<2>(w1, s1[2]), v7 = C::template cvt<3>(w1, s1[3]);
    lo = typename mx_frag<DT>::t{v0[0], v1[0], v2[0], v3[0], v4[0], v5[0], v6[0], v7[0]};
    hi = typename mx_frag<DT>::t{v0[1], v1[1], v2[1], v3[1], v4[1], v5[1], v6[1], v7[1]};
}

// two adjacent output columns (i even) in one store
template <int ODT>
__device__ __forceinline__ void mx_store2(void* p, long i, float v0, float v1) {
    if constexpr (ODT == BIE_F32) *reinterpret_cast<float2_t*>(reinterpret_cast<float*>(p) + i) = float2_t{v0, v1};
    else if constexpr (ODT == BIE_BF16) reinterpret_cast<uint32_t*>(p)[i >> 1] = pack_bf16x2(v0, v1);
    else reinterpret_cast<uint32_t*>(p)[i >> 1] = f32_to_f16_bits(v0) | (f32_to_f16_bits(v1) << 16);
}

// One 128 x 128 tile of gx = gy . W on v_mfma_f32_32x32x16_{bf16,f16}, contracted over the N weight rows that start at row r0 of qw / sc
// (0, or (long)e * N for expert e): tile rows from `rows` (a live row reads gy[src] and writes gx[dst]), columns k0 .. of K, rebiased by
// eblk[k / 32] (the caller's pointer already at the expert's K / 32 codes).  ODT, the element type of gx, is DT or BIE_F32.  4 waves as
// 2 x 2, wave tile 64 x 64.  Per stage of 64 n a thread loads 4 x 16 bytes of gy, four dwords of codes (rows 4 n4 .. + 3, byte columns
// 4 d .. + 3) and one scale byte into registers while the MFMAs run on the other LDS buffer, then writes them: the codes TRANSPOSED
// (a 4 x 4 byte transpose in registers; LDS holds [byte column][n]) and the scale rebiased to fp32 as [block-column][n].  Lane
// (r = lane & 31, h = lane >> 5) of a 16-n step then reads the 8 bytes of byte column r, rows 8 h .. + 7, in one ds_read_b64 and their 8
// scales in two ds_read_b128; each byte is one convert at its row's scale (a byte = the adjacent output columns 2 r, 2 r + 1); the 8
// low halves and the 8 high halves are the B fragments of two MFMAs whose output column for lane r is k0 + 2 r and k0 + 2 r + 1, so the
// epilogue stores two adjacent columns per lane.  gy rows have any length N: whole 16-byte pieces where `vec` (N % 8 == 0 and gy
// 16-byte aligned), else 16-bit loads, each guarded by n < N.  Dead rows and whatever lies past N / K: gy and codes load as zero,
// scales as 1.0, so the padding adds exact zeros.  All 256 threads of the workgroup must call it together.
template <int DT, int ODT, class Rows>
__device__ __forceinline__ void mx_dgrad_tile(const Rows& rows, const uint16_t* __restrict__ gy, const uint8_t* __restrict__ qw,
                                              const uint8_t* __restrict__ sc, const uint8_t* __restrict__ eblk, void* __restrict__ gx, long r0,
                                              int k0, int N, int K, bool vec) {
    typedef mx_frag<DT> F;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * MX_DG_STAGE];
    constexpr int B_OFF = MX_DG_BM * MX_DG_APITCH, S_OFF = B_OFF + (MX_DG_BK / 2) * MX_DG_BPITCH;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int NT = (N + MX_DG_BN - 1) / MX_DG_BN, KB = K >> 5, KH = K >> 1;

    // this thread's load slots
    const int bd = t & 15, bn4 = t >> 4;  // codes: dword bd of the tile's 64 byte columns, rows 4 bn4 .. + 3 of the stage
    const bool bk_ok = (k0 >> 1) + bd * 4 < KH;
    const uint8_t* wsrc = qw + r0 * KH + (k0 >> 1) + bd * 4;
    const int sn = t >> 2, sb = t & 3;  // scale: row sn of the stage, block-column sb of the tile
    const bool sb_ok = (k0 >> 5) + sb < KB;
    const uint8_t* ssrc = sc + r0 * KB + (k0 >> 5) + sb;
    const uint32_t eb = sb_ok ? eblk[(k0 >> 5) + sb] : 0u;
    const uint16_t* grow[4];  // the gy rows of this thread's four 16-byte pieces per stage: tile row (t + 256 i) / 8, piece t & 7
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = (t + 256 * i) >> 3;
        grow[i] = rows.live(row) ? gy + rows.src(row) * N : nullptr;
    }
    uint4_t ra[4];
    uint32_t rb[4];
    float rs;
    auto load = [&](int nt) {
        const int na = nt * MX_DG_BN + (t & 7) * 8;  // the first n of this thread's pieces
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
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = nt * MX_DG_BN + bn4 * 4 + i;
            rb[i] = (bk_ok && n < N) ? *reinterpret_cast<const uint32_t*>(wsrc + (long)n * KH) : 0u;
        }
        const int n = nt * MX_DG_BN + sn;
        rs = (sb_ok && n < N) ? mx_rebias(ssrc[(long)n * KB], eb) : 1.0f;
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * MX_DG_STAGE;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 256 * i, row = q >> 3, c16 = q & 7;
            *reinterpret_cast<uint4_t*>(st + row * MX_DG_APITCH + c16 * 16) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {  // byte column 4 bd + i of rows 4 bn4 .. + 3
            const uint32_t w = ((rb[0] >> (8 * i)) & 0xffu) | (((rb[1] >> (8 * i)) & 0xffu) << 8) | (((rb[2] >> (8 * i)) & 0xffu) << 16) |
                               (((rb[3] >> (8 * i)) & 0xffu) << 24);
            *reinterpret_cast<uint32_t*>(st + B_OFF + (bd * 4 + i) * MX_DG_BPITCH + bn4 * 4) = w;
        }
        reinterpret_cast<float*>(st + S_OFF)[sb * MX_DG_SPITCH + sn] = rs;
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
        const unsigned char* st = lds + buf * MX_DG_STAGE;
        const unsigned char* bcol = st + B_OFF + (wx * 32 + rl) * MX_DG_BPITCH + hh * 8;
        const float* scol = reinterpret_cast<const float*>(st + S_OFF) + (wx * 2 + (rl >> 4)) * MX_DG_SPITCH + hh * 8;
#pragma unroll
        for (int ns = 0; ns < MX_DG_BN / 16; ns++) {
            typename F::t a[2];
#pragma unroll
            for (int i = 0; i < 2; i++)
                a[i] = __builtin_bit_cast(typename F::t, *reinterpret_cast<const uint4_t*>(st + (wy * 64 + i * 32 + rl) * MX_DG_APITCH + ns * 32 + hh * 16));
            const uint2_t w = *reinterpret_cast<const uint2_t*>(bcol + ns * 16);
            const float4_t s0 = *reinterpret_cast<const float4_t*>(scol + ns * 16), s1 = *reinterpret_cast<const float4_t*>(scol + ns * 16 + 4);
            typename F::t b0, b1;  // output columns 2 rl and 2 rl + 1 of the wave's 64
            mx_frag_columns<DT>(w.x, w.y, s0, s1, b0, b1);
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

// ---- the routing workspace of the grouped expert GEMMs (mxm_route_kernel of mxfp4_moe.hip writes it; mxfp4_moe.hip and mxfp4_moe_a4.hip read it)
// int32: head [MXM_HEAD], tile_expert [max_tiles], tile_first [max_tiles], tile_rows [max_tiles], pair list [P]
constexpr int MXM_BM = 128;      // rows of a row tile
constexpr int MXM_MAX_E = 1024;  // bins of the routing kernel's scan
constexpr int MXM_HEAD = 4;      // int32 words before the tile table: [0] the tile count

// The start of a grouped GEMM workgroup: its (row tile, column tile of BN columns), the row tile's expert e and first column n0, and
// the tile's pairs in prow[MXM_BM] (LDS; -1 past the segment), published by a barrier.  Workgroup -> tile: the workgroups of one XCD
// (blockIdx.x & 7) walk the row tiles of one column tile after another, so the tiles of one expert, which follow each other in the
// table, find the expert's BN columns of weights in that XCD's L2.  Returns false where the workgroup has no GEMM to run: a surplus
// workgroup (beyond the tile count the routing kernel wrote), or a tile of the skipped bin, whose rows of y it has then zeroed.  Both
// exits are workgroup-uniform and come before any address is formed from e.
template <int DT, int BN>
__device__ __forceinline__ bool mxm_tile_begin(const int32_t* __restrict__ ws, int max_tiles, int E, int N, void* __restrict__ y, int* prow, int& e, int& n0) {
    const int t = threadIdx.x;
    int bid = blockIdx.x;
    {
        const int nblk = gridDim.x, xcd = bid & 7, per = nblk >> 3, rem = nblk & 7;
        bid = xcd * per + (xcd < rem ? xcd : rem) + (bid >> 3);
    }
    const int tile_m = bid % max_tiles, tile_n = bid / max_tiles;
    if (tile_m >= ws[0]) return false;
    e = ws[MXM_HEAD + tile_m];
    const int first = ws[MXM_HEAD + max_tiles + tile_m], nrows = ws[MXM_HEAD + 2 * max_tiles + tile_m];
    const int32_t* list = ws + MXM_HEAD + 3 * (long)max_tiles;
    if (t < MXM_BM) prow[t] = t < nrows ? list[first + t] : -1;
    __syncthreads();
    n0 = tile_n * BN;
    if (e < E) return true;
    for (int i = t; i < MXM_BM * BN; i += 256) {
        const int p = prow[i / BN], n = n0 + i % BN;
        if (p >= 0 && n < N) dt_traits<DT>::store(y, (long)p * N + n, 0.0f);
    }
    return false;
}

}  // namespace bie
