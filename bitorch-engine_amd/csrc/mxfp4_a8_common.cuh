// The device-side pieces of the W4A8 translation units (mxfp4_a8.hip, mxfp4_moe_a8.hip; gfx950): the MXFP8 (E4M3)
// activation quantiser's rule for one 8-value unit, so that a kernel that quantises a row itself (mxma8_decode_kernel) produces the
// bits of mxa8_quantize_kernel, and the prefill tile body on v_mfma_scale_f32_32x32x64_f8f6f4 with an FP4 A operand and an E4M3 B operand
// (mxa8_gemm_tile: mxa8_gemm_kernel of mxfp4_a8.hip and mxma8_gemm_kernel of mxfp4_moe_a8.hip; it takes the row sources of mxfp4_common.cuh like mxa4_gemm_tile).
#pragma once
#include "mxfp4_a4_common.cuh"

namespace bie {

// The instruction's 8-VGPR E4M3 operand from its two 16-byte halves.  With an FP4 partner the halves are NOT one block of 32
// (tools/probe/probe_mx_a8.hip, profiles/mxfp4_a8_probe.txt): of the G = 2 (32x32x64) or 4 (16x16x128) lane groups, group g holds in
// bytes 0 .. 15 the elements k = 16 g .. 16 g + 15 of the instruction's K and in bytes 16 .. 31 the elements k = 16 G + 16 g .. + 15,
// while the FP4 operand of group g holds k = 32 g .. 32 g + 31 and the scale byte of group g applies to block g (k = 32 g .. + 31) on
// either operand.  xq stays row-major in memory: a lane takes its halves from two places of the row, nothing is permuted in registers.
__device__ __forceinline__ mxa4_v8i a8_frag(const uint4_t& lo, const uint4_t& hi) {
    return mxa4_v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// A block's scale from its largest magnitude amax > 0 with E4M3 elements (emax = 8): mx_block_scale's rule with - 8 in place of - 2.
// e <= 119 for any finite amax, so inv = 2^-e is normal and v * inv an exact power-of-two multiply.
__device__ __forceinline__ uint32_t mxa8_block_scale(float amax, float& inv) {
    const uint32_t bits = __float_as_uint(amax);
    const int ex = (int)(bits >> 23);
    const int fl = ex ? ex - 127 : (31 - __builtin_clz(bits & 0x7fffffu)) - 149;  // floor(log2(amax))
    const int e = min(max(fl - 8, -127), 127);
    inv = __uint_as_float((uint32_t)(127 - e) << 23);
    return (uint32_t)(e + 127);
}

// v * inv -> the value handed to the convert: magnitude clamped to 448 (the largest E4M3 value) here, so that the result does not depend
// on the convert's overflow mode and no NaN code is ever produced; the sign of v is kept (-0.0 -> 0x80).
__device__ __forceinline__ float a8_clamp(float v, float inv) {
    return __uint_as_float(__float_as_uint(fminf(fabsf(v * inv), 448.0f)) | (__float_as_uint(v) & 0x80000000u));
}

// One 8-value unit (16 bytes of x) of a block of 32 whose four units sit on the four lanes of a quad: the block maximum over the quad on
// the DPP network, the block's E8M0 code and this lane's 8 bytes of E4M3 codes (round to nearest even, OCP e4m3fn).  `bad` collects a NaN
// or +-inf.  All lanes of the quad must call it together.
template <int DT>
__device__ __forceinline__ void a8_quantize_unit(const uint4_t& raw, int& bad, uint2_t& codes, uint32_t& scode) {
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
    codes = uint2_t{0u, 0u};
    scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mxa8_block_scale(amax, inv);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[0], inv), a8_clamp(v[1], inv), lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[2], inv), a8_clamp(v[3], inv), lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[4], inv), a8_clamp(v[5], inv), hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[6], inv), a8_clamp(v[7], inv), hi, true);
        codes = uint2_t{(uint32_t)lo, (uint32_t)hi};
    }
}

// ---- the W4A8 prefill tile ------------------------------------------------------------------------------------------------------------------
constexpr int A8_BK = 128;               // k per stage: 128 x bytes, 64 weight code bytes and 4 scale bytes per row
constexpr int A8_XPITCH = A8_BK + 16;    // 144 bytes per x row in LDS (36 dwords): the 16-byte fragment reads of 16 rows fall on distinct banks
constexpr int A8_WPITCH = A8_BK / 2 + 16;  // 80 bytes per weight row (20 dwords): likewise

// One (64 WM rows) x (64 WN columns) tile of the W4A8 product: tile rows from `rows` (mxfp4_common.cuh; they index xq / xs / row_flag),
// columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for an expert e).  4 waves as 2 x 2;
// per 64 k a wave reads WM x fragments (two 16-byte reads 32 bytes apart, see a8_frag) and WN weight fragments (16 bytes) with as many scale bytes and
// issues WM * WN MFMAs.  The weight fragment is the A operand (FP4, cbsz 4) and the x fragment the B operand (E4M3, blgp 0), so a lane's
// accumulator holds 4 consecutive columns of one row of y.  LDS stage, double-buffered and filled through registers: x codes
// [64 WM][144], weight codes [64 WN][80], x scales [64 WM] dwords, weight scales [64 WN] dwords (byte j of a row's dword = the scale of
// the stage's block j): 29696 bytes at WM = WN = 2, so 59392 bytes (58 KB) of static LDS for the two buffers, and 29696 bytes for the two
// at WM = WN = 1.  Dead rows and
// whatever lies past N / K: zero codes under scale 2^0.  All 256 threads must call it together.
template <int DT, int WM, int WN, class Rows>
__device__ __forceinline__ void mxa8_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                               const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                               const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                               int N, int K) {
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN;
    constexpr int XLD = BM * 8 / 256, WLD = BN * 4 / 256;  // 16-byte pieces per thread and stage: x row = piece / 8, weight row = piece / 4
    constexpr int WOFF = BM * A8_XPITCH, SOFF = WOFF + BN * A8_WPITCH;
    constexpr int STAGE = SOFF + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + A8_BK - 1) / A8_BK;

    // load slots: x pieces t, t + 256, ... (8 per row: block (piece & 7) >> 1 of the stage, half piece & 1), then weight pieces (4 per
    // row: block piece & 3); thread t < ROWS also loads the scales of row t of the stage image (rows 0 .. BM - 1 = x, BM .. = weights)
    const uint8_t* xsrc[XLD];
    const uint8_t* wsrc[WLD];
    bool xok[XLD], wok[WLD];
#pragma unroll
    for (int i = 0; i < XLD; i++) {
        const int row = (t + 256 * i) >> 3;
        xok[i] = rows.live(row);
        xsrc[i] = xq + (xok[i] ? rows.src(row) : 0L) * K + (t & 1) * 16;
    }
#pragma unroll
    for (int i = 0; i < WLD; i++) {
        const int row = (t + 256 * i) >> 2;
        wok[i] = n0 + row < N;
        wsrc[i] = qw + (r0 + min(n0 + row, N - 1)) * (K >> 1);
    }
    const bool s_thread = ROWS == 256 || t < ROWS;
    bool sok = false;
    const uint8_t* ssrc = xs;
    if (s_thread) {
        if (t < BM) {
            sok = rows.live(t);
            ssrc = xs + (sok ? rows.src(t) : 0L) * KB;
        } else {
            sok = n0 + t - BM < N;
            ssrc = sc + (r0 + min(n0 + t - BM, N - 1)) * KB;
        }
    }
    uint4_t rx[XLD], rw[WLD];
    uint32_t rs = 0x7f7f7f7fu;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < XLD; i++) {
            const int kb = kt * 4 + ((t & 7) >> 1);
            rx[i] = (xok[i] && kb < KB) ? *reinterpret_cast<const uint4_t*>(xsrc[i] + (long)kb * 32) : uint4_t{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < WLD; i++) {
            const int kb = kt * 4 + (t & 3);
            rw[i] = (wok[i] && kb < KB) ? *reinterpret_cast<const uint4_t*>(wsrc[i] + (long)kb * 16) : uint4_t{0u, 0u, 0u, 0u};
        }
        if (s_thread) {
            rs = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int kb = kt * 4 + j;
                const uint32_t s = (sok && kb < KB) ? (uint32_t)ssrc[kb] : 127u;
                rs |= s << (8 * j);
            }
        }
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < XLD; i++) {
            const int p = t + 256 * i;
            *reinterpret_cast<uint4_t*>(st + (p >> 3) * A8_XPITCH + (p & 7) * 16) = rx[i];
        }
#pragma unroll
        for (int i = 0; i < WLD; i++) {
            const int p = t + 256 * i;
            *reinterpret_cast<uint4_t*>(st + WOFF + (p >> 2) * A8_WPITCH + (p & 3) * 16) = rw[i];
        }
        if (s_thread) reinterpret_cast<uint32_t*>(st + SOFF)[t] = rs;
    };

    float16_t acc[WN][WM];  // [weight row block j][x row block i]: D rows = columns n of y, D columns = rows of the tile
#pragma unroll
    for (int j = 0; j < WN; j++)
#pragma unroll
        for (int i = 0; i < WM; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][i][r] = 0.0f;

    const int rl = lane & 31, hh = lane >> 5;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load(kt + 1);
        const unsigned char* st = lds + buf * STAGE;
        const uint32_t* ss = reinterpret_cast<const uint32_t*>(st + SOFF);
        uint32_t sxa[WM], swa[WN];  // the row's four scale bytes, shifted so that this lane's block of k-step ks sits in byte 2 ks
#pragma unroll
        for (int i = 0; i < WM; i++) sxa[i] = ss[wy * 32 * WM + i * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int j = 0; j < WN; j++) swa[j] = ss[BM + wx * 32 * WN + j * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            mxa4_v8i fx[WM], fw[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) {
                const uint4_t* p = reinterpret_cast<const uint4_t*>(st + (wy * 32 * WM + i * 32 + rl) * A8_XPITCH + ks * 64 + hh * 16);
                fx[i] = a8_frag(p[0], p[2]);  // k 16 hh .. + 15 of the step's first block and of its second (a8_frag)
            }
#pragma unroll
            for (int j = 0; j < WN; j++)
                fw[j] = a4_frag(*reinterpret_cast<const uint4_t*>(st + WOFF + (wx * 32 * WN + j * 32 + rl) * A8_WPITCH + (ks * 2 + hh) * 16));
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], 4, 0, 0, (int)((swa[j] >> (16 * ks)) & 0xffu), 0,
                                                                                (int)((sxa[i] >> (16 * ks)) & 0xffu));
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: D column (= tile row) = lane & 31, D row (= column n of y) = (r & 3) + 8 (r >> 2) + 4 hh: registers 4q .. 4q + 3 are four
    // consecutive n of one row -> one 8-byte store where N allows it.  A flagged row of x and a column with e_col = 255 are NaN; the bias
    // is added after that, as in mxa4_gemm_tile.
    const bool vec = (N & 3) == 0;
#pragma unroll
    for (int i = 0; i < WM; i++) {
        const int row = wy * 32 * WM + i * 32 + rl;
        if (!rows.live(row)) continue;
        const bool rbad = row_flag[rows.src(row)] != 0;
        uint16_t* yr = reinterpret_cast<uint16_t*>(y) + rows.dst(row) * N;
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int n = n0 + wx * 32 * WN + j * 32 + 8 * q + 4 * hh;
                if (n >= N) continue;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    v[r] = acc[j][i][4 * q + r];
                    if (n + r < N) {
                        if (rbad || ecol[r0 + n + r] == 255u) v[r] = a4_nan();
                        if (bias) v[r] += dt_traits<DT>::load(bias, r0 + n + r);
                    }
                }
                if (vec) {
                    uint16_t h[4];
                    dt_traits<DT>::store(h, 0, v[0]); dt_traits<DT>::store(h, 1, v[1]);
                    dt_traits<DT>::store(h, 2, v[2]); dt_traits<DT>::store(h, 3, v[3]);
                    uint2_t o;
                    o.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
                    o.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
                    *reinterpret_cast<uint2_t*>(yr + n) = o;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (n + r < N) dt_traits<DT>::store(yr, n + r, v[r]);
                }
            }
    }
}

}  // namespace bie
