// The MXFP6 (OCP microscaling FP6, E2M3 elements) format's device-side rules and the W6A8 prefill tile body (gfx950): the quantiser's
// rounding rule, code <-> fp32, a block's 24 bytes <-> its 32 codes, the FP6 operand of the block-scaled matrix instructions, and
// mx6a8_gemm_tile on v_mfma_scale_f32_32x32x64_f8f6f4 with an FP6 A operand (cbsz 2) and an E4M3 B operand (blgp 0).  The E8M0 block
// scales, the block-scale rule (mx_block_scale: emax = 2 for E2M3 as for E2M1), the row sources and the MXFP8 activations are those of
// mxfp4_common.cuh / mxfp4_a8_common.cuh.
//
// A block of 32 codes is 24 bytes: code j in bits 6 j .. 6 j + 5 of the block's little-endian 192-bit integer, which is the order in
// which the instructions read a lane's six operand registers (tools/probe/probe_mx_fp6.hip part (a2), profiles/mxfp6_a8_probe.txt), so
// a lane's fragment is a plain 24-byte copy.  Code bits: bit 5 sign, bits 4:3 exponent (bias 1), bits 2:0 mantissa; no Inf / NaN code.
#pragma once
#include "mxfp4_a8_common.cuh"

namespace bie {

constexpr int MX6_BLOCK_BYTES = 24;

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

// the instruction's FP6 operand (six of the eight registers) from a block's three 8-byte pieces
__device__ __forceinline__ mxa4_v8i a6_frag(const uint2_t& p0, const uint2_t& p1, const uint2_t& p2) {
    return mxa4_v8i{(int)p0.x, (int)p0.y, (int)p1.x, (int)p1.y, (int)p2.x, (int)p2.y, 0, 0};
}

// ---- the W6A8 prefill tile ------------------------------------------------------------------------------------------------------------------
constexpr int A6_BK = 128;                // k per stage: 128 x bytes, 96 weight code bytes and 4 scale bytes per row
constexpr int A6_WROW = A6_BK / 32 * 24;  // 96
// 104 bytes per weight row in LDS (26 dwords).  A lane's fragment is the 24 bytes at row * 104 + 24 * block, three 8-byte reads (a row
// is only 8-byte aligned, in memory as here).  The lanes of a half-wave read the same block of rows r = 0 .. 31: per piece the dwords
// 26 r + c and 26 r + c + 1.  As ds_read_b64 (served per 32 lanes, bank = dword mod 64): 26 r mod 64 = 2 (13 r mod 32) takes 32
// distinct even values, so the 32 dword pairs tile all 64 banks.  As ds_read2_b64, which the compiler emits for two of the three
// pieces (each piece served per 16 consecutive lanes, bank = dword mod 32): 26 r mod 32 = 2 (13 r mod 16) takes 16 distinct even
// values over 16 consecutive r, so the 16 pairs tile all 32 banks.  No conflict either way.  (96 + 16 = 112 bytes, the W4A8 pad, would
// put the two buffers of a 128 x 128 tile at 67584 bytes, over the 64 KiB of static LDS; with 104 they are exactly 65536.)
constexpr int A6_WPITCH = A6_WROW + 8;

// One (64 WM rows) x (64 WN columns) tile of the W6A8 product: mxa8_gemm_tile (mxfp4_a8_common.cuh) with MXFP6 weights.  Tile rows from
// `rows` (mxfp4_common.cuh; they index xq / xs / row_flag), columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol /
// bias (0, or (long)e * N for an expert e).  4 waves as 2 x 2; per 64 k a wave reads WM x fragments (two 16-byte reads 32 bytes apart,
// a8_frag: the E4M3 operand is split in two halves with an FP6 partner as with an FP4 one, probe part (a1)) and WN weight fragments
// (three 8-byte reads) with as many scale bytes and issues WM * WN MFMAs.  The weight fragment is the A operand (FP6, cbsz 2) and the
// x fragment the B operand (E4M3, blgp 0), so a lane's accumulator holds 4 consecutive columns of one row of y.  LDS stage,
// double-buffered and filled through registers: x codes [64 WM][144], weight codes [64 WN][104], x scales [64 WM] dwords, weight scales
// [64 WN] dwords (byte j of a row's dword = the scale of the stage's block j): 32768 bytes at WM = WN = 2, so 65536 bytes of static LDS
// for the two buffers, and 32768 for the two at WM = WN = 1.  Weight rows are read from memory in 8-byte pieces (12 per row and stage):
// a row's pitch is 24 K / 32 bytes, so nothing wider is aligned.  Dead rows and whatever lies past N / K: zero codes under scale 2^0.
// All 256 threads must call it together.
template <int DT, int WM, int WN, class Rows>
__device__ __forceinline__ void mx6a8_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                                int N, int K) {
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN;
    constexpr int XLD = BM * 8 / 256, WLD = BN * 12 / 256;  // pieces per thread and stage: x row = piece / 8 (16 bytes), weight row = piece / 12 (8 bytes)
    constexpr int WOFF = BM * A8_XPITCH, SOFF = WOFF + BN * A6_WPITCH;
    constexpr int STAGE = SOFF + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    static_assert(2 * STAGE <= 65536, "static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + A6_BK - 1) / A6_BK;

    // load slots: x pieces t, t + 256, ... (8 per row: block (piece & 7) >> 1 of the stage, half piece & 1), then weight pieces (12 per
    // row: block part / 3 of the stage, 8-byte third part % 3); thread t < ROWS also loads the scales of row t of the stage image (rows
    // 0 .. BM - 1 = x, BM .. = weights)
    const uint8_t* xsrc[XLD];
    const uint8_t* wsrc[WLD];
    bool xok[XLD], wok[WLD];
    int wpart[WLD], wdst[WLD];
#pragma unroll
    for (int i = 0; i < XLD; i++) {
        const int row = (t + 256 * i) >> 3;
        xok[i] = rows.live(row);
        xsrc[i] = xq + (xok[i] ? rows.src(row) : 0L) * K + (t & 1) * 16;
    }
#pragma unroll
    for (int i = 0; i < WLD; i++) {
        const int p = t + 256 * i, row = p / 12;
        wpart[i] = p - row * 12;
        wdst[i] = WOFF + row * A6_WPITCH + wpart[i] * 8;
        wok[i] = n0 + row < N;
        wsrc[i] = qw + (r0 + min(n0 + row, N - 1)) * ((long)KB * MX6_BLOCK_BYTES) + wpart[i] * 8;
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
    uint4_t rx[XLD];
    uint2_t rw[WLD];
    uint32_t rs = 0x7f7f7f7fu;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < XLD; i++) {
            const int kb = kt * 4 + ((t & 7) >> 1);
            rx[i] = (xok[i] && kb < KB) ? *reinterpret_cast<const uint4_t*>(xsrc[i] + (long)kb * 32) : uint4_t{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < WLD; i++) {
            const int kb = kt * 4 + wpart[i] / 3;
            rw[i] = (wok[i] && kb < KB) ? *reinterpret_cast<const uint2_t*>(wsrc[i] + (long)kt * A6_WROW) : uint2_t{0u, 0u};
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
        for (int i = 0; i < WLD; i++) *reinterpret_cast<uint2_t*>(st + wdst[i]) = rw[i];
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
            for (int j = 0; j < WN; j++) {
                const uint2_t* p = reinterpret_cast<const uint2_t*>(st + WOFF + (wx * 32 * WN + j * 32 + rl) * A6_WPITCH + (ks * 2 + hh) * MX6_BLOCK_BYTES);
                fw[j] = a6_frag(p[0], p[1], p[2]);
            }
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], 2, 0, 0, (int)((swa[j] >> (16 * ks)) & 0xffu), 0,
                                                                                (int)((sxa[i] >> (16 * ks)) & 0xffu));
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: D column (= tile row) = lane & 31, D row (= column n of y) = (r & 3) + 8 (r >> 2) + 4 hh: registers 4q .. 4q + 3 are four
    // consecutive n of one row -> one 8-byte store where N allows it.  A flagged row of x and a column with e_col = 255 are NaN; the bias
    // is added after that, as in mxa8_gemm_tile.
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
