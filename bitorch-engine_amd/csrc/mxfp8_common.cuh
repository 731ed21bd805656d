// The device-side pieces of the W8A8 translation unit (mxfp8_a8.hip; gfx950): the prefill tile body on
// v_mfma_scale_f32_32x32x64_f8f6f4 with an E4M3 A operand (the weights) and an E4M3 B operand (the activations of mxa8_quantize_kernel).
// mx8a8_gemm_tile takes the row sources of mxfp4_common.cuh and a weight row offset r0 exactly as mxa8_gemm_tile does, so that a grouped
// expert GEMM can adopt it unchanged.  The operand map is the one tools/probe/probe_mx_fp8x8.hip printed (profiles/mxfp8_a8_probe.txt):
// byte j of lane group g of A meets byte j of lane group g of B, and on either operand bytes 0 .. 15 of lane group g lie in block g / 2
// of the instruction's K and bytes 16 .. 31 in block G / 2 + g / 2 (G = 2 lane groups here) -- a8_frag's two halves on both sides.
#pragma once
#include "mxfp4_a8_common.cuh"

namespace bie {

// ---- the W8A8 prefill tile ------------------------------------------------------------------------------------------------------------------
// k per stage.  With one byte per weight the x image and the weight image of a stage are the same size, and a 128 x 128 tile at 128 k per
// stage would need 2 x 37888 = 75776 bytes for its two buffers, over the 65536 bytes of static LDS.  So the stage size is a parameter:
// 128 x 128 tiles run at 64 k per stage (BK = 64: 2 x 21504 = 43008 bytes) and 64 x 64 tiles at 128 k per stage (BK = 128:
// 2 x 18944 = 37888 bytes); 128 x 64 at 128 k per stage (2 x 28416 = 56832 bytes) fits as well and was measured (the launcher of
// mxfp8_a8.hip says what the measurement kept).  The pitch is BK + 16 bytes for both images: 36 dwords at BK = 128 (A8_XPITCH) and 20
// dwords at BK = 64 (A8_WPITCH's), at which the 16-byte fragment reads of 16 consecutive rows fall on distinct banks.
template <int BK>
struct mx8_stage {
    static_assert(BK == 64 || BK == 128, "a stage is one or two 64-k steps");
    static constexpr int PITCH = BK + 16;
    static constexpr int PIECES = BK / 16;  // 16-byte pieces per row and stage
};

// One (64 WM rows) x (64 WN columns) tile of the W8A8 product: tile rows from `rows` (mxfp4_common.cuh; they index xq / xs / row_flag),
// columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for an expert e).  4 waves as 2 x 2;
// per 64 k a wave reads WM x fragments and WN weight fragments (each two 16-byte reads 32 bytes apart, see a8_frag) with as many scale
// bytes and issues WM * WN MFMAs.  The weight fragment is the A operand and the x fragment the B operand (cbsz 0, blgp 0), so a lane's
// accumulator holds 4 consecutive columns of one row of y.  LDS stage, double-buffered and filled through registers: x codes
// [64 WM][BK + 16], weight codes [64 WN][BK + 16], both row-major as in memory, x scales [64 WM] dwords, weight scales [64 WN] dwords
// (byte j of a row's dword = the scale of the stage's block j).  Dead rows and whatever lies past N / K: zero codes under scale 2^0.
// All 256 threads must call it together.
template <int DT, int WM, int WN, class Rows, int BK = 128>
__device__ __forceinline__ void mx8a8_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                                int N, int K) {
    constexpr int PITCH = mx8_stage<BK>::PITCH, PIECES = mx8_stage<BK>::PIECES, SB = BK / 32;
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN;
    constexpr int XLD = BM * PIECES / 256, WLD = BN * PIECES / 256;  // 16-byte pieces per thread and stage: row = piece / PIECES
    constexpr int WOFF = BM * PITCH, SOFF = WOFF + BN * PITCH;
    constexpr int STAGE = SOFF + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    static_assert(2 * STAGE <= 65536, "two stages must fit the static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + BK - 1) / BK;

    // load slots: x pieces t, t + 256, ... (PIECES per row: bytes 16 (piece % PIECES) .. + 15 of the row's stage), then weight pieces
    // likewise; thread t < ROWS also loads the scales of row t of the stage image (rows 0 .. BM - 1 = x, BM .. = weights)
    const uint8_t* xsrc[XLD];
    const uint8_t* wsrc[WLD];
    bool xok[XLD], wok[WLD];
    const int pc = (t % PIECES) * 16;  // 256 is a multiple of PIECES: the same for every slot of a thread
#pragma unroll
    for (int i = 0; i < XLD; i++) {
        const int row = (t + 256 * i) / PIECES;
        xok[i] = rows.live(row);
        xsrc[i] = xq + (xok[i] ? rows.src(row) : 0L) * K + pc;
    }
#pragma unroll
    for (int i = 0; i < WLD; i++) {
        const int row = (t + 256 * i) / PIECES;
        wok[i] = n0 + row < N;
        wsrc[i] = qw + (r0 + min(n0 + row, N - 1)) * K + pc;
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
        const bool kin = kt * BK + pc < K;  // K is a multiple of 32: a 16-byte piece is whole inside the row or whole outside
#pragma unroll
        for (int i = 0; i < XLD; i++)
            rx[i] = (xok[i] && kin) ? *reinterpret_cast<const uint4_t*>(xsrc[i] + (long)kt * BK) : uint4_t{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < WLD; i++)
            rw[i] = (wok[i] && kin) ? *reinterpret_cast<const uint4_t*>(wsrc[i] + (long)kt * BK) : uint4_t{0u, 0u, 0u, 0u};
        if (s_thread) {
            rs = 0x7f7f7f7fu;
#pragma unroll
            for (int j = 0; j < SB; j++) {
                const int kb = kt * SB + j;
                const uint32_t s = (sok && kb < KB) ? (uint32_t)ssrc[kb] : 127u;
                rs = (rs & ~(0xffu << (8 * j))) | (s << (8 * j));
            }
        }
    };
    auto store = [&](int buf) {
        unsigned char* st = lds + buf * STAGE;
#pragma unroll
        for (int i = 0; i < XLD; i++) *reinterpret_cast<uint4_t*>(st + ((t + 256 * i) / PIECES) * PITCH + pc) = rx[i];
#pragma unroll
        for (int i = 0; i < WLD; i++) *reinterpret_cast<uint4_t*>(st + WOFF + ((t + 256 * i) / PIECES) * PITCH + pc) = rw[i];
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
        uint32_t sxa[WM], swa[WN];  // the row's scale bytes, shifted so that this lane's block of k-step ks sits in byte 2 ks
#pragma unroll
        for (int i = 0; i < WM; i++) sxa[i] = ss[wy * 32 * WM + i * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int j = 0; j < WN; j++) swa[j] = ss[BM + wx * 32 * WN + j * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int ks = 0; ks < BK / 64; ks++) {
            mxa4_v8i fx[WM], fw[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) {
                const uint4_t* p = reinterpret_cast<const uint4_t*>(st + (wy * 32 * WM + i * 32 + rl) * PITCH + ks * 64 + hh * 16);
                fx[i] = a8_frag(p[0], p[2]);  // bytes 16 hh .. + 15 of the step's first block and of its second (a8_frag)
            }
#pragma unroll
            for (int j = 0; j < WN; j++) {
                const uint4_t* p = reinterpret_cast<const uint4_t*>(st + WOFF + (wx * 32 * WN + j * 32 + rl) * PITCH + ks * 64 + hh * 16);
                fw[j] = a8_frag(p[0], p[2]);  // the same two halves: byte j of a lane group of A meets byte j of that lane group of B
            }
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], 0, 0, 0, (int)((swa[j] >> (16 * ks)) & 0xffu), 0,
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
