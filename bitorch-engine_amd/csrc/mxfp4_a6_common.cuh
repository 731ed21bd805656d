// The device-side piece of the W4A6 translation unit (mxfp4_a6.hip; gfx950): the prefill tile body on v_mfma_scale_f32_32x32x64_f8f6f4
// with an FP4 A operand (the MXFP4 weights, cbsz 4) and an FP6 E2M3 B operand (the MXFP6 activations of mx6a6_quantize_kernel, blgp 2).
// Its weight half is mxa4_gemm_tile's (mxfp4_a4_common.cuh: 64 code bytes per row and stage at A4_PITCH, 16-byte pieces, a4_frag) and its
// x half mx6a6_gemm_tile's (mxfp6_common.cuh: 96 code bytes per row and stage at A6_WPITCH, 8-byte pieces, a6_frag); it takes the row
// sources of mxfp4_common.cuh and a weight row offset like either, so that a grouped expert GEMM can call it as it stands.
#pragma once
#include "mxfp6_common.cuh"

namespace bie {

// One (64 WM rows) x (64 WN columns) tile of the W4A6 product.  xq6 [rows, 3K/4] / xs / row_flag are indexed by `rows`; columns n0 .. of
// the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for an expert e).  How the instruction reads this
// mixed pair was pinned by tools/probe/probe_mx_fp4x6.hip (profiles/mxfp4_a6_probe.txt): lane group hh = lane >> 5 holds k = 32 hh ..
// 32 hh + 31 of the instruction's 64 on EITHER operand, the FP4 one as 16 bytes (code j in bits 4 j .. 4 j + 3: qweight's bytes) and the
// FP6 one as 24 bytes (code j in bits 6 j .. 6 j + 5: xq6's bytes), and the scale byte of group hh applies to block hh.  So both
// fragments are plain copies: the x fragment three 8-byte reads (block 2 ks + hh of the stage), the weight fragment one 16-byte read.
// 4 waves as 2 x 2; per 64 k a wave reads WM x fragments and WN weight fragments with as many scale bytes and issues WM * WN MFMAs.  The
// weight fragment is the A operand, so a lane's accumulator holds 4 consecutive columns of one row of y.  LDS stage, double-buffered
// and filled through registers: x codes [64 WM][104] (A6_WPITCH and its bank argument: the same bytes read by the same lanes in the
// same way), weight codes [64 WN][80] (A4_PITCH: the 16-byte fragment reads of 16 rows fall on distinct banks), x scales [64 WM]
// dwords, weight scales [64 WN] dwords (byte j of a row's dword = the scale of the stage's block j): 13312 + 10240 + 1024 = 24576 bytes
// at WM = WN = 2, 49152 for the two buffers.  x rows are read from memory in 8-byte pieces (12 per row and stage: a row's pitch is
// 24 K / 32 bytes, nothing wider is aligned), weight rows in 16-byte pieces (4 per row and stage).  Dead rows and whatever lies past
// N / K: zero codes under scale 2^0.  All 256 threads must call it together.
template <int DT, int WM, int WN, class Rows>
__device__ __forceinline__ void mx4a6_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                                int N, int K) {
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN;
    constexpr int XLD = BM * 12 / 256, WLD = BN * 4 / 256;  // pieces per thread and stage: x row = piece / 12 (8 bytes), weight row = piece / 4 (16 bytes)
    constexpr int WOFF = BM * A6_WPITCH, SOFF = WOFF + BN * A4_PITCH;
    constexpr int STAGE = SOFF + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    static_assert(WOFF % 16 == 0 && SOFF % 16 == 0, "16-byte weight pieces, dword scales");
    static_assert(2 * STAGE < 65536, "static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + A6_BK - 1) / A6_BK;
    const long xrowb = (long)KB * MX6_BLOCK_BYTES;

    // load slots: x pieces t, t + 256, ... (12 per row: block part / 3 of the stage, 8-byte third part % 3), then weight pieces (4 per
    // row: block piece & 3); thread t < ROWS also loads the scales of row t of the stage image (rows 0 .. BM - 1 = x, BM .. = weights)
    const uint8_t* xsrc[XLD];
    const uint8_t* wsrc[WLD];
    bool xok[XLD], wok[WLD];
    int xpart[XLD], xdst[XLD];
#pragma unroll
    for (int i = 0; i < XLD; i++) {
        const int p = t + 256 * i, row = p / 12;
        xpart[i] = p - row * 12;
        xdst[i] = row * A6_WPITCH + xpart[i] * 8;
        xok[i] = rows.live(row);
        xsrc[i] = xq + (xok[i] ? rows.src(row) : 0L) * xrowb + xpart[i] * 8;
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
    uint2_t rx[XLD];
    uint4_t rw[WLD];
    uint32_t rs = 0x7f7f7f7fu;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < XLD; i++) {
            const int kb = kt * 4 + xpart[i] / 3;
            rx[i] = (xok[i] && kb < KB) ? *reinterpret_cast<const uint2_t*>(xsrc[i] + (long)kt * A6_WROW) : uint2_t{0u, 0u};
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
        for (int i = 0; i < XLD; i++) *reinterpret_cast<uint2_t*>(st + xdst[i]) = rx[i];
#pragma unroll
        for (int i = 0; i < WLD; i++) {
            const int p = t + 256 * i;
            *reinterpret_cast<uint4_t*>(st + WOFF + (p >> 2) * A4_PITCH + (p & 3) * 16) = rw[i];
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
                const uint2_t* p = reinterpret_cast<const uint2_t*>(st + (wy * 32 * WM + i * 32 + rl) * A6_WPITCH + (ks * 2 + hh) * MX6_BLOCK_BYTES);
                fx[i] = a6_frag(p[0], p[1], p[2]);
            }
#pragma unroll
            for (int j = 0; j < WN; j++)
                fw[j] = a4_frag(*reinterpret_cast<const uint4_t*>(st + WOFF + (wx * 32 * WN + j * 32 + rl) * A4_PITCH + (ks * 2 + hh) * 16));
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], 4, 2, 0, (int)((swa[j] >> (16 * ks)) & 0xffu), 0,
                                                                                (int)((sxa[i] >> (16 * ks)) & 0xffu));
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D as in mxa8_gemm_tile: D column (= tile row) = lane & 31, D row (= column n of y) = (r & 3) + 8 (r >> 2) + 4 hh: registers
    // 4q .. 4q + 3 are four consecutive n of one row -> one 8-byte store where N allows it.  A flagged row of x and a column with
    // e_col = 255 are NaN; the bias is added after that.
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
