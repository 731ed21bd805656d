// The device-side pieces shared by the W4A4 translation units (mxfp4_a4.hip, mxfp4_moe_a4.hip; gfx950): the operand types of the
// block-scaled matrix instructions, the activation quantiser's rule for one 8-value unit, so that a kernel that quantises a row
// itself produces the bits of mxa4_quantize_kernel, and the prefill tile body on v_mfma_scale_f32_32x32x64_f8f6f4 (mxa4_gemm_tile:
// mxa4_gemm_kernel of mxfp4_a4.hip and mxma4_gemm_kernel of mxfp4_moe_a4.hip).
#pragma once
#include "mxfp4_common.cuh"

namespace bie {

typedef int mxa4_v8i __attribute__((ext_vector_type(8)));
typedef float mxa4_v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float a4_nan() { return __uint_as_float(0x7fc00000u); }

__device__ __forceinline__ mxa4_v8i a4_frag(const uint4_t& v) { return mxa4_v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0}; }

template <int CTRL>
__device__ __forceinline__ float a4_dpp_max(float v) {
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)));
}

// One 8-value unit (16 bytes of x) of a block of 32 whose four units sit on the four lanes of a quad: the block maximum over the quad on
// the DPP network, the block's E8M0 code and this lane's dword of codes.  `bad` collects a NaN or +-inf.  All lanes of the quad must
// call it together.
template <int DT>
__device__ __forceinline__ void a4_quantize_unit(const uint4_t& raw, int& bad, uint32_t& codes, uint32_t& scode) {
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
    codes = 0u;
    scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mx_block_scale(amax, inv);
#pragma unroll
        for (int i = 0; i < 8; i++) codes |= (mx_round_e2m1(fabsf(v[i] * inv)) | ((__float_as_uint(v[i]) >> 28) & 8u)) << (4 * i);
    }
}

// ---- the W4A4 prefill tile ------------------------------------------------------------------------------------------------------------------
constexpr int A4_BK = 128;                // k per stage: 64 code bytes and 4 scale bytes per row
constexpr int A4_PITCH = A4_BK / 2 + 16;  // 80 bytes per row in LDS: the 16-byte fragment reads of 16 rows fall on distinct banks

// One (64 WM rows) x (64 WN columns) tile of the W4A4 product: tile rows from `rows` (mxfp4_common.cuh; they index xq / xs / row_flag),
// columns n0 .. of the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for expert e).  4 waves as 2 x 2;
// per 64 k a wave reads WM + WN fragments and as many scale bytes and issues WM * WN MFMAs.  The weight fragment is the A operand, so a
// lane's accumulator holds 4 consecutive columns of one row of y.  LDS stage, double-buffered and filled through registers: x codes
// [64 WM][80], weight codes [64 WN][80], x scales [64 WM] dwords, weight scales [64 WN] dwords (byte j of a row's dword = the scale of
// the stage's block j).  Dead rows and whatever lies past N / K: zero codes under scale 2^0.  All 256 threads must call it together.
template <int DT, int WM, int WN, class Rows>
__device__ __forceinline__ void mxa4_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                               const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                               const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                               int N, int K) {
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN;
    constexpr int NLD = ROWS * 4 / 256;  // 16-byte pieces per thread and stage: row = piece / 4, quarter = piece % 4
    constexpr int STAGE = ROWS * A4_PITCH + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + A4_BK - 1) / A4_BK;

    // load slots: pieces t, t + 256, ... of the stage image (rows 0 .. BM - 1 = x, BM .. = weights); thread t < ROWS also loads row t's scales
    const uint8_t* csrc[NLD];
    bool cok[NLD];
#pragma unroll
    for (int i = 0; i < NLD; i++) {
        const int row = (t + 256 * i) >> 2;
        if (row < BM) {
            cok[i] = rows.live(row);
            csrc[i] = xq + (cok[i] ? rows.src(row) : 0L) * (K >> 1);
        } else {
            cok[i] = n0 + row - BM < N;
            csrc[i] = qw + (r0 + min(n0 + row - BM, N - 1)) * (K >> 1);
        }
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
    uint4_t rc[NLD];
    uint32_t rs = 0x7f7f7f7fu;
    auto load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NLD; i++) {
            const int kb = kt * 4 + ((t + 256 * i) & 3);
            rc[i] = (cok[i] && kb < KB) ? *reinterpret_cast<const uint4_t*>(csrc[i] + (long)kb * 16) : uint4_t{0u, 0u, 0u, 0u};
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
        for (int i = 0; i < NLD; i++) {
            const int p = t + 256 * i;
            *reinterpret_cast<uint4_t*>(st + (p >> 2) * A4_PITCH + (p & 3) * 16) = rc[i];
        }
        if (s_thread) reinterpret_cast<uint32_t*>(st + ROWS * A4_PITCH)[t] = rs;
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
        const uint32_t* ss = reinterpret_cast<const uint32_t*>(st + ROWS * A4_PITCH);
        uint32_t sxa[WM], swa[WN];  // the row's four scale bytes, shifted so that this lane's block of k-step ks sits in byte 2 ks
#pragma unroll
        for (int i = 0; i < WM; i++) sxa[i] = ss[wy * 32 * WM + i * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int j = 0; j < WN; j++) swa[j] = ss[BM + wx * 32 * WN + j * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            mxa4_v8i fx[WM], fw[WN];
#pragma unroll
            for (int i = 0; i < WM; i++)
                fx[i] = a4_frag(*reinterpret_cast<const uint4_t*>(st + (wy * 32 * WM + i * 32 + rl) * A4_PITCH + (ks * 2 + hh) * 16));
#pragma unroll
            for (int j = 0; j < WN; j++)
                fw[j] = a4_frag(*reinterpret_cast<const uint4_t*>(st + (BM + wx * 32 * WN + j * 32 + rl) * A4_PITCH + (ks * 2 + hh) * 16));
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], 4, 4, 0, (int)((swa[j] >> (16 * ks)) & 0xffu), 0,
                                                                                (int)((sxa[i] >> (16 * ks)) & 0xffu));
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: D column (= tile row) = lane & 31, D row (= column n of y) = (r & 3) + 8 (r >> 2) + 4 hh: registers 4q .. 4q + 3 are four
    // consecutive n of one row -> one 8-byte store where N allows it.  A flagged row of x and a column with e_col = 255 are NaN.
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
