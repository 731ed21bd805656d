// Ternary-weight / int8-activation linear layer (BitNet b1.58 "BitLinear" arithmetic) for gfx950.  No reference implementation exists;
// the semantics are this library's own (include/bie_hip.h, INTEGRATION.md "Ternary W1.58A8 linear layer").
//
//   a_m = max(max_k |x[m, k]|, 1e-5),  s_m = 127 / a_m,  q[m, k] = clamp(rint(x[m, k] * s_m), -128, 127),  r_m = a_m / 127   (fp32, no FMA)
//   (a_m = NaN where row m holds a NaN or an infinity: every y of that row is NaN)
//   D[m, n] = sum_k t[n, k] * q[m, k]  (exact int32; K <= 65536)          y[m, n] = dt((float(D) * r_m) * alpha[n])
//
// The weights are ternary.hip's qweight, uint8 [2, N, K/8] (plane 0 = non-zero mask, plane 1 = +1), read as packed bits by both forms:
// no int8 image of the weights exists in HBM.
//
// Trit expansion.  Four trits (m_i, p_i) become four int8 bytes with one v_perm_b32: the selector byte i = m_i | p_i << 1 picks byte 0
// (0x00), 1 (0xFF = -1) or 3 (0x01 = +1) of the table 0x0100FF00.  The selector needs bit i of each plane in bit 0 / 1 of byte i, so the
// four trits of one expansion are k, k + 8, k + 16, k + 24 of a 32-bit word (a shift and a mask per plane, no multiply) -- and the int8
// activations are laid out to match: the decode form keeps q in LDS in that permuted order; the GEMM form reads q in natural order, so
// it spreads a nibble (four consecutive k) with v_mul_u32_u24 by 0x204081 instead.
//
// Decode form (ta8_fused_kernel, small M): one launch.  Every workgroup quantises the M rows of x into LDS (an absmax pass, then the
// write pass) and streams the bit planes of its output columns: a wave takes 4 columns at a time, lanes stride the 32-trit words, and
// per word and row eight v_dot4_i32_i8 accumulate; the K-split partials are summed on the DPP network (wave_sum_dpp, bie_common.h).
// GEMM form (prefill): ta8_quantize_kernel writes q (row pitch a multiple of 64 bytes, padding zeroed) and r, then ta8_gemm_kernel runs
// v_mfma_i32_32x32x32_i8 on the ordered pipeline of intgemm_pipe.hip's i8_pipe_gemm_kernel: q by 16-byte LDS-DMA as there, the two bit
// planes by 4-byte LDS-DMA (16 bytes per weight row and stage instead of 64), expanded to int8 fragments in registers behind the MFMAs.
#include "mfma_pipe.cuh"

namespace bie {

typedef int int16v_t __attribute__((ext_vector_type(16)));

// ---- activation quantisation (shared by both forms) ----------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void ta8_load8(const void* p, long i, float (&v)[8]) {
    if constexpr (DT == BIE_F32) {
        const float4_t a = *reinterpret_cast<const float4_t*>((const float*)p + i);
        const float4_t b = *reinterpret_cast<const float4_t*>((const float*)p + i + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4_t a = *reinterpret_cast<const uint4_t*>((const uint16_t*)p + i);
        const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if constexpr (DT == BIE_BF16) {
                v[2 * q] = __uint_as_float(w[q] << 16);
                v[2 * q + 1] = __uint_as_float(w[q] & 0xffff0000u);
            } else {
                v[2 * q] = f16_bits_to_f32(w[q] & 0xffffu);
                v[2 * q + 1] = f16_bits_to_f32(w[q] >> 16);
            }
        }
    }
}

__device__ __forceinline__ int ta8_q(float v, float s) {  // clamp(rint(v * s), -128, 127): one fp32 multiply, round half to even
    return (int)fminf(fmaxf(__builtin_rintf(v * s), -128.0f), 127.0f);
}

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// absmax of R rows of x (rows >= M contribute nothing), reduced over the 256 threads: every thread returns the same a_m.  Its static LDS (128 bytes at most) is why the decode
// form keeps 1 KiB of the 64 KiB free.  The max is taken on the bits of |x|, which order as the values do and put every NaN above +inf, so a
// row holding a NaN or an infinity gets a_m = NaN (fmaxf would drop a NaN): r_m is NaN and so is every y of that row, in both forms.
template <int DT, int R>
__device__ __forceinline__ void ta8_absmax(const void* x, int M, int K, float (&a)[R]) {
    __shared__ uint32_t red[4][R];
    uint32_t mx[R];
#pragma unroll
    for (int r = 0; r < R; r++) mx[r] = 0u;
    for (int t = threadIdx.x; t < (K >> 3); t += 256) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (r < M) {
                float v[8];
                ta8_load8<DT>(x, (long)r * K + t * 8, v);
#pragma unroll
                for (int e = 0; e < 8; e++) mx[r] = max(mx[r], __float_as_uint(v[e]) & 0x7fffffffu);
            }
        }
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t w = wave_umax(mx[r]);
        if ((threadIdx.x & 63) == 0) red[wave][r] = w;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) {
        const uint32_t m = max(max(red[0][r], red[1][r]), max(red[2][r], red[3][r]));
        a[r] = m >= 0x7f800000u ? __uint_as_float(0x7fc00000u) : fmaxf(__uint_as_float(m), 1e-5f);
    }
}

// One workgroup per row: q [M, ldq] int8 (bytes K .. ldq - 1 zeroed), r [M] fp32.
template <int DT>
__global__ __launch_bounds__(256) void ta8_quantize_kernel(const void* __restrict__ x, int8_t* __restrict__ q, float* __restrict__ rv, int K, int ldq) {
    const int m = blockIdx.x;
    const void* xr = (const char*)x + (long)m * K * dt_traits<DT>::bytes;
    float a[1];
    ta8_absmax<DT, 1>(xr, 1, K, a);
    const float s = 127.0f / a[0];
    if (threadIdx.x == 0) rv[m] = a[0] / 127.0f;
    int8_t* qr = q + (long)m * ldq;
    for (int t = threadIdx.x; t < (ldq >> 3); t += 256) {
        uint2_t o = {0u, 0u};
        if (t * 8 < K) {
            float v[8];
            ta8_load8<DT>(xr, t * 8, v);
#pragma unroll
            for (int e = 0; e < 8; e++) o[e >> 2] |= ((uint32_t)ta8_q(v[e], s) & 0xffu) << (8 * (e & 3));
        }
        *reinterpret_cast<uint2_t*>(qr + t * 8) = o;
    }
}

// y before its rounding to the dtype: two fp32 multiplies.  The empty asm keeps hipcc from folding the second multiply and the conversion
// to fp16 into one v_fma_mixlo_f16, which rounds once from the exact product (seen on this epilogue despite -ffp-contract=off).
__device__ __forceinline__ float ta8_y(int d, float r, float alpha) {
    float v = ((float)d * r) * alpha;
    asm("" : "+v"(v));
    return v;
}

// ---- trit expansion ----------------------------------------------------------------------------------------------------------------
// sm / sp: one plane bit in bit 0 of each byte (sm = mask, sp = "+1" already shifted to bit 1) -> int8 x4 of {0, -1, +1}
__device__ __forceinline__ uint32_t trit_bytes(uint32_t sm, uint32_t sp1) { return __builtin_amdgcn_perm(0u, 0x0100FF00u, sm | sp1); }

// ---- decode form ----------------------------------------------------------------------------------------------------------------------
// LDS q image: per row, per 32-trit word w, 8 dwords; byte i of dword d = q[32 w + 8 i + d] (the order trit_bytes expands the planes in).
template <int DT, int R>
__global__ __launch_bounds__(256) void ta8_fused_kernel(const void* __restrict__ x, const uint32_t* __restrict__ Wm, const uint32_t* __restrict__ Wp,
                                                        const void* __restrict__ alpha, void* __restrict__ y, int M, int N, int K, int cols_per_wg, int raw) {
    extern __shared__ uint4_t qs[];  // [R][KW][2]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KW = K >> 5;
    float a[R];
    ta8_absmax<DT, R>(x, M, K, a);
    for (int t = threadIdx.x; t < R * KW; t += 256) {
        const int r = t / KW, w = t - r * KW;
        uint32_t o[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (r < M) {
            float s = 0.0f;
#pragma unroll
            for (int rr = 0; rr < R; rr++)
                if (rr == r) s = 127.0f / a[rr];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float v[8];
                ta8_load8<DT>(x, (long)r * K + w * 32 + i * 8, v);
#pragma unroll
                for (int d = 0; d < 8; d++) o[d] |= ((uint32_t)ta8_q(v[d], s) & 0xffu) << (8 * i);
            }
        }
        qs[t * 2] = uint4_t{o[0], o[1], o[2], o[3]};
        qs[t * 2 + 1] = uint4_t{o[4], o[5], o[6], o[7]};
    }
    __syncthreads();
    const int col0 = blockIdx.x * cols_per_wg;
    const int col1 = min(N, col0 + cols_per_wg);
    for (int nb = col0 + wave * 4; nb < col1; nb += 16) {  // 4 columns at a time: their 8 loads are in flight together
        int acc[4][R];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < R; r++) acc[c][r] = 0;
        const uint32_t *wm[4], *wp[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const long o = (long)min(nb + c, N - 1) * KW;
            wm[c] = Wm + o;
            wp[c] = Wp + o;
        }
        for (int k = lane; k < KW; k += 64) {
            uint32_t m[4], p[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                m[c] = wm[c][k];
                p[c] = wp[c][k];
            }
            uint32_t qv[R][8];
#pragma unroll
            for (int r = 0; r < R; r++) {  // rows >= M hold zeros: counted, never stored
                const uint4_t lo = qs[(r * KW + k) * 2], hi = qs[(r * KW + k) * 2 + 1];
                qv[r][0] = lo.x; qv[r][1] = lo.y; qv[r][2] = lo.z; qv[r][3] = lo.w;
                qv[r][4] = hi.x; qv[r][5] = hi.y; qv[r][6] = hi.z; qv[r][7] = hi.w;
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
#pragma unroll
                for (int d = 0; d < 8; d++) {
                    const uint32_t sp1 = d ? (p[c] >> (d - 1)) & 0x02020202u : (p[c] << 1) & 0x02020202u;
                    const uint32_t w = trit_bytes((m[c] >> d) & 0x01010101u, sp1);
#pragma unroll
                    for (int r = 0; r < R; r++) acc[c][r] = __builtin_amdgcn_sdot4((int)w, (int)qv[r][d], acc[c][r], false);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int n = nb + c;
            const float aw = (alpha && !raw) ? dt_traits<DT>::load(alpha, min(n, N - 1)) : 1.0f;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (r >= M) continue;  // M is wave-uniform
                const int d = wave_sum_dpp(acc[c][r]);
                if (lane == 0 && n < col1) {
                    if (raw) ((int*)y)[(long)r * N + n] = d;
                    else dt_traits<DT>::store(y, (long)r * N + n, ta8_y(d, a[r] / 127.0f, aw));
                }
            }
        }
    }
}

// ---- GEMM form ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mfma_i8(int16v_t& c, const v4i_t& a, const v4i_t& b) {
    asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
template <int OFF>
__device__ __forceinline__ uint2_t lds_read8(uint32_t addr) {
    uint2_t r;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
template <int N>
__device__ __forceinline__ void wait_raw(uint2_t (&b)[N]) {
    static_assert(N == 2 || N == 4, "2 or 4 raw weight words");
    if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])::"memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(b[0]), "+v"(b[1])::"memory");
}
// 16 trits (bits 16 S .. 16 S + 15 of a (mask, pos) word pair) -> the 16 int8 of one MFMA operand, byte i of dword d = trit 16 S + 4 d + i
template <int S>
__device__ __forceinline__ v4i_t expand16(uint2_t mp) {
    v4i_t o;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t nm = (mp.x >> (16 * S + 4 * d)) & 0xfu, np = (mp.y >> (16 * S + 4 * d)) & 0xfu;
        const uint32_t sm = __umul24(nm, 0x204081u) & 0x01010101u;
        const uint32_t sp1 = __umul24(np, 0x408102u) & 0x02020202u;
        o[d] = (int)trit_bytes(sm, sp1);
    }
    return o;
}

// A = q [M, ldq] (k contiguous), the weight planes Wq [2, N, K/8].  Per stage (64 k) the LDS holds the tile's q rows as intgemm_pipe.hip
// does (64 bytes per row, 16-byte slots XORed by (row >> 2) & 3) and, behind them, the weight rows as 16 bytes each: mask and pos of
// k 0..31, then mask and pos of k 32..63.  A lane of half hh covers k 32 hh .. 32 hh + 31 of the stage (k step S: the 16-byte slot
// 2 hh + S of q, bits 16 S .. of its weight words), so it reads ONE 8-byte (mask, pos) pair per weight block and stage.
// y = dt((float(acc) * r[m]) * alpha[n]) or, raw, int32 acc.  K % 64 == 32: the weight half past K is expanded as zeros.
template <int DT, bool RAW, int WM, int WN>
__global__ __launch_bounds__(256) void ta8_gemm_kernel(const uint8_t* __restrict__ A, const float* __restrict__ rv, const uint8_t* __restrict__ Wq,
                                                       const void* __restrict__ alpha, void* __restrict__ yv, int M, int N, int K, int ldq, int tiles_n) {
    constexpr int AF = 2 * WM, BF = 2 * WN;
    constexpr int A_BYTES = AF * 2048, B_BYTES = BF * 512;  // 64 bytes x 32 AF rows; 16 bytes x 32 BF rows
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int PA = AF * 2 / 4, PB = BF * 2 / 4;  // pieces per wave: A 1 KiB (16 rows), B 256 bytes (16 rows)
    constexpr int PW = PA + PB;
    constexpr int NR = WM, NM = WM * WN;
    constexpr int RPM = (2 * NR + NM - 1) / NM, M0 = (NR + RPM - 1) / RPM, DPM = (PW + (NM - M0) - 1) / (NM - M0);
    constexpr int EPM = (WN + NM - 2) / (NM - 1);  // expansions per MFMA, behind MFMAs 1 ..
    __shared__ __attribute__((aligned(1024))) unsigned char lds[3 * STAGE];
    __shared__ __attribute__((aligned(16))) float ep[AF * 32 + BF * 32];  // the epilogue's r of the tile rows, alpha of the tile columns

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wy = wave >> 1, wx = wave & 1;
    int tile_m, tile_n;
    pipe_tile(blockIdx.x, gridDim.x, tiles_n, BIE_PIPE_GM, tile_m, tile_n);
    const int KT = (K + 63) >> 6, KB = K >> 3;
    const bool tail = (K & 63) != 0;

    // LDS-DMA sources.  A: as i8_pipe_gemm_kernel.  B: lane l of piece j moves dword (l & 3) of weight row 16 j + (l >> 2): 0 / 2 mask,
    // 1 / 3 pos, of k 0..31 / 32..63; a word past the row's end (K % 64 == 32) re-reads the last in-bounds one (expanded as zeros).
    const uint8_t* asrc[PA];
#pragma unroll
    for (int j = 0; j < PA; j++) {
        const int rt = (wave * PA + j) * 16 + (lane >> 2);
        const long r = min(tile_m * (AF * 32) + rt, M - 1);
        asrc[j] = A + r * ldq + (((lane & 3) ^ ((rt >> 2) & 3)) << 4);
    }
    const uint8_t* bsrc[PB];
#pragma unroll
    for (int j = 0; j < PB; j++) {
        const int rt = (wave * PB + j) * 16 + (lane >> 2);
        const long r = min(tile_n * (BF * 32) + rt, N - 1);
        bsrc[j] = Wq + ((lane & 1) ? (long)N * KB : 0L) + r * KB;
    }
    const int bhalf = (lane & 2) * 2;  // 0 or 4 bytes
    [[maybe_unused]] const int kt_last = KT - 1;
    auto issue_piece = [&](int kt, int j) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int ks = kt < kt_last ? kt : kt_last;
        auto* dst = (__attribute__((address_space(3))) unsigned char*)lds + (kt % 3) * STAGE;
        if (j < PA) {
            __builtin_amdgcn_global_load_lds(asrc[j] + (long)ks * 64, dst + wave * (PA * 1024) + j * 1024, 16, 0, 0);
        } else {
            const int jb = j - PA, o = min(8 * ks + bhalf, KB - 4);
            __builtin_amdgcn_global_load_lds(bsrc[jb] + o, dst + A_BYTES + wave * (PB * 256) + jb * 256, 4, 0, 0);
        }
#endif
    };

    const uint32_t lds_base = (uint32_t)(uintptr_t)lds;
    const int rl = lane & 31, hh = lane >> 5, sw = (rl >> 2) & 3;
    uint32_t a_addr[2];  // k step s: slot 2 hh + s of row rl of the wave's first block
#pragma unroll
    for (int s = 0; s < 2; s++) a_addr[s] = lds_base + (uint32_t)((wy * WM * 32 + rl) * 64 + (((2 * hh + s) ^ sw) << 4));
    const uint32_t b_addr = lds_base + A_BYTES + (uint32_t)((wx * WN * 32 + rl) * 16 + 8 * hh);

    int16v_t acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0;

    v4i_t XA[WM], YA[WM], ZA[WM];
    v4i_t E0[WN], E1[WN];  // the stage's weight operands of k step 0 / 1
    uint2_t RB[WN];        // raw (mask, pos) words of the weight blocks
    auto read_a = [&](auto ic, auto hc, uint32_t so, v4i_t (&TA)[WM]) {
        constexpr int R = decltype(ic)::value, H = decltype(hc)::value;
        TA[R] = lds_read16<R * 2048>(a_addr[H] + so);
    };
    auto read_b = [&](uint32_t so) {
        static_for<0, WN>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            RB[J] = lds_read8<J * 512>(b_addr + so);
        });
    };
    // the raw words of stage kt have landed: clear the half past K
    auto cut_b = [&](int kt) {
        if (tail && kt == kt_last && hh) {
#pragma unroll
            for (int j = 0; j < WN; j++) RB[j] = uint2_t{0u, 0u};
        }
    };
    // The expansions are VALU results an asm MFMA reads: the empty asm pins each to its slot, the s_nop 1 ahead of the first consuming
    // MFMA covers the VALU-write -> MFMA-read wait states the compiler does not insert for an asm statement.
    auto expand = [&](auto jc, auto sc) {
        constexpr int J = decltype(jc)::value, S = decltype(sc)::value;
        if constexpr (S == 0) {
            E0[J] = expand16<0>(RB[J]);
            asm volatile("" : "+v"(E0[J]));
        } else {
            E1[J] = expand16<1>(RB[J]);
            asm volatile("" : "+v"(E1[J]));
        }
    };

#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
        for (int j = 0; j < PW; j++) issue_piece(s, j);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PW) : "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, NR>([&](auto rc) { read_a(rc, ic_t<0>{}, 0u, XA); });
    read_b(0u);
    wait_raw(RB);
    cut_b(0);
    static_for<0, WN>([&](auto jc) { expand(jc, ic_t<0>{}); });

    // entering stage kt: P (k step 0 of q) read, RB (the stage's weight words) landed, E0 expanded
    auto stage = [&](int kt, v4i_t (&PA_)[WM], v4i_t (&QA)[WM], v4i_t (&NA)[WM]) {
        const uint32_t so = (uint32_t)(kt % 3) * STAGE, sn = (uint32_t)((kt + 1) % 3) * STAGE;
        wait_frags<0>(PA_, E0);
        asm volatile("s_nop 1" ::: "memory");
        // cluster 1: k step 0; reads of k step 1 behind the first MFMAs, E1 = k step 1 weights behind the rest
        static_for<0, NM>([&](auto mc) {
            constexpr int m = decltype(mc)::value, i = m / WN, j = m % WN;
            mfma_i8(acc[i][j], E0[j], PA_[i]);
            static_for<imin(m * RPM, NR), imin((m + 1) * RPM, NR)>([&](auto rc) { read_a(rc, ic_t<1>{}, so, QA); });
            if constexpr (m >= 1) static_for<imin((m - 1) * EPM, WN), imin(m * EPM, WN)>([&](auto jc) { expand(jc, ic_t<1>{}); });
        });
        wait_frags<0>(QA, E1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("s_nop 1" ::: "memory");
        read_b(sn);  // the next stage's weight words
        // cluster 2: k step 1; the next stage's q reads and E0 expansions, refill pieces behind the rest
        static_for<0, NM>([&](auto mc) {
            constexpr int m = decltype(mc)::value, i = m / WN, j = m % WN;
            mfma_i8(acc[i][j], E1[j], QA[i]);
            if constexpr (m == 0) {
                wait_raw(RB);
                cut_b(kt + 1);
            }
            static_for<imin(m * RPM, NR), imin((m + 1) * RPM, NR)>([&](auto rc) { read_a(rc, ic_t<0>{}, sn, NA); });
            if constexpr (m >= 1) static_for<imin((m - 1) * EPM, WN), imin(m * EPM, WN)>([&](auto jc) { expand(jc, ic_t<0>{}); });
            if constexpr (m >= M0)
                static_for<imin((m - M0) * DPM, PW), imin((m - M0 + 1) * DPM, PW)>([&](auto pc) { issue_piece(kt + 3, decltype(pc)::value); });
        });
    };
    int kt = 0;
    for (; kt + 3 <= KT; kt += 3) {
        stage(kt, XA, YA, ZA);
        stage(kt + 1, ZA, XA, YA);
        stage(kt + 2, YA, ZA, XA);
    }
    if (kt < KT) {
        stage(kt, XA, YA, ZA);
        if (kt + 1 < KT) stage(kt + 1, ZA, XA, YA);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    mfma_drain();

    // epilogue: the tile's r (rows) and alpha (columns) staged once in LDS
    if constexpr (!RAW) {
        for (int t = threadIdx.x; t < AF * 32 + BF * 32; t += 256) {
            if (t < AF * 32) ep[t] = rv[min(tile_m * AF * 32 + t, M - 1)];
            else ep[t] = alpha ? dt_traits<DT>::load(alpha, min(tile_n * BF * 32 + t - AF * 32, N - 1)) : 1.0f;
        }
        __syncthreads();
    }
    // C/D: column = lane & 31 = row m of q, row = (r & 3) + 8 (r >> 2) + 4 hh = column n inside the 32-block: four consecutive n per
    // register group
    const int n_l = 4 * hh;
    const bool vec = (N & 3) == 0;
#pragma unroll
    for (int i = 0; i < WM; i++) {
        const int ml = (wy * WM + i) * 32 + rl, m = tile_m * AF * 32 + ml;
        if (m < M) {
            const float rm = RAW ? 1.0f : ep[ml];
#pragma unroll
            for (int j = 0; j < WN; j++) {
                const int nl0 = (wx * WN + j) * 32 + n_l;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int nl = nl0 + 8 * q, n = tile_n * BF * 32 + nl;
                    if (n >= N) continue;
                    if constexpr (RAW) {
                        int* yr = (int*)yv + (long)m * N + n;
                        if (vec) *reinterpret_cast<v4i_t*>(yr) = v4i_t{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                        else
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                if (n + e < N) yr[e] = acc[i][j][4 * q + e];
                    } else {
                        float o[4];
#pragma unroll
                        for (int e = 0; e < 4; e++) o[e] = ta8_y(acc[i][j][4 * q + e], rm, ep[AF * 32 + nl + e]);
                        const long yi = (long)m * N + n;
                        if (vec) {
                            if constexpr (DT == BIE_F32) *reinterpret_cast<float4_t*>((float*)yv + yi) = float4_t{o[0], o[1], o[2], o[3]};
                            else if constexpr (DT == BIE_F16)
                                *reinterpret_cast<uint2_t*>((uint16_t*)yv + yi) = uint2_t{f32_to_f16_bits(o[0]) | (f32_to_f16_bits(o[1]) << 16), f32_to_f16_bits(o[2]) | (f32_to_f16_bits(o[3]) << 16)};
                            else *reinterpret_cast<uint2_t*>((uint16_t*)yv + yi) = uint2_t{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                if (n + e < N) dt_traits<DT>::store(yv, yi + e, o[e]);
                        }
                    }
                }
            }
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
int ta8_quantize_launch(const void* x, int8_t* q, float* r, long M, long K, long ldq, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)M);
    if (dtype == BIE_F16) hipLaunchKernelGGL(ta8_quantize_kernel<BIE_F16>, grid, dim3(256), 0, st, x, q, r, (int)K, (int)ldq);
    else if (dtype == BIE_BF16) hipLaunchKernelGGL(ta8_quantize_kernel<BIE_BF16>, grid, dim3(256), 0, st, x, q, r, (int)K, (int)ldq);
    else hipLaunchKernelGGL(ta8_quantize_kernel<BIE_F32>, grid, dim3(256), 0, st, x, q, r, (int)K, (int)ldq);
    return check_launch("ta8_quantize_kernel");
}

// The decode form serves 1 <= M <= TA8_FUSED_ROWS; the instance is the smallest R in {1, 2, 4, 8} >= M, whose R * K bytes of q sit in one
// workgroup's LDS.  The bound was measured against the GEMM form (tools/ternary_a8_bench.py, profiles/ternary_a8_bench.jsonl): the decode
// form was ahead at every M <= 8 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 in fp16 and bf16 (at M = 8, 4096 -> 11008: 23.5 against
// 36.9 us per call).  A 16-row instance would need 16 K bytes of LDS, 64 KiB at K = 4096.
constexpr int TA8_FUSED_ROWS = 8;
static int ta8_rows(long M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8; }

bool ternary_a8_fused_ok(long M, long N, long K) {
    return M >= 1 && M <= TA8_FUSED_ROWS && N >= 1 && N < (1L << 31) && K >= 32 && K % 32 == 0 && K <= 65536 && (long)ta8_rows(M) * K <= 65536 - 1024;
}

template <int DT, int R>
static void ta8_fused_launch_r(const void* x, const uint8_t* q, const void* alpha, void* y, int M, int N, int K, int raw, hipStream_t st) {
    const size_t lds = (size_t)R * K;
    // up to 1024 column blocks of at least the 16 columns one sweep of the 4 waves covers (the grid of ternary.hip's decode form)
    const int cols = (int)cdivl(cdivl(N, 1024), 16) * 16;
    const dim3 grid((unsigned)cdivl(N, cols));
    const uint32_t* wm = reinterpret_cast<const uint32_t*>(q);
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(q + (size_t)N * (K / 8));
    hipLaunchKernelGGL((ta8_fused_kernel<DT, R>), grid, dim3(256), lds, st, x, wm, wp, alpha, y, M, N, K, cols, raw);
}

template <int DT>
static void ta8_fused_launch_dt(const void* x, const uint8_t* q, const void* alpha, void* y, int M, int N, int K, int raw, hipStream_t st) {
    switch (ta8_rows(M)) {
    case 1: ta8_fused_launch_r<DT, 1>(x, q, alpha, y, M, N, K, raw, st); break;
    case 2: ta8_fused_launch_r<DT, 2>(x, q, alpha, y, M, N, K, raw, st); break;
    case 4: ta8_fused_launch_r<DT, 4>(x, q, alpha, y, M, N, K, raw, st); break;
    default: ta8_fused_launch_r<DT, 8>(x, q, alpha, y, M, N, K, raw, st); break;
    }
}

int ternary_a8_fused_launch(const void* x, const uint8_t* q, const void* alpha, void* y, long M, long N, long K, int dtype, int raw, hipStream_t st) {
    if (dtype == BIE_F16) ta8_fused_launch_dt<BIE_F16>(x, q, alpha, y, (int)M, (int)N, (int)K, raw, st);
    else if (dtype == BIE_BF16) ta8_fused_launch_dt<BIE_BF16>(x, q, alpha, y, (int)M, (int)N, (int)K, raw, st);
    else ta8_fused_launch_dt<BIE_F32>(x, q, alpha, y, (int)M, (int)N, (int)K, raw, st);
    return check_launch("ta8_fused_kernel");
}

// Tiles as i8_pipe_launch: 256 x 256 where that grid has >= 192 tiles, else 128 x 128.  The raw (int32 D) output takes the 128 x 128
// tile only: its 256 x 256 instance does not fit the register file.
int ternary_a8_gemm_launch(const int8_t* q, const float* r, long ldq, const uint8_t* qw, const void* alpha, void* y, long M, long N, long K, int dtype,
                           int raw, hipStream_t st) {
    const long t256 = cdivl(M, 256) * cdivl(N, 256);
    const bool big = t256 >= 192 && !raw;
    const int tn = (int)cdivl(N, big ? 256 : 128);
    const dim3 grid((unsigned)(big ? t256 : cdivl(M, 128) * tn));
    const uint8_t* A = reinterpret_cast<const uint8_t*>(q);
#define BIE_TA8(DTV, RAWV) \
    do { \
        if (big) hipLaunchKernelGGL((ta8_gemm_kernel<DTV, RAWV, 4, 4>), grid, dim3(256), 0, st, A, r, qw, alpha, y, (int)M, (int)N, (int)K, (int)ldq, tn); \
        else hipLaunchKernelGGL((ta8_gemm_kernel<DTV, RAWV, 2, 2>), grid, dim3(256), 0, st, A, r, qw, alpha, y, (int)M, (int)N, (int)K, (int)ldq, tn); \
    } while (0)
    if (raw) hipLaunchKernelGGL((ta8_gemm_kernel<BIE_F32, true, 2, 2>), grid, dim3(256), 0, st, A, r, qw, alpha, y, (int)M, (int)N, (int)K, (int)ldq, tn);
    else if (dtype == BIE_F16) BIE_TA8(BIE_F16, false);
    else if (dtype == BIE_BF16) BIE_TA8(BIE_BF16, false);
    else BIE_TA8(BIE_F32, false);
#undef BIE_TA8
    return check_launch("ta8_gemm_kernel");
}

}  // namespace bie
