// The decode side of the translation units on the block-scaled matrix instructions (gfx950), on v_mfma_scale_f32_16x16x128_f8f6f4: the
// dense body (mx_scaled_decode_rows: mx4a6_, mxa8_ and mx6a6_decode_kernel) and the routed body of the expert layers
// (mx_scaled_decode_pair: mx4m6_, mxma8_, mx6m6_ and mx6m_decode_kernel), parameterised on the formats of their two operands
// (mx_op_fp4 / mx_op_fp6 / mx_op_e4m3 of mx_scaled_tile.cuh), as mx_scaled_gemm_tile is on the prefill side.  The weight fragment is the
// A operand in both: a lane's accumulator holds 4 consecutive columns of one row of y.  mxa4_decode_kernel and mxma4_decode_kernel
// (W4A4) take x as the A operand and keep bodies of their own: instantiated on these bodies (FP4 x FP4, the weight as A) they gave the
// same bits on every line of tools/mxfp4_digest.py and needed no more registers, but the dense layer at M = 1 was 4 to 6 % slower in both
// dtypes (profiles/mx_scaled_decode_ab.txt), and these bodies take no orientation switch.
// mx6a8_decode_kernel and mx8a8_decode_kernel (W6A8, W8A8) keep bodies of their own too: on the dense body, which computes the same
// bits, W6A8 was 3.4 % slower at M = 64 with no cause found in the compiled loop, and the 64-row W8A8 instance needed 82 VGPRs where its
// own body needs 69 and lost a wave of occupancy (profiles/mx_scaled_decode_ab.txt, profiles/mx_scaled_decode_resources.txt).
//
// The clamp and mask rules, once.  Of a row in memory (a weight row, or a row of xq) a load is clamped and unconditional, then masked: a
// block index past K / 32 reads block K / 32 - 1, a column past N reads column N - 1, a row past M reads row M - 1, so every address lies
// in the tensor and all loads of a step issue before anything depends on them; then whatever was out of range becomes zero codes under
// scale code 127 (2^0), which contribute +0 to every sum.  A column past N is not masked: it is computed and never stored.  The routed
// body's one x row is loaded by the lanes with (lane & 15) == 0 alone, under the same rule; the other lanes hold zero codes under scale
// code 127.  A skipped slot (idx outside [0, E)) leaves before any address is formed from the index.
#pragma once
#include "mx_scaled_tile.cuh"

namespace bie {

// Where lane group kq's fragment of the 128-k step s lies in a row of KB blocks in Op's format (the decode view of mx_op_*): per part
// its byte offset in the row, the block clamped to KB - 1, and whether the block lies below KB.
template <class Op>
struct mx_step {
    int off[Op::PARTS];
    bool in[Op::PARTS];
    __device__ __forceinline__ mx_step(int s, int kq, int KB) {
#pragma unroll
        for (int i = 0; i < Op::PARTS; i++) {
            const int b = Op::part_block(s, kq, i);
            in[i] = b < KB;
            off[i] = min(b, KB - 1) * Op::BLOCK + Op::part_off(kq);
        }
    }
};

// A lane's fragment of that step of a row.  load() is clamped and unconditional, NT for the weight stream; mask() must follow it and
// turns the parts past K, or all of them for a dead row, into zero codes.
template <class Op>
struct mx_lane {
    typename Op::part_t part[Op::PARTS];

    template <bool NT>
    __device__ __forceinline__ void load(const uint8_t* row, const mx_step<Op>& st) {
#pragma unroll
        for (int i = 0; i < Op::PARTS; i++) part[i] = Op::template part_load<NT>(row + st.off[i]);
    }
    __device__ __forceinline__ void mask(const mx_step<Op>& st, bool dead) {
#pragma unroll
        for (int i = 0; i < Op::PARTS; i++)
            if (dead || !st.in[i]) part[i] = typename Op::part_t{};
    }
    __device__ __forceinline__ mxa4_v8i frag() const { return Op::lane_frag(part); }
};

// An activation format's row quantiser, defined beside its 8-value unit (mxfp4_a4_common.cuh, mxfp4_a8_common.cuh, mxfp6_common.cuh):
// thread t of the 256 takes the units t, t + 256, ... of the row xr and writes the row's K / 32 blocks of codes and K / 32 scale bytes
// through `codes` and `scales` (memory or LDS); `bad` collects a NaN or +-inf for the caller's __syncthreads_or.  The dense quantise
// kernels and the FUSED branch below call the same function, so a FUSED kernel's row image has the bits of the dense kernel's row.
// That holds by construction for FP6 and E4M3.  The FP4 overload has the dense mxa4_quantize_kernel as its only caller:
// mxma4_decode_kernel keeps its own copy of the loop with its body, and a test holds its bits.
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_fp4, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad);
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_fp6, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad);
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_e4m3, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad);

// ---- the dense body -----------------------------------------------------------------------------------------------------------------------------
// Workgroup: columns 16 * blockIdx.x .. + 15, rows 0 .. M - 1 (M <= 16 G).  Wave w takes the 128-k steps w, w + 4, ...; lane l holds
// column (row) l & 15 and lane group l >> 4 of the step on both sides: its fragment of the weights (non-temporal) and of every 16-row
// group of x, and the scale byte of block l >> 4 of either.  One MFMA per 16 rows and 128 k; the four partial tiles are summed in LDS as
// ((w0 + w1) + w2) + w3.  All 256 threads must call it together.
template <int DT, int G, class OpW, class OpX>
__device__ __forceinline__ void mx_scaled_decode_rows(const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                      const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc, const uint8_t* __restrict__ ecol,
                                                      const void* __restrict__ bias, void* __restrict__ y, int M, int N, int K) {
    __shared__ mxa4_v4f red[3][G][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const int wrowb = KB * OpW::BLOCK, xrowb = KB * OpX::BLOCK;  // a row's bytes: at most K
    const int n0 = blockIdx.x * 16;
    const long nl = min(n0 + r16, N - 1);
    const uint8_t* wrow = qw + nl * wrowb;
    const uint8_t* srow = sc + nl * KB;
    mxa4_v4f acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);
        const bool kin = kb < KB;
        const mx_step<OpW> stw(s, kq, KB);
        const mx_step<OpX> stx(s, kq, KB);
        mx_lane<OpW> w;
        w.template load<true>(wrow, stw);
        int sw = __builtin_nontemporal_load(srow + kc);
        mx_lane<OpX> a[G];
        int sa[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int m = min(g * 16 + r16, M - 1);
            a[g].template load<false>(xq + (long)m * xrowb, stx);
            sa[g] = xs[(uint32_t)(m * KB + kc)];  // m < 64 and KB < 2^26: below 2^32
        }
        w.mask(stw, false);
        if (!kin) sw = 127;
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool dead = g * 16 + r16 >= M;
            a[g].mask(stx, dead);
            if (!kin || dead) sa[g] = 127;
        }
        const mxa4_v8i fw = w.frag();
#pragma unroll
        for (int g = 0; g < G; g++)
            acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, a[g].frag(), acc[g], OpW::CODE, OpX::CODE, 0, sw, 0, sa[g]);
    }
    if (wave) {
#pragma unroll
        for (int g = 0; g < G; g++) red[wave - 1][g][lane] = acc[g];
    }
    __syncthreads();
    if (wave) return;
    // C/D: D column (= row m of the 16) = lane & 15, D row (= column n of y) = 4 (lane >> 4) + r: four consecutive n of one row of y (mx_store4)
    const int n = n0 + 4 * kq;
    if (n >= N) return;
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int m = g * 16 + r16;
        if (m >= M) continue;
        const mxa4_v4f p1 = red[0][g][lane], p2 = red[1][g][lane], p3 = red[2][g][lane];
        const bool rbad = row_flag[m] != 0;
        uint16_t* yr = reinterpret_cast<uint16_t*>(y) + (long)m * N;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = ((acc[g][r] + p1[r]) + p2[r]) + p3[r];
        mx_store4<DT>(v, rbad, ecol, bias, n, yr, n, N);
    }
}

// ---- the routed body ----------------------------------------------------------------------------------------------------------------------------
// Workgroup: pair blockIdx.y, columns 16 C16 blockIdx.x .. + 16 C16 - 1 of its expert e = idx[pair] (rows (long)e * N .. of the
// [E * N, K] view).  Wave w takes the 128-k steps w, w + 4, ...; lane l holds column l & 15 of each of the C16 groups and lane group
// l >> 4 of the step's weights (non-temporal); the pair's row is column 0 of the B operand, so the lanes with (l & 15) == 0 hold its
// fragment and scale byte.  The four partial sums meet in LDS and are summed as ((w0 + w1) + w2) + w3, the dense body's order: a pair's
// row has the bits of the dense decode form.  FUSED (K <= ONE_K): xin is x, and the workgroup quantises x_row(pair) into LDS itself
// (mx_quantize_row: K / 32 blocks of codes, then K / 32 scale bytes; the non-finite flag through the barrier) and reads neither xs nor
// row_flag.  Not FUSED: xin is xq.  All 256 threads must call it together.
template <int DT, int C16, bool FUSED, class OpW, class OpX, int ONE_K>
__device__ __forceinline__ void mx_scaled_decode_pair(const void* __restrict__ xin, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ row_flag,
                                                      const int32_t* __restrict__ idx, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                      const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, int S, int E,
                                                      int N, int K, int x_per_pair) {
    constexpr int C = 16 * C16;
    __shared__ float red[4][C];
    __shared__ __attribute__((aligned(16))) unsigned char img[FUSED ? OpX::BLOCK * ONE_K / 32 + ONE_K / 32 : 16];
    static_assert(!FUSED || sizeof(img) == (OpX::BLOCK + 1) * (ONE_K / 32), "the row image: ONE_K / 32 blocks of codes and as many scale bytes");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int p = blockIdx.y, n0 = blockIdx.x * C;
    const int e = idx[p];
    if ((unsigned)e >= (unsigned)E) {  // a skipped slot (uniform): zeros, and no address is formed from e
        if (t < C && n0 + t < N) dt_traits<DT>::store(y, (long)p * N + n0 + t, 0.0f);
        return;
    }
    const int KB = K >> 5, KS = (KB + 3) >> 2;
    const long wrowb = (long)KB * OpW::BLOCK, xrowb = (long)KB * OpX::BLOCK;
    const long xrow = x_per_pair ? p : p / S;
    const uint8_t* xqr;  // the row's code bytes: the LDS image or xq
    const uint8_t* xsr;  // its scale bytes
    int flagged;
    if constexpr (FUSED) {
        int bad = 0;
        mx_quantize_row<DT>(OpX{}, reinterpret_cast<const uint16_t*>(xin) + xrow * K, K, img, img + KB * OpX::BLOCK, bad);
        flagged = __syncthreads_or(bad);  // the barrier that publishes the image
        xqr = img;
        xsr = img + KB * OpX::BLOCK;
    } else {
        xqr = reinterpret_cast<const uint8_t*>(xin) + xrow * xrowb;
        xsr = xs + xrow * KB;
        flagged = row_flag[xrow];
    }
    const long r0 = (long)e * N;  // the expert's first row of the [E * N, K] view
    const uint8_t* wrow[C16];
    const uint8_t* srow[C16];
#pragma unroll
    for (int c = 0; c < C16; c++) {
        const long n = r0 + min(n0 + c * 16 + r16, N - 1);
        wrow[c] = qw + n * wrowb;
        srow[c] = sc + n * KB;
    }
    mxa4_v4f acc[C16];
#pragma unroll
    for (int c = 0; c < C16; c++) acc[c] = mxa4_v4f{0.f, 0.f, 0.f, 0.f};
    for (int s = wave; s < KS; s += 4) {
        const int kb = s * 4 + kq, kc = min(kb, KB - 1);
        const bool kin = kb < KB;
        const mx_step<OpW> stw(s, kq, KB);
        mx_lane<OpW> w[C16];
        int sw[C16];
#pragma unroll
        for (int c = 0; c < C16; c++) {
            w[c].template load<true>(wrow[c], stw);
            sw[c] = __builtin_nontemporal_load(srow[c] + kc);
        }
        mx_lane<OpX> a{};
        int sa = 127;
        if (r16 == 0) {
            const mx_step<OpX> stx(s, kq, KB);
            a.template load<false>(xqr, stx);
            sa = xsr[kc];
            a.mask(stx, false);
            if (!kin) sa = 127;
        }
#pragma unroll
        for (int c = 0; c < C16; c++) {
            w[c].mask(stw, false);
            if (!kin) sw[c] = 127;
        }
        const mxa4_v8i fx = a.frag();
#pragma unroll
        for (int c = 0; c < C16; c++)
            acc[c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w[c].frag(), fx, acc[c], OpW::CODE, OpX::CODE, 0, sw[c], 0, sa);
    }
    // C/D: D column (= row of the x operand) = lane & 15, D row (= column n of the strip) = 4 (lane >> 4) + r: the pair's row is
    // registers 0 .. 3 of lanes 0, 16, 32, 48
    if (r16 == 0) {
#pragma unroll
        for (int c = 0; c < C16; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[wave][c * 16 + 4 * kq + r] = acc[c][r];
    }
    __syncthreads();
    if (t < C) {
        const int n = n0 + t;
        if (n < N) {
            float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
            if (flagged || ecol[r0 + n] == 255u) v = a4_nan();
            if (bias) v += dt_traits<DT>::load(bias, r0 + n);
            dt_traits<DT>::store(y, (long)p * N + n, v);
        }
    }
}

}  // namespace bie
