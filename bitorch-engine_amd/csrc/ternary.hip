// Ternary-weight / binary-activation linear layer (weights in {-1, 0, +1}, TWN; activations sign(x + bias_a) = +-1) for gfx950.
// No reference implementation exists; the semantics are fixed in include/bie_hip.h and INTEGRATION.md.
//
// Weight format (the checkpoint's qweight): uint8 [2, N, K/8], plane 0 = "non-zero" mask, plane 1 = "value is +1" (a subset of
// plane 0), LSB first (bit j of byte b = k 8b + j) -- two bie_binary_pack_rows_u8 row images.  With s = +-1 the x sign and xbits its
// bit (1 = +1), a word of 32 weights contributes  sum t*s = popc(mask) - 2*popc(mask & (pos ^ xbits)):  a masked position agrees
// (+1) when pos == xbit, else -1.  So  D[m, n] = nnz_n - 2 * popc_k(mask & (pos ^ x)), an exact integer (|D| <= K < 2^24).
//
// Decode form (ternary_fused_kernel, small M): one launch per layer forward after the design of xnor_fused_kernel (binary.hip):
// the workgroup sign-packs ALL M rows of (x + bias_a) into LDS, so each weight word is read from HBM once per launch; a wave takes 4
// output columns at a time, lanes stride the K words (two coalesced dword loads per column and word: mask, pos), per word and row
// v_xor + v_and + v_bcnt (accumulating), and nnz_n is one more v_bcnt per word shared by all rows (recomputed here rather than
// stored: no third tensor in the checkpoint; a lab build without the count, the lower bound of a stored nnz, measured no faster:
// profiles/ternary_decode_probe.txt).  The K-split partials are summed on the DPP network.
// Matrix-pipe form (large M): the two planes become an FP4 (E2M1) image in the fragment order of bie_binary_fp4_image with +1 = 0x2,
// -1 = 0xA and 0 = 0x0, and binary_fp4.hip's GEMM runs against the unchanged x image of bie_binary_fp4_image_from_values with an
// epilogue that reads alpha per column.  Both forms compute the same integers and the same roundings, bit for bit.
#include "bie_common.h"

namespace bie {

int binary_fp4_gemm_colscale_launch(const uint8_t* ximg, const uint8_t* wimg, void* y, long M, long N, long K, const void* sa, const void* sw_vec, int dtype,
                                    int tile, hipStream_t st);  // binary_fp4.hip

// ---- pack / unpack: trits int8 [N, K] <-> qweight [2, N, K/8].  One thread per (row, byte) -------------------------------------------
// Any positive int8 packs as +1, any negative one as -1.  Unpack reads a plane-1 bit only under plane 0, as the kernels do.
__global__ __launch_bounds__(256) void ternary_pack_kernel(const int8_t* __restrict__ t, uint8_t* __restrict__ q, long nbytes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbytes) return;
    uint32_t m = 0, p = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int8_t e = t[i * 8 + j];
        m |= (uint32_t)(e != 0) << j;
        p |= (uint32_t)(e > 0) << j;
    }
    q[i] = (uint8_t)m;
    q[nbytes + i] = (uint8_t)p;
}

__global__ __launch_bounds__(256) void ternary_unpack_kernel(const uint8_t* __restrict__ q, int8_t* __restrict__ t, long nbytes) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nbytes) return;
    const uint32_t m = q[i], p = q[nbytes + i];
#pragma unroll
    for (int j = 0; j < 8; j++) t[i * 8 + j] = ((m >> j) & 1u) ? (((p >> j) & 1u) ? 1 : -1) : 0;
}

// ---- FP4 weight image: 8 (mask, pos) bit pairs -> 8 E2M1 nibbles (0x0 / 0x2 / 0xA) -------------------------------------------------
__device__ __forceinline__ uint32_t spread4(uint32_t b) {  // bit j of the low byte -> bit 4j
    uint32_t x = b & 0xffu;
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    return (x | (x << 3)) & 0x11111111u;
}
__device__ __forceinline__ uint32_t fp4_from_trits8(uint32_t m, uint32_t p) {
    const uint32_t sign = 0xaaaaaaaau ^ (spread4(p) << 3);  // 0x2 where +1, 0xA where -1
    return sign & (spread4(m) * 0xfu);                       // 0x0 where the mask is clear
}

// The fragment order of fp4_image_kernel (binary_fp4.hip): fragment f = (row block rb, k half-tile kb), lane l owns row 32*rb + (l & 31),
// k 64*kb + 32*(l >> 5) .. +31 = one 32-bit word of each plane; rows past N and k past K are 0.0 nibbles.  K % 32 == 0: a lane's word
// lies wholly inside the row or wholly past it.
__global__ __launch_bounds__(256) void ternary_fp4_image_kernel(const uint8_t* __restrict__ q, uint4_t* __restrict__ img, long N, long row_bytes, long nfrag,
                                                                int kb_per_row) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= nfrag) return;
    const int lane = threadIdx.x & 63;
    const long rb = f / kb_per_row;
    const int kb = (int)(f - rb * kb_per_row);
    const long row = rb * 32 + (lane & 31);
    const long b0 = (long)kb * 8 + (lane >> 5) * 4;
    uint4_t o = {0u, 0u, 0u, 0u};
    if (row < N && b0 < row_bytes) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(q + row * row_bytes + b0);
        const uint32_t p = *reinterpret_cast<const uint32_t*>(q + (N + row) * row_bytes + b0);
        o = uint4_t{fp4_from_trits8(m, p), fp4_from_trits8(m >> 8, p >> 8), fp4_from_trits8(m >> 16, p >> 16), fp4_from_trits8(m >> 24, p >> 24)};
    }
    img[f * 64 + lane] = o;
}

// ---- decode form ----------------------------------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void tern_load8(const void* p, long i, float (&v)[8]) {
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

// y[m][n] = dt( dt( dt(D) * scale_a ) * alpha[n] ) (scale_a / alpha NULL = 1), or with y_f32 the fp32 D.  ROWS >= M: every row of x is in
// the one workgroup row block.  The sign of fl(x + b) in the layer dtype is the sign of the fp32 sum (only exact cancellation gives 0,
// and 0 >= 0 either way).
constexpr int ROWS = 4;

template <int DT>
__global__ __launch_bounds__(256) void ternary_fused_kernel(const void* __restrict__ x, const void* __restrict__ bias_a, const uint32_t* __restrict__ Wm,
                                                            const uint32_t* __restrict__ Wp, const void* __restrict__ scale_a, const void* __restrict__ alpha,
                                                            void* __restrict__ y, int M, int N, int K, int cols_per_wg, int y_f32) {
    extern __shared__ uint32_t xb[];  // [ROWS][KW + 1]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KW = K >> 5, XS = KW + 1, KB = K >> 3;
    uint8_t* xbytes = reinterpret_cast<uint8_t*>(xb);
    for (int t = threadIdx.x; t < ROWS * KB; t += 256) {
        const int r = t / KB, kb = t - r * KB;
        uint32_t bits = 0;
        if (r < M) {
            float v[8];
            tern_load8<DT>(x, (long)r * K + kb * 8, v);
            if (bias_a) {
                float b[8];
                tern_load8<DT>(bias_a, kb * 8, b);
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] += b[q];
            }
#pragma unroll
            for (int q = 0; q < 8; q++) bits |= (uint32_t)(v[q] >= 0.0f) << q;
        }
        xbytes[r * XS * 4 + kb] = (uint8_t)bits;
    }
    __syncthreads();
    const float sa = scale_a ? dt_traits<DT>::load(scale_a, 0) : 1.0f;
    const int col0 = blockIdx.x * cols_per_wg;
    const int col1 = min(N, col0 + cols_per_wg);
    for (int nb = col0 + wave * 4; nb < col1; nb += 16) {  // 4 columns at a time: their 8 loads are in flight together
        int acc[4][ROWS] = {};
        int nnz[4] = {0, 0, 0, 0};
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
#ifndef BIE_TERNARY_NNZ_LAB  // lab build (timing only, D is wrong): no nnz count at all, a lower bound for an nnz stored at pack time
#pragma unroll
            for (int c = 0; c < 4; c++) nnz[c] += __builtin_popcount(m[c]);
#endif
#pragma unroll
            for (int r = 0; r < ROWS; r++) {  // rows >= M hold zero bits: counted, never stored
                const uint32_t xv = xb[r * XS + k];
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c][r] += __builtin_popcount(m[c] & (p[c] ^ xv));
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int n = nb + c;
            const int nz = wave_sum_dpp(nnz[c]);
            const float aw = (alpha && !y_f32) ? dt_traits<DT>::load(alpha, min(n, N - 1)) : 1.0f;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                if (r >= M) continue;  // M is wave-uniform
                const int d = nz - 2 * wave_sum_dpp(acc[c][r]);
                if (lane == 0 && n < col1) {
                    float v = (float)d;
                    if (y_f32) {
                        ((float*)y)[(long)r * N + n] = v;
                    } else {
                        dt_traits<DT>::store(y, (long)r * N + n, layer_round<DT>(v, sa, aw));  // sa / aw are 1.0 where NULL
                    }
                }
            }
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------
int ternary_pack_launch(const int8_t* trits, uint8_t* qweight, long N, long K, hipStream_t st) {
    const long nbytes = N * (K / 8);
    hipLaunchKernelGGL(ternary_pack_kernel, dim3((unsigned)cdivl(nbytes, 256)), dim3(256), 0, st, trits, qweight, nbytes);
    return check_launch("ternary_pack_kernel");
}

int ternary_unpack_launch(const uint8_t* qweight, int8_t* trits, long N, long K, hipStream_t st) {
    const long nbytes = N * (K / 8);
    hipLaunchKernelGGL(ternary_unpack_kernel, dim3((unsigned)cdivl(nbytes, 256)), dim3(256), 0, st, qweight, trits, nbytes);
    return check_launch("ternary_unpack_kernel");
}

int ternary_fp4_image_launch(const uint8_t* qweight, uint8_t* image, long N, long K, hipStream_t st) {
    const long kb_per_row = 2 * cdivl(K, 128), nfrag = cdivl(N, 32) * kb_per_row;
    hipLaunchKernelGGL(ternary_fp4_image_kernel, dim3((unsigned)cdivl(nfrag, 4)), dim3(256), 0, st, qweight, (uint4_t*)image, N, K / 8, nfrag, (int)kb_per_row);
    return check_launch("ternary_fp4_image_kernel");
}

// The decode form serves M <= ROWS = 4.  Measured against the matrix-pipe form on the MI355X (tools/ternary_bench.py, profiles/ternary_bench.jsonl,
// profiles/ternary_bench_16rows.jsonl): ahead at M = 1..4 on 4096 x 4096, 4096 -> 11008 and 11008 -> 4096 in fp16 and bf16.  A 16-row instance
// was ahead at M = 8 only on 4096 x 4096 (17.1 / 18.0 against 21.9 / 22.0 us, fp16 / bf16), behind at M = 8 on both 11008 shapes (33 - 38 against
// 22 - 34 us) and behind at M = 16 on all three (25 - 57 against 22 - 34 us): one shape-independent bound, 4.  The x bits of the ROWS rows sit in
// one workgroup's LDS, which bounds K.
bool ternary_linear_fused_ok(long M, long N, long K) {
    return M >= 1 && M <= ROWS && N >= 1 && N < (1L << 31) && K >= 32 && K % 32 == 0 && K < (1L << 24) && (size_t)ROWS * (K / 32 + 1) * 4 <= 65536;
}

template <int DT>
static void ternary_fused_launch_dt(const void* x, const void* bias_a, const uint8_t* q, const void* sa, const void* alpha, void* y, int M, int N, int K,
                                    int y_f32, hipStream_t st) {
    const size_t lds = (size_t)ROWS * (K / 32 + 1) * 4;
    // up to 1024 column blocks of at least the 16 columns one sweep of the 4 waves covers: every wave has one quad of columns in flight
    // (4096 -> 11008, M = 1 and 4: 11.2 us per launch against 16.0 with 256 blocks, profiles/ternary_decode_probe.txt; each block repeats the
    // packing of x, an L2 read)
    const int cols = (int)cdivl(cdivl(N, 1024), 16) * 16;
    const dim3 grid((unsigned)cdivl(N, cols));
    const uint32_t* wm = reinterpret_cast<const uint32_t*>(q);
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(q + (size_t)N * (K / 8));
    hipLaunchKernelGGL(ternary_fused_kernel<DT>, grid, dim3(256), lds, st, x, bias_a, wm, wp, sa, alpha, y, M, N, K, cols, y_f32);
}

int ternary_linear_fused_launch(const void* x, const void* bias_a, const uint8_t* q, const void* sa, const void* alpha, void* y, long M, long N, long K,
                                int dtype, int y_f32, hipStream_t st) {
    if (dtype == BIE_F16) ternary_fused_launch_dt<BIE_F16>(x, bias_a, q, sa, alpha, y, (int)M, (int)N, (int)K, y_f32, st);
    else if (dtype == BIE_BF16) ternary_fused_launch_dt<BIE_BF16>(x, bias_a, q, sa, alpha, y, (int)M, (int)N, (int)K, y_f32, st);
    else ternary_fused_launch_dt<BIE_F32>(x, bias_a, q, sa, alpha, y, (int)M, (int)N, (int)K, y_f32, st);
    return check_launch("ternary_fused_kernel");
}

int ternary_layer_fp4_launch(const uint8_t* ximg, const uint8_t* wimg, const void* sa, const void* alpha, void* y, long M, long N, long K, int dtype,
                             hipStream_t st) {
    return binary_fp4_gemm_colscale_launch(ximg, wimg, y, M, N, K, sa, alpha, dtype, 0, st);
}

}  // namespace bie
