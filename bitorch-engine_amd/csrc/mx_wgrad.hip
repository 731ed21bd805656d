// Weight gradient of the weight-only MX linear layers for gfx950: gw = gy^T . x (and gb = sum_m gy) for the backward of MXFP4LinearCuda,
// MXFP6LinearCuda and MXFP8LinearCuda (include/bie_hip.h, INTEGRATION.md "MX weight gradient").  The latent weight is a float tensor, so
// one kernel serves the three formats.  No reference implementation exists.
//
//   gw[n, k] = odt( sum_m gy[m, n] * x[m, k] )     gy [M, N], x [M, K] fp16 / bf16, row-major;  gw [N, K]
//   gb[n]    = odt( sum_m gy[m, n] )               optional
//   products exact in fp32 (two 16-bit significands), the sum in fp32 in an order fixed by (M, N, K, splits) alone, one rounding to odt
//   (the dtype, or fp32).  No atomics: two calls with the same arguments give the same bits.
//
// The contraction runs over M, the STRIDED dimension of both operands: v_mfma_f32_32x32x16_{f16,bf16} wants a lane to hold 8 consecutive
// m of one n (one k), and memory holds 8 consecutive n (k) of one m.  Neither operand is transposed in global memory and none is widened:
// a slab gy[m0 : m0 + 32, 128 n] and x[m0 : m0 + 32, 128 k] is staged into LDS as it lies in memory (16-byte loads along n and k, one
// ds_write_b128 each), and both fragments are built by the hardware's transposed LDS read, ds_read_b64_tr_b16 (mx6_tr2 of
// mxfp6_common.cuh, where its lane layout is written down): lane 4 q + p of a 16-lane group gives the address of slab row q, columns
// 4 p .. + 3 of a 4 x 16 block and receives the 4 rows of column (lane & 15), so two reads (rows 8 h .. + 3 and + 4 .. + 7) are the 8 m
// that lane (r = lane & 31, h = lane >> 5) owes the instruction for column r.  gy^T is the A operand (rows n) and x the B operand
// (columns k): an accumulator register holds one n and the lanes run along k, so a store instruction writes two runs of 32 adjacent k.
//
// Tile 128 n x 128 k, 4 waves as 2 x 2, wave tile 64 x 64 (2 x 2 MFMA blocks, 64 accumulators), slab BM = 32 m = two 16-m steps; per
// step a lane issues 8 transposed reads for 4 MFMAs.  A slab row is 256 bytes with no pad; its 64-byte chunk c (32 columns) is stored at
// chunk c ^ (m & 3).  Banks ((a / 4) mod 64): a transposed read is served per half-wave, which reads 4 rows m = 4 j + q (q = 0 .. 3) and
// 32 columns of one chunk c: the stored chunks c ^ q are distinct, 4 x 64 bytes cover the 64 banks once: no conflict.  A ds_write_b128 is
// served per 8 lanes, which hold 8 adjacent pieces of one row: 128 contiguous bytes up to the order of two chunks: no conflict.
// Double-buffered over m: the next slab's 4 x 16 bytes per thread are in flight while the MFMAs run, one barrier per slab.
// LDS: 2 buffers x (8 KiB gy + 8 KiB x) + 1 KiB for the bias sum = 33792 bytes.  mx_wgrad_kernel: 104 VGPRs + 64 AGPRs with gw in the
// dtype, 82 + 64 with gw in fp32 (both dtypes), no scratch, 3 waves per SIMD (profiles/mx_wgrad_resources.txt), so workgroups share a
// CU and cover each other's barrier.
//
// Edges.  Any M: rows past the slice's end are stored to LDS as zeros (every slab is written whole, so stale LDS is never multiplied).
// Any N: where N % 8 != 0 or gy is not 16-byte aligned a gy row starts on a 2-byte boundary only, and the slab is loaded by 16-bit
// loads, each guarded by n < N (`vec` = 0).  K % 32 == 0 and x 16-byte aligned, so x always loads whole pieces.  Columns past N / K load
// as zeros and are masked on store.  Row offsets are 64-bit.  Non-finite inputs go through the products as they are: a NaN in gy[m, n]
// is in the A fragment of row n alone, so it reaches row n of gw and gb[n] and nothing else.
//
// Split over M.  N K / 128^2 tiles are often fewer than the 256 CUs can hold, so the plan cuts the ceil(M / 32) slabs into S slices of
// ceil(slabs / S) slabs (the last ones may be partial or empty: an empty slice stores +0).  S = 1 rounds and stores gw / gb directly.
// S > 1: slice s stores fp32 partials to the workspace ([S][N K] of gw, then [S][N] of gb) and mx_wgrad_reduce_kernel adds the slices
// in slice order and rounds once.  The bias gradient is fused: the workgroups of k-tile 0 column-sum the gy slab they hold in LDS
// (thread t: column t & 127, rows 16 (t >> 7) .. + 15 of every slab in m order; the two halves are added at the end).
//
// The plan (mx_wgrad_splits), a function of (M, N, K) alone, measured on an MI355X (tools/mx_wgrad_bench.py,
// profiles/mx_wgrad_bench.jsonl): S = the largest value that keeps tiles * S <= 512 workgroups (two per CU) and leaves a slice at least
// 8 slabs (256 rows), at least 1.  The sweep (fp16, M = 2048 and 8192, S forced to 1 .. 64, us per call, eager, with the bias sum):
//   tiles    M      S = 1     2      4      8     16     32     64     plan
//      1   8192     178.8   93.5   50.6   29.7   21.1   20.2   24.4      32
//     16   8192     179.0   94.2   51.3   30.9   23.5   24.7   39.0      32      (5 % over the best)
//     64   8192     185.1  112.2   63.5   44.4   59.6   71.7  123.8       8
//     64   2048      48.7   30.5   21.9   21.0   31.0   48.2   99.6       8
//    128   8192     216.1  119.8   76.6   90.9  100.2  159.4              4
//    256   8192     217.5  131.4  145.2  144.6  202.4                     2
//   1024   8192     453.3  416.3  467.6                                   1      (8 % over the best; at M = 2048 S = 1 is the best)
// The plan picks the fastest measured S in every other row of the file.  On the Llama-7B shapes (4096 x 4096, 11008 x 4096,
// 4096 x 11008; M = 512, 2048, 8192; S = 1 throughout) the kernel with the bias sum takes 0.17 .. 0.24 of the time of the torch
// composition it replaces (two fp32 copies, an fp32 product, a reduction): 36 us / 168 us at 4096 x 4096, M = 512 and 1020 us / 5325 us
// at 11008 x 4096, M = 8192, i.e. 480 .. 745 TFLOP/s; fp16 and bf16 agree within 3 %.
#include "mxfp6_common.cuh"

#pragma clang fp contract(off)

namespace bie {

constexpr int WG_BN = 128, WG_BK = 128, WG_BM = 32;
constexpr int WG_PITCH = 256;                 // bytes per slab row: 128 16-bit values, no pad (the chunk swizzle spreads the banks)
constexpr int WG_SLAB = WG_BM * WG_PITCH;     // 8 KiB per operand and buffer
// the plan: at most this many workgroups (two per CU), and at least this many slabs (256 rows of M) per slice
constexpr long WG_PLAN_WGS = 512, WG_PLAN_SLABS = 8;

// byte offset of the 16-byte piece (8 columns) `piece` of slab row m
__device__ __forceinline__ int wg_off(int m, int piece) { return m * WG_PITCH + ((((piece >> 2) ^ (m & 3))) << 6) + ((piece & 3) << 4); }

// 8 columns col .. + 7 of a row of `ncols`: one 16-byte load where the row is piece-aligned, else 16-bit loads guarded by the row's end
__device__ __forceinline__ uint4_t wg_piece(const uint16_t* __restrict__ row, int col, int ncols, bool vec) {
    if (col >= ncols) return uint4_t{0u, 0u, 0u, 0u};
    if (vec) return *reinterpret_cast<const uint4_t*>(row + col);
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = col + j < ncols ? row[col + j] : 0u;
    return uint4_t{v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16, v[6] | v[7] << 16};
}

// A workgroup per (slice s, n-tile, k-tile), the k-tiles adjacent so that neighbours share the gy slab.  out_gw / out_gb: gw / gb
// (S = 1, stride 0) or the fp32 partials of slice 0 (stride N K / N elements per slice); out_gb NULL = no bias gradient.
template <int DT, int ODT>
__global__ __launch_bounds__(256) void mx_wgrad_kernel(const uint16_t* __restrict__ gy, const uint16_t* __restrict__ x, void* __restrict__ out_gw,
                                                       void* __restrict__ out_gb, long stride_gw, long stride_gb, int M, int N, int K, int tn, int tk,
                                                       int per, int vec) {
    typedef mx_frag<DT> F;
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * WG_SLAB];
    __shared__ float gbs[256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wn = wave >> 1, wk = wave & 1;
    int b = blockIdx.x;
    const int tile_k = b % tk;
    b /= tk;
    const int tile_n = b % tn, s = b / tn;
    const int n0 = tile_n * WG_BN, k0 = tile_k * WG_BK;
    const int slabs = (M + WG_BM - 1) / WG_BM;
    const int sl0 = min(s * per, slabs), sl1 = min(sl0 + per, slabs);  // uniform
    const bool with_gb = out_gb != nullptr && tile_k == 0;            // uniform

    // staging: thread t holds piece t & 15 of slab rows (t >> 4) and (t >> 4) + 16, of both operands
    const int piece = t & 15, r0 = t >> 4;
    uint4_t ra[2], rb[2];
    auto fetch = [&](int sl) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long m = (long)sl * WG_BM + r0 + 16 * j;
            const bool live = m < M;
            ra[j] = live ? wg_piece(gy + m * N, n0 + piece * 8, N, vec != 0) : uint4_t{0u, 0u, 0u, 0u};
            rb[j] = live ? wg_piece(x + m * K, k0 + piece * 8, K, true) : uint4_t{0u, 0u, 0u, 0u};
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int o = buf * 2 * WG_SLAB + wg_off(r0 + 16 * j, piece);
            *reinterpret_cast<uint4_t*>(lds + o) = ra[j];
            *reinterpret_cast<uint4_t*>(lds + WG_SLAB + o) = rb[j];
        }
    };

    // fragment addresses: slab row 8 h + q (+ 4 for the second read, + 16 for the second step), 8 bytes at column 16 g + 4 p of a 32-column chunk
    const int q = (lane >> 2) & 3, h = lane >> 5;
    const int frow = (8 * h + q) * WG_PITCH, fcol = ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
    int offa[2], offb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        offa[i] = frow + (((wn * 2 + i) ^ q) << 6) + fcol;
        offb[i] = WG_SLAB + frow + (((wk * 2 + i) ^ q) << 6) + fcol;
    }
    // the bias sum: column t & 127, slab rows 16 (t >> 7) .. + 15
    const int gcol = t & 127, grow = (t >> 7) * 16;

    float16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    float gsum = 0.0f;

    if (sl0 < sl1) {
        fetch(sl0);
        stash(0);
    }
    __syncthreads();
    for (int sl = sl0; sl < sl1; ++sl) {  // uniform: EXEC is all ones at the transposed reads
        const int buf = (sl - sl0) & 1;
        const unsigned char* base = lds + buf * 2 * WG_SLAB;
        if (sl + 1 < sl1) fetch(sl + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const unsigned char* st = base + ks * 16 * WG_PITCH;
            typename F::t a[2], w[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = mx6_dg<DT>::tr2(st + offa[i], st + offa[i] + 4 * WG_PITCH);
                w[i] = mx6_dg<DT>::tr2(st + offb[i], st + offb[i] + 4 * WG_PITCH);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = F::mfma(a[i], w[j], acc[i][j]);
        }
        if (with_gb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = grow + r;
                gsum += dt_traits<DT>::load(base + m * WG_PITCH + (((gcol >> 5) ^ (m & 3)) << 6), gcol & 31);
            }
        }
        if (sl + 1 < sl1) stash(buf ^ 1);
        __syncthreads();
    }

    // epilogue: register e of block (i, j) is row 8 (e / 4) + 4 h + e % 4 (n), column lane & 31 (k)
    char* og = reinterpret_cast<char*>(out_gw) + (long)s * stride_gw * dt_traits<ODT>::bytes;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + wk * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + wn * 64 + i * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
                if (n < N && k < K) dt_traits<ODT>::store(og, (long)n * K + k, acc[i][j][e]);
            }
        }
    if (with_gb) {
        gbs[t] = gsum;
        __syncthreads();
        if (t < 128 && n0 + t < N)
            dt_traits<ODT>::store(reinterpret_cast<char*>(out_gb) + (long)s * stride_gb * dt_traits<ODT>::bytes, n0 + t, gbs[t] + gbs[t + 128]);
    }
}

// gw[i] = odt( part[0][i] + part[1][i] + ... ) in slice order, four elements per thread (N K % 4 == 0); the threads past N K / 4 do gb.
template <int ODT>
__global__ __launch_bounds__(256) void mx_wgrad_reduce_kernel(const float* __restrict__ part, void* __restrict__ gw, void* __restrict__ gb, long NK, int N,
                                                              int S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, n4 = NK >> 2;
    if (i < n4) {
        const float4_t* p = reinterpret_cast<const float4_t*>(part) + i;
        float4_t a = p[0];
        for (int s = 1; s < S; ++s) {
            const float4_t v = p[(long)s * n4];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        dt_traits<ODT>::store(gw, 4 * i, a.x);
        dt_traits<ODT>::store(gw, 4 * i + 1, a.y);
        dt_traits<ODT>::store(gw, 4 * i + 2, a.z);
        dt_traits<ODT>::store(gw, 4 * i + 3, a.w);
    } else if (gb != nullptr && i - n4 < N) {
        const float* p = part + (long)S * NK + (i - n4);
        float a = p[0];
        for (int s = 1; s < S; ++s) a += p[(long)s * N];
        dt_traits<ODT>::store(gb, i - n4, a);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
long mx_wgrad_max_splits(long M) { return cdivl(M, WG_BM); }

int mx_wgrad_splits(long M, long N, long K) {
    const long tiles = cdivl(N, WG_BN) * cdivl(K, WG_BK), slabs = cdivl(M, WG_BM);
    const long s = std::min(WG_PLAN_WGS / tiles, slabs / WG_PLAN_SLABS);
    return (int)std::max(1L, s);
}

size_t mx_wgrad_workspace_bytes(long N, long K, int S) {
    if (S <= 1) return 0;
    return (((size_t)S * ((size_t)N * K + N) * 4) + 15) & ~(size_t)15;
}

template <int DT, int ODT>
static void mx_wgrad_main(const uint16_t* gy, const uint16_t* x, void* og, void* ob, long sgw, long sgb, long M, long N, long K, int S, hipStream_t st) {
    const int tn = (int)cdivl(N, WG_BN), tk = (int)cdivl(K, WG_BK);
    const int per = (int)cdivl(cdivl(M, WG_BM), S);
    const int vec = (N % 8 == 0 && reinterpret_cast<uintptr_t>(gy) % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL((mx_wgrad_kernel<DT, ODT>), dim3((unsigned)((long)tn * tk * S)), dim3(256), 0, st, gy, x, og, ob, sgw, sgb, (int)M, (int)N, (int)K, tn,
                       tk, per, vec);
}

int mx_wgrad_launch(const void* gy, const void* x, void* gw, void* gb, void* workspace, long M, long N, long K, int dtype, int out_fp32, int S,
                    hipStream_t st) {
    const uint16_t *g = reinterpret_cast<const uint16_t*>(gy), *xs = reinterpret_cast<const uint16_t*>(x);
    if (S == 1) {
        if (dtype == BIE_F16) {
            if (out_fp32) mx_wgrad_main<BIE_F16, BIE_F32>(g, xs, gw, gb, 0, 0, M, N, K, 1, st);
            else mx_wgrad_main<BIE_F16, BIE_F16>(g, xs, gw, gb, 0, 0, M, N, K, 1, st);
        } else {
            if (out_fp32) mx_wgrad_main<BIE_BF16, BIE_F32>(g, xs, gw, gb, 0, 0, M, N, K, 1, st);
            else mx_wgrad_main<BIE_BF16, BIE_BF16>(g, xs, gw, gb, 0, 0, M, N, K, 1, st);
        }
        return check_launch("mx_wgrad_kernel");
    }
    float* part = reinterpret_cast<float*>(workspace);
    void* pb = gb ? part + (long)S * N * K : nullptr;
    if (dtype == BIE_F16) mx_wgrad_main<BIE_F16, BIE_F32>(g, xs, part, pb, N * K, N, M, N, K, S, st);
    else mx_wgrad_main<BIE_BF16, BIE_F32>(g, xs, part, pb, N * K, N, M, N, K, S, st);
    const int rc = check_launch("mx_wgrad_kernel");
    if (rc) return rc;
    const dim3 grid((unsigned)cdivl(N * K / 4 + N, 256));
    if (out_fp32) hipLaunchKernelGGL((mx_wgrad_reduce_kernel<BIE_F32>), grid, dim3(256), 0, st, part, gw, gb, N * K, (int)N, S);
    else if (dtype == BIE_F16) hipLaunchKernelGGL((mx_wgrad_reduce_kernel<BIE_F16>), grid, dim3(256), 0, st, part, gw, gb, N * K, (int)N, S);
    else hipLaunchKernelGGL((mx_wgrad_reduce_kernel<BIE_BF16>), grid, dim3(256), 0, st, part, gw, gb, N * K, (int)N, S);
    return check_launch("mx_wgrad_reduce_kernel");
}

}  // namespace bie
