// Internal helpers shared by the HIP translation units of libbie_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include "../../include/bie_hip.h"

namespace bie {

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef uint32_t uint4_t __attribute__((ext_vector_type(4)));
typedef uint32_t uint2_t __attribute__((ext_vector_type(2)));

// ---- error plumbing --------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);

#define BIE_REQUIRE(cond, code, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            ::bie::set_error(__VA_ARGS__); \
            return (code);                \
        }                                 \
    } while (0)

// zero modes of the MPQ weights (the rounding of each is spelled out in mpq_dequant.cuh)
constexpr int ZM_SYM = 0, ZM_ASYM = 1, ZM_FUSED = 2;

// ---- tuning knobs ---------------------------------------------------------------------------------
// An unset knob reads as `dflt` (a set but empty one as 0).
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// BIE_TUNING (tests, sweep tools) is read once per process; under it the knobs read through BIE_KNOB are re-read on every call.
static inline bool tuning() {
    static const bool t = getenv("BIE_TUNING") != nullptr;
    return t;
}
// A knob read once per process -- or per call under BIE_TUNING.  No getenv on the launch path otherwise.
#define BIE_KNOB(name, dflt) \
    (::bie::tuning() ? ::bie::env_int(name, dflt) : [] { static const int once_ = ::bie::env_int(name, dflt); return once_; }())

// nearest point of an ascending grid in log space (the geometric mean of two neighbours is the boundary); -1 when x is more than
// 20 % outside the grid.  Looks up the measured tables (mpq_gemm_plan_table.inc, mpq_dense_table.inc).
static inline int grid_index(const int* g, int n, long x) {
    if ((double)x * 1.2 < (double)g[0] || (double)x > (double)g[n - 1] * 1.2) return -1;
    int i = 0;
    while (i + 1 < n && (double)x * (double)x > (double)g[i] * (double)g[i + 1]) i++;
    return i;
}

// Wave-wide integer sum on the DPP network (no LDS traffic): quad swaps, half-row and row mirrors, then the two row broadcasts;
// the total lands in lane 63 and is read back as a scalar.
__device__ __forceinline__ int wave_sum_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, false);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, false);  // row_mirror: every lane of a row holds the row's sum
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// ---- 16-bit float <-> float on device, bit-level (torch semantics: RNE) -----------------------
__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ uint32_t f32_to_bf16_bits(float f) {
    // v_cvt_pk_bf16_f32 (RNE, NaN-preserving) -- one instruction for two values; used pairwise below
    bf16x2_t r = __builtin_convertvector(float2_t{f, 0.0f}, bf16x2_t);
    return __builtin_bit_cast(uint32_t, r) & 0xffffu;
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    bf16x2_t r = __builtin_convertvector(float2_t{lo, hi}, bf16x2_t);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ float f16_bits_to_f32(uint32_t h) {
    return (float)__builtin_bit_cast(half_t, (uint16_t)h);
}
__device__ __forceinline__ uint32_t f32_to_f16_bits(float f) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (half_t)f);
}

template <int DT> struct dt_traits;
template <> struct dt_traits<BIE_F16> {
    static __device__ __forceinline__ float load(const void* p, long i) { return f16_bits_to_f32(((const uint16_t*)p)[i]); }
    static __device__ __forceinline__ float round(float v) { return (float)(half_t)v; }
    static __device__ __forceinline__ void store(void* p, long i, float v) { ((uint16_t*)p)[i] = (uint16_t)f32_to_f16_bits(v); }
    static constexpr int bytes = 2;
};
template <> struct dt_traits<BIE_BF16> {
    static __device__ __forceinline__ float load(const void* p, long i) { return bf16_bits_to_f32(((const uint16_t*)p)[i]); }
    static __device__ __forceinline__ float round(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }
    static __device__ __forceinline__ void store(void* p, long i, float v) { ((uint16_t*)p)[i] = (uint16_t)f32_to_bf16_bits(v); }
    static constexpr int bytes = 2;
};
template <> struct dt_traits<BIE_F32> {
    static __device__ __forceinline__ float load(const void* p, long i) { return ((const float*)p)[i]; }
    static __device__ __forceinline__ float round(float v) { return v; }
    static __device__ __forceinline__ void store(void* p, long i, float v) { ((float*)p)[i] = v; }
    static constexpr int bytes = 4;
};

// The ternary layers' per-value epilogue: dt( dt( dt(d) * sa ) * sw ) in the layer dtype (a scale of 1.0 leaves its step exact).
// ternary.hip's decode form and both one-launch ternary convs (binary_conv_fused.hip) round through this one function.
template <int DT>
__device__ __forceinline__ float layer_round(float d, float sa, float sw) {
    return dt_traits<DT>::round(dt_traits<DT>::round(dt_traits<DT>::round(d) * sa) * sw);
}

// Every workspace starts with a 16 KiB head (zero on first use); every scratch user starts behind it.  Two protocols live in it
// and must not share words: the first half holds split-K ARRIVAL TICKETS (one per 64-column output tile, returned to zero
// by the last arriver: mpq_gemv.hip), the second half the tiles' GENERATION words of the tagged-granule reduction
// (monotonic, never reset: mpq_gemv_lut.hip).
constexpr size_t BIE_WS_HEAD_BYTES = 16384;
constexpr int BIE_WS_COUNTERS = (int)(BIE_WS_HEAD_BYTES / 8);  // 2048 tiles = 131072 output columns per launch, each protocol
constexpr int BIE_WS_GEN_OFFSET = BIE_WS_COUNTERS;             // in 32-bit words from the start of the workspace

unsigned next_launch_epoch();  // splitk.hip

// shared split-K epilogue (splitk.hip): y[m][n] = dt( sum_s part[s][m][n] ) (+ bias[n])
int launch_splitk_finalize(const float* part, const void* bias, void* y, int S, int M, int N, int dtype,
                           hipStream_t stream);

}  // namespace bie
