// The MXFP4 format's device-side rules and the instruction wrappers shared by mxfp4.hip and mxfp4_moe.hip (gfx950): E8M0 scale codes to
// fp32, the prefill forms' rebias, the fp4 -> fp16 / bf16 converts with their dot2 and MFMA, the fp32 wave sum on the DPP network, and
// the layout of the expert GEMMs' routing workspace.
#pragma once
#include "mfma_pipe.cuh"

namespace bie {

typedef __bf16 mx_bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 mx_half8_t __attribute__((ext_vector_type(8)));

// E8M0 -> fp32: 2^(s - 127), code 0 the subnormal 2^-127 (not 0.0), code 255 NaN (not +inf, which the plain s << 23 would give)
__device__ __forceinline__ float e8m0_f32(uint32_t s) { return __uint_as_float(s == 0u ? 0x00400000u : s == 255u ? 0x7fc00000u : s << 23); }

// 2^d for d <= 0 as the convert's scale: 0 below 2^-126 (e2m1 * 2^d then lies below every fp16 / bf16 normal the fragments keep)
__device__ __forceinline__ float mx_rebias(uint32_t s, uint32_t e) {
    const int d = (int)s - (int)e;
    return __uint_as_float(d < -126 ? 0u : (uint32_t)(d + 127) << 23);
}

// ---- decode forms: two codes -> two exact 16-bit values (scale 1.0), dot2 into fp32 -----------------------------------------------------
template <int DT> struct mx_pair;
template <> struct mx_pair<BIE_BF16> {
    typedef bf16x2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, SEL); }
    static __device__ __forceinline__ float dot(t a, uint32_t b, float c) { return __builtin_amdgcn_fdot2_f32_bf16(a, __builtin_bit_cast(t, b), c, false); }
};
template <> struct mx_pair<BIE_F16> {
    typedef half2_t t;
    template <int SEL>
    static __device__ __forceinline__ t cvt(uint32_t w) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, SEL); }
    static __device__ __forceinline__ float dot(t a, uint32_t b, float c) { return __builtin_amdgcn_fdot2(a, __builtin_bit_cast(t, b), c, false); }
};

template <int CTRL, int RMASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, RMASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum_f32(float v) {  // wave_sum_dpp's network (bie_common.h) on fp32; the total of lane 63
    v = dpp_add<0xB1, 0xf>(v);
    v = dpp_add<0x4E, 0xf>(v);
    v = dpp_add<0x141, 0xf>(v);
    v = dpp_add<0x140, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v);
    v = dpp_add<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- the routing workspace of the grouped expert GEMMs (mxm_route_kernel of mxfp4_moe.hip writes it; mxfp4_moe.hip and mxfp4_moe_a4.hip read it)
// int32: head [MXM_HEAD], tile_expert [max_tiles], tile_first [max_tiles], tile_rows [max_tiles], pair list [P]
constexpr int MXM_BM = 128;      // rows of a row tile
constexpr int MXM_MAX_E = 1024;  // bins of the routing kernel's scan
constexpr int MXM_HEAD = 4;      // int32 words before the tile table: [0] the tile count

// ---- prefill forms: four code bytes -> one 8-k MFMA fragment at the block's rebiased scale ---------------------------------------------
template <int DT> struct mx_frag;
template <> struct mx_frag<BIE_BF16> {
    typedef mx_bf16x8_t t;
    static __device__ __forceinline__ t cvt(uint32_t w, float s) {
        const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1);
        const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3);
        return t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ float16_t mfma(const t& a, const t& b, const float16_t& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct mx_frag<BIE_F16> {
    typedef mx_half8_t t;
    static __device__ __forceinline__ t cvt(uint32_t w, float s) {
        const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 1);
        const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, 3);
        return t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    static __device__ __forceinline__ float16_t mfma(const t& a, const t& b, const float16_t& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

}  // namespace bie
