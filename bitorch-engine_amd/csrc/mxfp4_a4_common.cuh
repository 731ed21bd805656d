// The device-side pieces shared by the W4A4 translation units (mxfp4_a4.hip, mxfp4_moe_a4.hip; gfx950): the operand types of the
// block-scaled matrix instructions, and the activation quantiser's rule for one 8-value unit, so that a kernel that quantises a row
// itself produces the bits of mxa4_quantize_kernel.
#pragma once
#include "mfma_pipe.cuh"

namespace bie {

typedef int mxa4_v8i __attribute__((ext_vector_type(8)));
typedef float mxa4_v4f __attribute__((ext_vector_type(4)));

// |a| -> E2M1 magnitude index, round to nearest, ties to the even index, saturating at 6 (mx_round_e2m1 of mxfp4.hip, restated)
__device__ __forceinline__ uint32_t a4_round_e2m1(float a) {
    return a <= 0.25f ? 0u : a < 0.75f ? 1u : a <= 1.25f ? 2u : a < 1.75f ? 3u : a <= 2.5f ? 4u : a < 3.5f ? 5u : a <= 5.0f ? 6u : 7u;
}

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
        const uint32_t bits = __float_as_uint(amax);
        const int ex = (int)(bits >> 23);
        const int fl = ex ? ex - 127 : (31 - __builtin_clz(bits & 0x7fffffu)) - 149;  // floor(log2(amax))
        const int e = min(max(fl - 2, -127), 127);
        scode = (uint32_t)(e + 127);
        const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
#pragma unroll
        for (int i = 0; i < 8; i++) codes |= (a4_round_e2m1(fabsf(v[i] * inv)) | ((__float_as_uint(v[i]) >> 28) & 8u)) << (4 * i);
    }
}

}  // namespace bie
