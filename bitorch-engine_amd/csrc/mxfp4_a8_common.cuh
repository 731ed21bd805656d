// The device-side piece of the translation units with MXFP8 (E4M3) activations (mxfp4_a8.hip, mxfp4_moe_a8.hip, mxfp6_a8.hip,
// mxfp6_moe_a8.hip, mxfp8_a8.hip; gfx950): the activation quantiser's rule for one 8-value unit and for a row, so that a kernel that
// quantises a row itself (mxma8_decode_kernel, mx6m_decode_kernel) produces the bits of mxa8_quantize_kernel.  The E4M3 operand of the instructions (a8_frag, mx_op_e4m3) and
// the prefill tile body are those of mx_scaled_tile.cuh.
#pragma once
#include "mxfp4_a4_common.cuh"

namespace bie {

// A block's scale from its largest magnitude amax > 0 with E4M3 elements (emax = 8): mx_block_scale's rule with - 8 in place of - 2.
// e <= 119 for any finite amax, so inv = 2^-e is normal and v * inv an exact power-of-two multiply.
__device__ __forceinline__ uint32_t mxa8_block_scale(float amax, float& inv) {
    const uint32_t bits = __float_as_uint(amax);
    const int ex = (int)(bits >> 23);
    const int fl = ex ? ex - 127 : (31 - __builtin_clz(bits & 0x7fffffu)) - 149;  // floor(log2(amax))
    const int e = min(max(fl - 8, -127), 127);
    inv = __uint_as_float((uint32_t)(127 - e) << 23);
    return (uint32_t)(e + 127);
}

// v * inv -> the value handed to the convert: magnitude clamped to 448 (the largest E4M3 value) here, so that the result does not depend
// on the convert's overflow mode and no NaN code is ever produced; the sign of v is kept (-0.0 -> 0x80).
__device__ __forceinline__ float a8_clamp(float v, float inv) {
    return __uint_as_float(__float_as_uint(fminf(fabsf(v * inv), 448.0f)) | (__float_as_uint(v) & 0x80000000u));
}

// One 8-value unit (16 bytes of x) of a block of 32 whose four units sit on the four lanes of a quad: the block maximum over the quad on
// the DPP network, the block's E8M0 code and this lane's 8 bytes of E4M3 codes (round to nearest even, OCP e4m3fn).  `bad` collects a NaN
// or +-inf.  All lanes of the quad must call it together.
template <int DT>
__device__ __forceinline__ void a8_quantize_unit(const uint4_t& raw, int& bad, uint2_t& codes, uint32_t& scode) {
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
    codes = uint2_t{0u, 0u};
    scode = 0u;
    if (amax > 0.0f) {
        float inv;
        scode = mxa8_block_scale(amax, inv);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[0], inv), a8_clamp(v[1], inv), lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[2], inv), a8_clamp(v[3], inv), lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[4], inv), a8_clamp(v[5], inv), hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(a8_clamp(v[6], inv), a8_clamp(v[7], inv), hi, true);
        codes = uint2_t{(uint32_t)lo, (uint32_t)hi};
    }
}

// A row of x to MXFP8 (mx_quantize_row of mx_scaled_decode.cuh): 8 bytes of codes per unit, the block's scale byte from the quad's lane 0.
// U = K / 8 is a multiple of 4 and the stride is 256: whole quads are in or out.
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_e4m3, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad) {
    const int U = K >> 3;
    for (int u = threadIdx.x; u < U; u += 256) {
        uint2_t c;
        uint32_t scode;
        a8_quantize_unit<DT>(*reinterpret_cast<const uint4_t*>(xr + (long)u * 8), bad, c, scode);
        reinterpret_cast<uint2_t*>(codes)[u] = c;
        if ((u & 3) == 0) scales[u >> 2] = (uint8_t)scode;
    }
}

}  // namespace bie
