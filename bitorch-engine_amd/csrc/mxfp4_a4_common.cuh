// The device-side piece shared by the W4A4 translation units (mxfp4_a4.hip, mxfp4_moe_a4.hip; gfx950): the activation quantiser's rule
// for one 8-value unit and for a row, so that a kernel that quantises a row itself produces the bits of mxa4_quantize_kernel.  The
// operand types of the block-scaled matrix instructions and the prefill tile body are those of mx_scaled_tile.cuh, the shared decode
// bodies those of mx_scaled_decode.cuh.
#pragma once
#include "mx_scaled_decode.cuh"

namespace bie {

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

// A row of x to MXFP4 (mx_quantize_row of mx_scaled_decode.cuh): a dword of codes per unit, the block's scale byte from the quad's lane 0.
// U = K / 8 is a multiple of 4 and the stride is 256: whole quads are in or out.
template <int DT>
__device__ __forceinline__ void mx_quantize_row(mx_op_fp4, const uint16_t* xr, int K, uint8_t* codes, uint8_t* scales, int& bad) {
    const int U = K >> 3;
    for (int u = threadIdx.x; u < U; u += 256) {
        uint32_t c, scode;
        a4_quantize_unit<DT>(*reinterpret_cast<const uint4_t*>(xr + (long)u * 8), bad, c, scode);
        reinterpret_cast<uint32_t*>(codes)[u] = c;
        if ((u & 3) == 0) scales[u >> 2] = (uint8_t)scode;
    }
}

}  // namespace bie
