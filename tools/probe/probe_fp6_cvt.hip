// What v_cvt_scalef32_pk32_{bf16,f16}_fp6 does on gfx950, for the MXFP6 input-gradient tile (mx6_dgrad_tile, csrc/mxfp6_common.cuh): six
// VGPRs (a block of 32 E2M3 codes, code j in bits 6 j .. 6 j + 5 of the little-endian 192 bits) -> 16 VGPRs (32 16-bit values), one fp32 scale.
//   (a) the element map: 32 distinct codes in the block; for every output element the position j whose value came out is printed (nothing
//       is assumed about the order), then all 64 codes at every position are compared with e2m3(code) exactly, scale 1.0
//   (b) the scale: powers of two 2^d, d = 0 .. -11 (every result a normal fp16 number for any nonzero code), compared exactly
//   (c) below the fp16 normal range: the smallest code (0.125) and 1.875 under 2^d, d = -12 .. -26; what comes out is printed beside the
//       exact value (an fp16 subnormal where representable).  The same for bf16 at d = -124 .. -126
//   (d) whether v_mfma_f32_32x32x16_f16 keeps a subnormal fp16 B operand: A = 1.0 (one element), B = 2^-20, the fp32 result printed
//   hipcc --offload-arch=gfx950 -O2 -o probe_fp6_cvt probe_fp6_cvt.hip && ./probe_fp6_cvt > profiles/mxfp6_grad_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef uint32_t v6u __attribute__((ext_vector_type(6)));
typedef _Float16 v32h __attribute__((ext_vector_type(32)));
typedef __bf16 v32b __attribute__((ext_vector_type(32)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// one block per lane: in [lanes][6] dwords, scale [lanes], out [lanes][32] 16-bit patterns
template <int BF>
__global__ __launch_bounds__(64) void cvt_kernel(const uint32_t* in, const float* scale, uint16_t* out) {
    const int l = threadIdx.x;
    v6u w;
    for (int i = 0; i < 6; i++) w[i] = in[l * 6 + i];
    uint16_t h[32];
    if (BF) {
        const v32b v = __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(w, scale[l]);
        __builtin_memcpy(h, &v, 64);
    } else {
        const v32h v = __builtin_amdgcn_cvt_scalef32_pk32_f16_fp6(w, scale[l]);
        __builtin_memcpy(h, &v, 64);
    }
    for (int j = 0; j < 32; j++) out[l * 32 + j] = h[j];
}

// A[0][0] = 1.0 (lane 0, element 0), B[0][c] = bits (every lane < 32, element 0): D[0][c] = the product
__global__ __launch_bounds__(64) void mfma_kernel(uint16_t bits, float* out) {
    const int l = threadIdx.x;
    v8h a, b;
    for (int i = 0; i < 8; i++) a[i] = b[i] = (_Float16)0.0f;
    if (l == 0) a[0] = (_Float16)1.0f;
    if (l < 32) b[0] = __builtin_bit_cast(_Float16, bits);
    v16f c;
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    if (l == 0) out[0] = c[0];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static double e2m3(int c) {
    const int e = (c >> 3) & 3, m = c & 7;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 1) : m / 8.0;
    return (c & 0x20) ? -v : v;
}
static double f16_val(uint16_t h) {
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 31 ? (m ? NAN : INFINITY) : e ? ldexp(1.0 + m / 1024.0, e - 15) : ldexp(m / 1024.0, -14);
    return s ? -v : v;
}
static double bf16_val(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static void set_code(uint32_t* w, int j, int code) {
    const int bit = 6 * j;
    w[bit >> 5] |= (uint32_t)code << (bit & 31);
    if ((bit & 31) > 26) w[(bit >> 5) + 1] |= (uint32_t)code >> (32 - (bit & 31));
}

static uint32_t h_in[64 * 6];
static float h_sc[64];
static uint16_t h_out[64 * 32];
static uint32_t* d_in;
static float* d_sc;
static uint16_t* d_out;

static void run(int bf) {
    CK(hipMemcpy(d_in, h_in, sizeof(h_in), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_sc, h_sc, sizeof(h_sc), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, sizeof(h_out)));
    if (bf) hipLaunchKernelGGL(cvt_kernel<1>, dim3(1), dim3(64), 0, 0, d_in, d_sc, d_out);
    else hipLaunchKernelGGL(cvt_kernel<0>, dim3(1), dim3(64), 0, 0, d_in, d_sc, d_out);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost));
}

int main() {
    CK(hipMalloc(&d_in, sizeof(h_in)));
    CK(hipMalloc(&d_sc, sizeof(h_sc)));
    CK(hipMalloc(&d_out, sizeof(h_out)));
    int map[2][32];
    for (int bf = 0; bf < 2; bf++) {
        const char* name = bf ? "bf16" : "f16";
        double (*val)(uint16_t) = bf ? bf16_val : f16_val;
        // (a) position j holds the positive code j + 1 (0.125 .. 4.0, all distinct and nonzero)
        memset(h_in, 0, sizeof(h_in));
        for (int l = 0; l < 64; l++) {
            h_sc[l] = 1.0f;
            for (int j = 0; j < 32; j++) set_code(h_in + l * 6, j, j + 1);
        }
        run(bf);
        printf("(a) %s element map: output element i <- code position j\n   ", name);
        int natural = 1;
        for (int i = 0; i < 32; i++) {
            int found = -1;
            for (int j = 0; j < 32; j++)
                if (val(h_out[i]) == e2m3(j + 1)) found = j;
            map[bf][i] = found;
            natural &= found == i;
            printf(" %d<-%d", i, found);
        }
        printf("\n    %s\n", natural ? "natural order: element i is code position i" : "NOT the natural order");
        // all 64 codes at every position: lane l, position j holds code (l + j) % 64
        memset(h_in, 0, sizeof(h_in));
        for (int l = 0; l < 64; l++)
            for (int j = 0; j < 32; j++) set_code(h_in + l * 6, j, (l + j) & 63);
        run(bf);
        int bad = 0, signed_zero = 1;
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 32; i++) {
                const int j = map[bf][i];
                if (j < 0) { bad++; continue; }
                const int code = (l + j) & 63;
                const double v = val(h_out[l * 32 + i]);
                if (v != e2m3(code)) bad++;
                if (code == 32 && h_out[l * 32 + i] != 0x8000) signed_zero = 0;
            }
        printf("    all 64 codes at all 32 positions, scale 1.0: %d mismatches of 2048; code 0x20 -> %s\n", bad, signed_zero ? "-0" : "not -0");

        // (b) scales 2^d, d = 0 .. -11
        memset(h_in, 0, sizeof(h_in));
        for (int l = 0; l < 64; l++) {
            h_sc[l] = ldexpf(1.0f, -(l % 12));
            for (int j = 0; j < 32; j++) set_code(h_in + l * 6, j, (l + 2 * j + 1) & 63);
        }
        run(bf);
        bad = 0;
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 32; i++) {
                const int j = map[bf][i];
                if (j < 0 || val(h_out[l * 32 + i]) != ldexp(e2m3((l + 2 * j + 1) & 63), -(l % 12))) bad++;
            }
        printf("(b) %s scales 2^0 .. 2^-11 (one per lane): %d mismatches of 2048\n", name, bad);

        // (c) below the normal range
        const int d0 = bf ? 122 : 12, nd = bf ? 8 : 15;
        memset(h_in, 0, sizeof(h_in));
        for (int l = 0; l < 64; l++) {
            h_sc[l] = l < nd ? ldexpf(1.0f, -(d0 + l)) : 1.0f;
            set_code(h_in + l * 6, 0, 1);       // 0.125
            set_code(h_in + l * 6, 1, 15);      // 1.875
            set_code(h_in + l * 6, 2, 32 + 1);  // -0.125
        }
        run(bf);
        printf("(c) %s below the normal range: scale 2^-d; codes 0.125, 1.875, -0.125 -> bits (value) [exact value]\n", name);
        int i0 = 0, i1 = 1, i2 = 2;
        for (int i = 0; i < 32; i++) {
            if (map[bf][i] == 0) i0 = i;
            if (map[bf][i] == 1) i1 = i;
            if (map[bf][i] == 2) i2 = i;
        }
        for (int l = 0; l < nd; l++) {
            const uint16_t a = h_out[l * 32 + i0], b = h_out[l * 32 + i1], c = h_out[l * 32 + i2];
            printf("    d=%3d  0x%04x (%.6g) [%.6g]   0x%04x (%.6g) [%.6g]   0x%04x (%.6g)\n", d0 + l, a, val(a), ldexp(0.125, -(d0 + l)), b, val(b),
                   ldexp(1.875, -(d0 + l)), c, val(c));
        }
    }
    // (d) the fp16 MFMA on a subnormal B operand
    float* d_f;
    float h_f = -1.f;
    CK(hipMalloc(&d_f, 4));
    const uint16_t sub[3] = {0x0010 /* 2^-20 */, 0x0001 /* 2^-24 */, 0x03ff /* the largest subnormal */};
    for (int i = 0; i < 3; i++) {
        hipLaunchKernelGGL(mfma_kernel, dim3(1), dim3(64), 0, 0, sub[i], d_f);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(&h_f, d_f, 4, hipMemcpyDeviceToHost));
        printf("(d) v_mfma_f32_32x32x16_f16: 1.0 * fp16 bits 0x%04x (%.9g) = %.9g  %s\n", sub[i], f16_val(sub[i]), h_f,
               h_f == (float)f16_val(sub[i]) ? "kept" : "NOT kept");
    }
    return 0;
}
