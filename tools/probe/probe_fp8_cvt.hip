// What v_cvt_scalef32_pk_{f16,bf16}_fp8 does on gfx950, for the MXFP8 weight-only kernels (csrc/mxfp8.hip, csrc/mxfp8_common.cuh): one
// dword of four E4M3 (e4m3fn) codes and an fp32 scale -> two 16-bit values, op_sel picking the half of the dword.
//   (a) the byte map: a dword of four distinct codes; for op_sel 0 and 1 the byte whose value came out in each half of the result
//   (b) all 256 codes at scale 1.0 in every byte position, compared with e4m3(code) exactly (NaN codes aside: part (d))
//   (c) fp16 below 2^-14 and at the maximum: codes 2^-9 (0x01), 1.875 * 2^-6 (0x0f), -2^-9 and 448 (0x7e) under 2^d, d = 0 .. -18 and
//       d = +6 .. +9; what comes out beside the exact value.  bf16 at d = -116 .. -126
//   (d) the NaN codes 0x7f and 0xff at scale 1.0 and 2^-3
//   hipcc --offload-arch=gfx950 -O2 -o probe_fp8_cvt probe_fp8_cvt.hip && ./probe_fp8_cvt > profiles/mxfp8_cvt_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef __bf16 v2b __attribute__((ext_vector_type(2)));

// one dword per lane: out [lanes][2 op_sel][2 halves] 16-bit patterns
template <int BF>
__global__ __launch_bounds__(64) void cvt_kernel(const uint32_t* in, const float* scale, uint16_t* out) {
    const int l = threadIdx.x;
    const uint32_t w = in[l];
    const float s = scale[l];
    uint32_t r0, r1;
    if (BF) {
        r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, false));
        r1 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, true));
    } else {
        r0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, false));
        r1 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, true));
    }
    out[l * 4 + 0] = (uint16_t)r0;
    out[l * 4 + 1] = (uint16_t)(r0 >> 16);
    out[l * 4 + 2] = (uint16_t)r1;
    out[l * 4 + 3] = (uint16_t)(r1 >> 16);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static double e4m3(int c) {  // e4m3fn: bias 7, no inf, 0x7f / 0xff NaN
    const int e = (c >> 3) & 15, m = c & 7;
    if (e == 15 && m == 7) return NAN;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return (c & 0x80) ? -v : v;
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

static uint32_t h_in[64];
static float h_sc[64];
static uint16_t h_out[64 * 4];
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
    for (int bf = 0; bf < 2; bf++) {
        const char* name = bf ? "bf16" : "f16";
        double (*val)(uint16_t) = bf ? bf16_val : f16_val;
        // (a) byte j holds the code 0x38 + 8 j: 1, 2, 4, 8
        int map[4];
        for (int l = 0; l < 64; l++) {
            h_sc[l] = 1.0f;
            h_in[l] = 0x38u | (0x40u << 8) | (0x48u << 16) | (0x50u << 24);
        }
        run(bf);
        printf("(a) %s byte map: result (op_sel, half) <- byte of the source dword\n   ", name);
        int natural = 1;
        for (int i = 0; i < 4; i++) {
            map[i] = -1;
            for (int j = 0; j < 4; j++)
                if (val(h_out[i]) == ldexp(1.0, j)) map[i] = j;
            natural &= map[i] == i;
            printf(" (%d, %d)<-%d", i >> 1, i & 1, map[i]);
        }
        printf("\n    %s\n", natural ? "natural order: op_sel s, half h is byte 2 s + h" : "NOT the natural order");
        // (b) all 256 codes in every byte: in pass rot, byte j of lane l holds code 4 l + (j + rot) % 4
        int bad = 0, nans = 0, neg_zero = 1;
        for (int rot = 0; rot < 4; rot++) {
            for (int l = 0; l < 64; l++) {
                h_in[l] = 0;
                for (int j = 0; j < 4; j++) h_in[l] |= (uint32_t)(4 * l + ((j + rot) & 3)) << (8 * j);
            }
            run(bf);
            for (int l = 0; l < 64; l++)
                for (int i = 0; i < 4; i++) {
                    if (map[i] < 0) { bad++; continue; }
                    const int code = 4 * l + ((map[i] + rot) & 3);
                    const double want = e4m3(code), got = val(h_out[l * 4 + i]);
                    if (isnan(want)) { nans++; continue; }
                    if (got != want) bad++;
                    if (code == 0x80 && h_out[l * 4 + i] != 0x8000) neg_zero = 0;
                }
        }
        printf("(b) %s all 256 codes at all 4 byte positions, scale 1.0: %d mismatches of %d (NaN codes aside); code 0x80 -> %s\n", name, bad,
               4 * 256 - nans, neg_zero ? "-0" : "not -0");
        // (c) the ends of the range
        const int nd = bf ? 11 : 23;
        int ds[23];
        for (int i = 0; i < nd; i++) ds[i] = bf ? -(116 + i) : (i < 19 ? -i : i - 19 + 6);
        for (int l = 0; l < 64; l++) {
            h_sc[l] = l < nd ? ldexpf(1.0f, ds[l]) : 1.0f;
            h_in[l] = 0x01u | (0x0fu << 8) | (0x81u << 16) | (0x7eu << 24);
        }
        run(bf);
        printf("(c) %s range ends: scale 2^d; codes 2^-9, 1.875 * 2^-6, -2^-9, 448 -> bits (value) [exact value]\n", name);
        int at[4] = {0, 1, 2, 3};
        for (int i = 0; i < 4; i++)
            if (map[i] >= 0) at[map[i]] = i;
        for (int l = 0; l < nd; l++) {
            printf("    d=%4d", ds[l]);
            const int codes[4] = {0x01, 0x0f, 0x81, 0x7e};
            for (int j = 0; j < 4; j++) {
                const uint16_t b = h_out[l * 4 + at[j]];
                printf("   0x%04x (%.6g) [%.6g]", b, val(b), ldexp(e4m3(codes[j]), ds[l]));
            }
            printf("\n");
        }
        // (d) NaN codes
        for (int l = 0; l < 64; l++) {
            h_sc[l] = (l & 1) ? 0.125f : 1.0f;
            h_in[l] = 0x7fu | (0xffu << 8) | (0x38u << 16) | (0x40u << 24);
        }
        run(bf);
        printf("(d) %s NaN codes: bytes 0x7f, 0xff, 0x38 (1.0), 0x40 (2.0)\n", name);
        for (int l = 0; l < 2; l++) {
            printf("    scale %g:", h_sc[l]);
            for (int j = 0; j < 4; j++) printf("  0x%04x (%g)", h_out[l * 4 + at[j]], val(h_out[l * 4 + at[j]]));
            printf("\n");
        }
    }
    return 0;
}
