// How v_mfma_scale_f32_32x32x64_f8f6f4 / v_mfma_scale_f32_16x16x128_f8f6f4 (FP4 x FP4, cbsz = blgp = 4) read their two scale operands on
// gfx950: which lane's scale byte applies to which (row, 32-value block), which byte of the scale VGPR the op_sel immediates pick, and what
// the instruction does with scale code 0, code 255 and scale sums beyond the fp32 exponent range.  Operands are one-hot / all-ones E2M1
// codes and every scale is a distinct power of two, so a wrong reading shows as a wrong exponent, not as noise.
//   hipcc --offload-arch=gfx950 -O2 -o probe_mx_scale probe_mx_scale.hip && ./probe_mx_scale > profiles/mxfp4_a4_scale_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct LaneIn { int a[4], b[4], sa, sb; };

template <int OA, int OB>
__global__ __launch_bounds__(64) void k32(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], 0, 0, 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], 0, 0, 0, 0};
    v16f c;
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, OA, v.sa, OB, v.sb);
    // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    for (int r = 0; r < 16; r++) out[((r & 3) + 8 * (r >> 2) + 4 * (threadIdx.x >> 5)) * 32 + (threadIdx.x & 31)] = c[r];
}
template <int OA, int OB>
__global__ __launch_bounds__(64) void k16(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], 0, 0, 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], 0, 0, 0, 0};
    v4f c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 4, OA, v.sa, OB, v.sb);
    // C/D: column = lane & 15, row = 4 (lane >> 4) + r
    for (int r = 0; r < 4; r++) out[(4 * (threadIdx.x >> 4) + r) * 16 + (threadIdx.x & 15)] = c[r];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static LaneIn* d_in;
static float* d_out;
static float h_out[1024];

template <int S, int OA, int OB>
static void run(const LaneIn* h) {
    CK(hipMemcpy(d_in, h, 64 * sizeof(LaneIn), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, sizeof(h_out)));
    if (S == 32) hipLaunchKernelGGL((k32<OA, OB>), dim3(1), dim3(64), 0, 0, d_in, d_out);
    else hipLaunchKernelGGL((k16<OA, OB>), dim3(1), dim3(64), 0, 0, d_in, d_out);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost));
}

// Operands for "only k-block kb contributes, every product is 1.0": A = 1.0 (code 2) over the whole block kb, B = 1.0 at the block's first
// value only.  Lane l is taken to hold row / column l % S and k-block l / S (the data map the FP4 kernels of this tree already rely on).
static void fill_block(LaneIn* h, int S, int kb) {
    memset(h, 0, 64 * sizeof(LaneIn));
    for (int l = 0; l < 64; l++) {
        if (l / S != kb) continue;
        for (int i = 0; i < 4; i++) h[l].a[i] = 0x22222222;
        h[l].b[0] = 0x2;
    }
}
static int all4(int c) { return c | c << 8 | c << 16 | c << 24; }
static int expo(float v) { return (v > 0.f && isfinite(v)) ? (int)lrintf(log2f(v)) : -9999; }

template <int S>
static int lane_map() {
    const int KB = 64 / S;
    int bad = 0;
    LaneIn h[64];
    for (int which = 0; which < 2; which++) {  // 0: scale A carries the lane tag, 1: scale B
        printf("%dx%dx%d, scale %c = 2^(lane - 32) in all four bytes, the other scale 2^0: the lane whose byte scaled (row|col, k-block)\n", S, S, 2048 / S,
               which ? 'B' : 'A');
        for (int kb = 0; kb < KB; kb++) {
            fill_block(h, S, kb);
            for (int l = 0; l < 64; l++) {
                h[l].sa = all4(which == 0 ? 95 + l : 127);
                h[l].sb = all4(which == 1 ? 95 + l : 127);
            }
            run<S, 0, 0>(h);
            printf("  k-block %d:", kb);
            for (int i = 0; i < S; i++) {
                int lane = -1, uniform = 1;
                for (int j = 0; j < S; j++) {
                    const float v = which == 0 ? h_out[i * S + j] : h_out[j * S + i];  // A tags rows of D, B tags columns
                    const int l = expo(v) + 32;
                    if (j == 0) lane = l;
                    else if (l != lane) uniform = 0;
                }
                printf(" %d%s", lane, uniform ? "" : "?");
                if (!uniform || lane != i + S * kb) bad++;
            }
            printf("\n");
        }
    }
    printf("%dx%d lane map: %s (expected lane = (row|col) + %d * k-block)\n\n", S, S, bad ? "DIFFERS" : "as expected", S);
    return bad;
}

template <int S, int OA, int OB>
static int byte_sel_one() {
    LaneIn h[64];
    fill_block(h, S, 0);
    for (int l = 0; l < 64; l++) {
        h[l].sa = 100 | 110 << 8 | 120 << 16 | 130 << 24;
        h[l].sb = 124 | 125 << 8 | 126 << 16 | 127 << 24;
    }
    run<S, OA, OB>(h);
    const int e = expo(h_out[0]);  // = (byte A - 127) + (byte B - 127) = 10 a + b - 30: one (a, b) per exponent
    int fa = -1, fb = -1;
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++)
            if ((100 + 10 * a - 127) + (124 + b - 127) == e) { fa = a; fb = b; }
    printf("  %dx%d builtin byte selects (A %d, B %d): D = 2^%d -> the instruction read byte %d of scale A, byte %d of scale B%s\n", S, S, OA, OB, e, fa, fb,
           (fa == OA && fb == OB) ? "" : "   DIFFERS");
    return !(fa == OA && fb == OB);
}

template <int S>
static void edge(const char* what, int sa, int sb) {
    LaneIn h[64];
    fill_block(h, S, 0);
    for (int l = 0; l < 64; l++) { h[l].sa = all4(sa); h[l].sb = all4(sb); }
    run<S, 0, 0>(h);
    unsigned bits;
    memcpy(&bits, &h_out[0], 4);
    printf("  %dx%d %-58s scale A %3d, scale B %3d: D = %-13g (0x%08x)\n", S, S, what, sa, sb, h_out[0], bits);
}

template <int S>
static void edge_zero_operand(int sa, int sb) {  // a block whose codes are all zero under a NaN / huge scale
    LaneIn h[64];
    memset(h, 0, sizeof(h));
    for (int l = 0; l < 64; l++) { h[l].sa = all4(sa); h[l].sb = all4(sb); }
    run<S, 0, 0>(h);
    unsigned bits;
    memcpy(&bits, &h_out[0], 4);
    printf("  %dx%d all codes zero,                                             scale A %3d, scale B %3d: D = %-13g (0x%08x)\n", S, S, sa, sb, h_out[0], bits);
}

template <int S>
static void edges() {
    edge<S>("product 1.0, both scales 2^0", 127, 127);
    edge<S>("scale code 0 (2^-127) against 2^0", 0, 127);
    edge<S>("scale code 0 against 2^127 (sum in range)", 0, 254);
    edge<S>("scale code 0 against code 0 (2^-254)", 0, 0);
    edge<S>("2^-100 against 2^-50 (2^-150, below the fp32 subnormals)", 27, 77);
    edge<S>("2^-100 against 2^-40 (2^-140, an fp32 subnormal)", 27, 87);
    edge<S>("2^127 against 2^127 (2^254)", 254, 254);
    edge<S>("2^100 against 2^27 (2^127)", 227, 154);
    edge<S>("2^100 against 2^28 (2^128)", 227, 155);
    edge<S>("scale code 255 on A", 255, 127);
    edge<S>("scale code 255 on B", 127, 255);
    edge_zero_operand<S>(255, 127);
    edge_zero_operand<S>(254, 254);
}

int main() {
    CK(hipMalloc(&d_in, 64 * sizeof(LaneIn)));
    CK(hipMalloc(&d_out, sizeof(h_out)));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("device: %s\n\n", p.gcnArchName);
    int bad = 0;
    bad += lane_map<32>();
    bad += lane_map<16>();
    printf("byte of the scale VGPR picked by the builtin's two byte-select arguments (scale A bytes 100 110 120 130, scale B bytes 124 125 126 127)\n");
    bad += byte_sel_one<32, 0, 0>();
    bad += byte_sel_one<32, 1, 3>();
    bad += byte_sel_one<32, 2, 1>();
    bad += byte_sel_one<32, 3, 2>();
    bad += byte_sel_one<16, 0, 0>();
    bad += byte_sel_one<16, 1, 3>();
    bad += byte_sel_one<16, 2, 1>();
    bad += byte_sel_one<16, 3, 2>();
    printf("\nedge cases (one product of 1.0 per output unless stated)\n");
    edges<32>();
    edges<16>();
    printf("\nsummary: %s\n", bad ? "the scale operands are NOT read as assumed" : "lane map and byte selects as assumed");
    return bad ? 1 : 0;
}
