// How v_mfma_scale_f32_32x32x64_f8f6f4 / v_mfma_scale_f32_16x16x128_f8f6f4 read an FP4 x FP6 pair of operands on gfx950: A = FP4 E2M1
// (cbsz 4, four VGPRs), B = FP6 E2M3 (blgp 2, six VGPRs).  profiles/mxfp4_a8_probe.txt pinned FP4 x E4M3 (where the B operand is split in
// two halves) and profiles/mxfp6_a6_probe.txt FP6 x FP6 (where it is not); this pair was pinned by neither.  For both shapes:
//   (a1) which element of the instruction's K each of the 32 six-bit fields of a lane's six B registers is.  k has a meaning only
//        through the pairing with A, so nothing is assumed about B: for every B position (lane group g, field j at bits 6 j .. 6 j + 5) the
//        B operand is one-hot there (2^(col % 4 - 1), every column); A holds codes distinct per (row, field) in ONE register of ONE lane
//        group at a time (8 four-bit fields: FP4 has only 14 distinct non-zero values) and zeros elsewhere, and the (A lane group, A
//        field) whose value came out is printed as k = 32 * group + field.  A position of B that no A position meets, or that several
//        meet, is printed as -1
//   (a2) the same for A: every A position (lane group g, field j at bits 4 j .. 4 j + 3) one-hot (2^(row % 4 - 1), every row), B codes
//        distinct per (column, field) in one lane group at a time; the B position 32 * group + field whose value came out
//   (b)  which lane's scale byte applies to which (row | column, block k = 32 b .. 32 b + 31) on either operand: every scale a distinct
//        power of two
//   (c)  the accumulation error of ONE instruction against float64, in fp32 ulps of sum |products|: on random codes under one scale (every
//        exact sum is then an fp32 value: E2M1 x E2M3 products lie on a 2^-4 grid with |p| <= 45), and on random codes under random block
//        scales, where the blocks of one instruction differ in scale and the exact sums need more than 24 bits
//   hipcc --offload-arch=gfx950 -O2 -o probe_mx_fp4x6 probe_mx_fp4x6.hip && ./probe_mx_fp4x6 > profiles/mxfp4_a6_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct LaneIn { int a[4], b[6], sa, sb; };

__global__ __launch_bounds__(64) void k32(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], 0, 0, 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], 0, 0};
    v16f c;
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 2, 0, v.sa, 0, v.sb);
    // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    for (int r = 0; r < 16; r++) out[((r & 3) + 8 * (r >> 2) + 4 * (threadIdx.x >> 5)) * 32 + (threadIdx.x & 31)] = c[r];
}
__global__ __launch_bounds__(64) void k16(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], 0, 0, 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], 0, 0};
    v4f c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 2, 0, v.sa, 0, v.sb);
    // C/D: column = lane & 15, row = 4 (lane >> 4) + r
    for (int r = 0; r < 4; r++) out[(4 * (threadIdx.x >> 4) + r) * 16 + (threadIdx.x & 15)] = c[r];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static LaneIn* d_in;
static float* d_out;
static float h_out[1024];

template <int S>
static void run(const LaneIn* h) {
    CK(hipMemcpy(d_in, h, 64 * sizeof(LaneIn), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, sizeof(h_out)));
    if (S == 32) hipLaunchKernelGGL(k32, dim3(1), dim3(64), 0, 0, d_in, d_out);
    else hipLaunchKernelGGL(k16, dim3(1), dim3(64), 0, 0, d_in, d_out);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost));
}

static double e2m3(int c) {  // bit 5 sign, bits 4:3 exponent (bias 1), bits 2:0 mantissa; no Inf / NaN code
    const int e = (c >> 3) & 3, m = c & 7;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 1) : m / 8.0;
    return (c & 0x20) ? -v : v;
}
static double e2m1(int c) {  // bit 3 sign, bits 2:1 exponent (bias 1), bit 0 mantissa
    static const double t[8] = {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0};
    return (c & 8) ? -t[c & 7] : t[c & 7];
}
static int all4(int c) { return c | c << 8 | c << 16 | c << 24; }
static int expo(float v) { return (v > 0.f && isfinite(v)) ? (int)lrintf(log2f(v)) : -9999; }

// a six-bit code into field j of lane l's 192 B operand bits, a four-bit code into field j of its 128 A operand bits, little-endian
static void set_field6(int* regs, int j, int code) {
    const int bit = 6 * j;
    uint32_t* a = reinterpret_cast<uint32_t*>(regs);
    a[bit >> 5] |= (uint32_t)code << (bit & 31);
    if ((bit & 31) > 26) a[(bit >> 5) + 1] |= (uint32_t)code >> (32 - (bit & 31));
}
static void set_field4(int* regs, int j, int code) { reinterpret_cast<uint32_t*>(regs)[j >> 3] |= (uint32_t)code << (4 * (j & 7)); }
// A by its position k = 32 * lane group + field (row = lane % S); B by position p = 32 * lane group + field, and by k through the map
// that part (a1) found
static void set_a(LaneIn* h, int S, int row, int k, int code) { set_field4(h[row + S * (k >> 5)].a, k & 31, code); }
static void set_b_pos(LaneIn* h, int S, int col, int p, int code) { set_field6(h[col + S * (p >> 5)].b, p & 31, code); }
static int pmap32[64], pmap16[128];  // k -> B position
static void set_b(LaneIn* h, int S, int col, int k, int code) { set_b_pos(h, S, col, S == 32 ? pmap32[k] : pmap16[k], code); }

// FP4 codes with 14 distinct non-zero values; distinct over the 8 fields j of one register of one row
static int acode(int row, int j) { static const int c[14] = {1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15}; return c[(j + row * 3) % 14]; }
static int bhot(int col) { static const int c[4] = {0x04, 0x08, 0x10, 0x18}; return c[col & 3]; }  // E2M3 0.5, 1, 2, 4
static int bcode(int col, int j) { return (j * 5 + col * 11) % 63 + 1; }                             // 1 .. 63, distinct over the j of one column
static int ahot(int row) { static const int c[4] = {1, 2, 4, 6}; return c[row & 3]; }              // E2M1 0.5, 1, 2, 4

template <int S>
static int field_map_b() {
    const int K = 2048 / S, KB = K / 32;
    int* pmap = S == 32 ? pmap32 : pmap16;
    int bad = 0;
    static LaneIn h[64];
    for (int k = 0; k < K; k++) pmap[k] = -1;
    printf("(a1) %dx%dx%d: B one-hot 2^(col %% 4 - 1) at field j (bits 6 j .. 6 j + 5) of lane group g, A codes distinct per field in one register (8 fields j', bits 4 j' .. 4 j' + 3) of one lane group g' at a time: k = 32 g' + j' whose value came out, per B field\n",
           S, S, K);
    for (int p = 0; p < K; p++) {
        int found = -2;  // the k every output agrees on over all A sub-groups; -1 where outputs disagree, match none, or two sub-groups answer
        for (int ga = 0; ga < KB * 4; ga++) {  // A sub-group: fields 8 ga .. 8 ga + 7 of the instruction's K by A position
            memset(h, 0, sizeof(h));
            for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
            for (int i = 0; i < S; i++)
                for (int j = 0; j < 8; j++) set_a(h, S, i, 8 * ga + j, acode(i, j));
            for (int c = 0; c < S; c++) set_b_pos(h, S, c, p, bhot(c));
            run<S>(h);
            int zero = 1, here = -2;
            for (int i = 0; i < S * S; i++)
                if (h_out[i] != 0.0f) zero = 0;
            if (zero) continue;
            for (int i = 0; i < S; i++)
                for (int c = 0; c < S; c++) {
                    int f = -1;
                    for (int jj = 0; jj < 8; jj++)
                        if ((double)h_out[i * S + c] == e2m1(acode(i, jj)) * e2m3(bhot(c))) f = jj;
                    if (here == -2) here = f;
                    else if (f != here) here = -1;
                }
            found = (found == -2 && here >= 0) ? 8 * ga + here : -1;
        }
        if (found == -2) found = -1;
        if (p % 32 == 0) printf("  lane group %d:", p / 32);
        printf(" %d", found);
        if (p % 32 == 31) printf("\n");
        if (found != p) bad++;
        if (found >= 0 && pmap[found] < 0) pmap[found] = p;
    }
    for (int k = 0; k < K; k++)
        if (pmap[k] < 0) {
            pmap[k] = k;
            bad++;
        }
    printf("%dx%d B field map and C/D map: %s (expected k = 32 g + j: lane group g of B holds k = 32 g .. 32 g + 31, element j at bits 6 j .. 6 j + 5, one block per lane as the FP4 A operand)\n\n",
           S, S, bad ? "DIFFERS" : "as expected");
    return bad;
}

template <int S>
static int field_map_a() {
    const int K = 2048 / S, KB = K / 32;
    int bad = 0;
    static LaneIn h[64];
    printf("(a2) %dx%dx%d: A one-hot 2^(row %% 4 - 1) at field j (bits 4 j .. 4 j + 3) of lane group g, B code (5 j' + 11 col) %% 63 + 1 at field j' of one lane group g' at a time: B position 32 g' + j' whose value came out, per A field\n",
           S, S, K);
    for (int p = 0; p < K; p++) {
        int found = -2;
        for (int gb = 0; gb < KB; gb++) {
            memset(h, 0, sizeof(h));
            for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
            for (int c = 0; c < S; c++)
                for (int j = 0; j < 32; j++) set_b_pos(h, S, c, 32 * gb + j, bcode(c, j));
            for (int i = 0; i < S; i++) set_a(h, S, i, p, ahot(i));
            run<S>(h);
            int zero = 1, here = -2;
            for (int i = 0; i < S * S; i++)
                if (h_out[i] != 0.0f) zero = 0;
            if (zero) continue;
            for (int i = 0; i < S; i++)
                for (int c = 0; c < S; c++) {
                    int f = -1;
                    for (int jj = 0; jj < 32; jj++)
                        if ((double)h_out[i * S + c] == e2m1(ahot(i)) * e2m3(bcode(c, jj))) f = jj;
                    if (here == -2) here = f;
                    else if (f != here) here = -1;
                }
            found = (found == -2 && here >= 0) ? 32 * gb + here : -1;
        }
        if (found == -2) found = -1;
        if (p % 32 == 0) printf("  lane group %d:", p / 32);
        printf(" %d", found);
        if (p % 32 == 31) printf("\n");
        if (found != p) bad++;
    }
    printf("%dx%d A field map: %s (expected B position = A position: lane group g of A holds k = 32 g .. 32 g + 31, element j at bits 4 j .. 4 j + 3, as in the W4A4 / W4A8 kernels)\n\n",
           S, S, bad ? "DIFFERS" : "as expected");
    return bad;
}

template <int S>
static int scale_map() {
    const int KB = 64 / S;
    int bad = 0;
    static LaneIn h[64];
    for (int which = 0; which < 2; which++) {  // 0: scale A carries the lane tag, 1: scale B
        printf("(b) %dx%dx%d, scale %c = 2^(lane - 32) in all four bytes, the other scale 2^0: the lane whose byte scaled (row|col, k-block)\n", S, S, 2048 / S,
               which ? 'B' : 'A');
        for (int kb = 0; kb < KB; kb++) {
            memset(h, 0, sizeof(h));
            for (int l = 0; l < 64; l++) {
                h[l].sa = all4(which == 0 ? 95 + l : 127);
                h[l].sb = all4(which == 1 ? 95 + l : 127);
            }
            for (int i = 0; i < S; i++)
                for (int k = 32 * kb; k < 32 * kb + 32; k++) set_a(h, S, i, k, 0x2);  // 1.0 over the whole block
            for (int j = 0; j < S; j++) set_b(h, S, j, 32 * kb, 0x08);                 // 1.0 at the block's first value only
            run<S>(h);
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
    printf("%dx%d scale map: %s (expected lane = (row|col) + %d * k-block)\n\n", S, S, bad ? "DIFFERS" : "as expected", S);
    return bad;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// mode 0: every code random; mode 1: large positive magnitudes (4 .. 6 on A, 6 .. 7.5 on B) with a few tiny values; both under scale 2^0
// on every block, where every exact sum is an fp32 value (products are multiples of 2^-4 with |p| <= 45, so 128 of them need 17 bits).
// mode 2: every code random and every block's scale random in 2^-8 .. 2^8 on either operand, so that blocks of different scales meet
// inside the instruction and the exact sum (still exact in float64: multiples of 2^-20 below 2^29) needs more than 24 bits
template <int S>
static double accumulate(int mode, int trials, long* inexact, long* total) {
    const int K = 2048 / S;
    static LaneIn h[64];
    static int A[32][128], B[32][128], SA[32][4], SB[32][4];
    double worst = 0.0;
    for (int t = 0; t < trials; t++) {
        memset(h, 0, sizeof(h));
        for (int i = 0; i < S; i++)
            for (int kb = 0; kb < K / 32; kb++) {  // the scale byte of lane group kb applies to block kb on either operand: part (b)
                SA[i][kb] = mode == 2 ? 119 + (int)(rnd() % 17) : 127;
                SB[i][kb] = mode == 2 ? 119 + (int)(rnd() % 17) : 127;
                h[i + S * kb].sa = all4(SA[i][kb]);
                h[i + S * kb].sb = all4(SB[i][kb]);
            }
        for (int i = 0; i < S; i++)
            for (int k = 0; k < K; k++) {
                int a, b;
                if (mode != 1) {
                    a = rnd() & 15;
                    b = rnd() & 63;
                } else {
                    a = 6 + (rnd() & 1);
                    b = (rnd() & 7) == 0 ? 1 + (rnd() & 7) : 0x1c + (rnd() & 3);
                }
                A[i][k] = a;
                B[i][k] = b;
                set_a(h, S, i, k, a);
                set_b(h, S, i, k, b);
            }
        run<S>(h);
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                double sum = 0.0, asum = 0.0;  // exact in float64
                for (int k = 0; k < K; k++) {
                    const double p = ldexp(e2m1(A[i][k]) * e2m3(B[j][k]), SA[i][k >> 5] + SB[j][k >> 5] - 254);
                    sum += p;
                    asum += fabs(p);
                }
                (*total)++;
                if ((double)(float)sum != sum) (*inexact)++;
                if (asum == 0.0) continue;
                const double ulp = ldexp(1.0, (int)floor(log2(asum)) - 23);
                const double err = fabs((double)h_out[i * S + j] - sum) / ulp;
                if (err > worst) worst = err;
            }
    }
    return worst;
}

template <int S>
static double accumulation() {
    double w = 0.0;
    for (int mode = 0; mode < 3; mode++) {
        long inexact = 0, total = 0;
        const double e = accumulate<S>(mode, 64, &inexact, &total);
        printf("(c) %dx%dx%d %s: %ld of %ld exact sums are not fp32 values; largest |D - exact| = %.4f fp32 ulps of sum |products|\n", S, S, 2048 / S,
               mode == 2 ? "random codes, random block scales 2^-8 .. 2^8" : mode ? "large positive products with a few tiny ones, scales 2^0" : "random codes, scales 2^0",
               inexact, total, e);
        if (e > w) w = e;
    }
    return w;
}

int main() {
    CK(hipMalloc(&d_in, 64 * sizeof(LaneIn)));
    CK(hipMalloc(&d_out, sizeof(h_out)));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("device: %s\nA = FP4 E2M1 (cbsz 4), B = FP6 E2M3 (blgp 2), byte selects 0\n\n", p.gcnArchName);
    int bad = 0;
    bad += field_map_b<32>();
    bad += field_map_b<16>();
    bad += field_map_a<32>();
    bad += field_map_a<16>();
    bad += scale_map<32>();
    bad += scale_map<16>();
    const double w32 = accumulation<32>(), w16 = accumulation<16>();
    printf("\nsummary: %s; worst accumulation error of one instruction %.4f fp32 ulps of sum |products| (32x32x64: %.4f over 64 products, 16x16x128: %.4f over 128)\n",
           bad ? "the operands are NOT read as assumed" : "field order, lane map and scale map as assumed", w32 > w16 ? w32 : w16, w32, w16);
    return bad ? 1 : 0;
}
