// How v_mfma_scale_f32_32x32x64_f8f6f4 / v_mfma_scale_f32_16x16x128_f8f6f4 read an FP6 x E4M3 pair of operands on gfx950: A = FP6 E2M3
// (cbsz 2, six VGPRs), B = OCP E4M3 (blgp 0, eight VGPRs).  profiles/mxfp4_a8_probe.txt pinned FP4 x E4M3 only.  For both shapes:
//   (a1) which byte of which lane group of the 32-byte B operand is element k of the instruction's K: one-hot FP6 weights (code 0x08 = 1.0
//        at bits 6 j + 3 of group g's 192 bits, every row) over E4M3 values that are distinct per (column, lane group, byte), compared
//        exactly.  Nothing is assumed about B: the position whose value came out is printed and then used by the other parts
//   (a2) the bit order of the FP6 operand and the C/D map: FP6 codes distinct per (row, j), code at bits 6 j .. 6 j + 5 little-endian, over
//        one-hot E4M3 values 2^(column % 4) at k
//   (b)  which lane's scale byte applies to which (row | column, block k = 32 b .. 32 b + 31) on either operand: every scale a distinct
//        power of two
//   (c)  the accumulation error of ONE instruction on random codes and on blocks whose exact sums need more than 24 bits, against float64,
//        in fp32 ulps of sum |products|
//   hipcc --offload-arch=gfx950 -O2 -o probe_mx_fp6 probe_mx_fp6.hip && ./probe_mx_fp6 > profiles/mxfp6_a8_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct LaneIn { int a[6], b[8], sa, sb; };

__global__ __launch_bounds__(64) void k32(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], v.a[4], v.a[5], 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], v.b[6], v.b[7]};
    v16f c;
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 2, 0, 0, v.sa, 0, v.sb);
    // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    for (int r = 0; r < 16; r++) out[((r & 3) + 8 * (r >> 2) + 4 * (threadIdx.x >> 5)) * 32 + (threadIdx.x & 31)] = c[r];
}
__global__ __launch_bounds__(64) void k16(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], v.a[4], v.a[5], 0, 0}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], v.b[6], v.b[7]};
    v4f c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 2, 0, 0, v.sa, 0, v.sb);
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
static double e4m3(int c) {  // OCP e4m3fn; 0x7f / 0xff (NaN) are never used here
    const int e = (c >> 3) & 15, m = c & 7;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return (c & 0x80) ? -v : v;
}
static int all4(int c) { return c | c << 8 | c << 16 | c << 24; }
static int expo(float v) { return (v > 0.f && isfinite(v)) ? (int)lrintf(log2f(v)) : -9999; }

// A (FP6), the layout under test: lane l holds row l % S and the elements k = 32 g .. 32 g + 31 of group g = l / S, element k in bits
// 6 (k % 32) .. + 5 of the lane's 192 bits, little-endian over its six registers.
static void set_a(LaneIn* h, int S, int row, int k, int code) {
    const int bit = 6 * (k & 31);
    uint32_t* a = reinterpret_cast<uint32_t*>(h[row + S * (k >> 5)].a);
    a[bit >> 5] |= (uint32_t)code << (bit & 31);
    if ((bit & 31) > 26) a[(bit >> 5) + 1] |= (uint32_t)code >> (32 - (bit & 31));
}
// B (E4M3) by position p = 32 * lane group + byte of the group's 32-byte operand, and by k through the map that part (a1) found
static void set_b_pos(LaneIn* h, int S, int col, int p, int code) { h[col + S * (p >> 5)].b[(p & 31) >> 2] |= code << (8 * (p & 3)); }
static int kmap32[64], kmap16[128];
static void set_b(LaneIn* h, int S, int col, int k, int code) { set_b_pos(h, S, col, S == 32 ? kmap32[k] : kmap16[k], code); }
// distinct over the positions of one column (the second lap of the 0x70 codes is negative), no NaN code
static int xcode(int col, int p) { return (0x08 + (p * 5 + col * 3) % 0x70) | (p >= 0x70 ? 0x80 : 0); }

// the two candidate maps: the E4M3 operand as with an FP4 partner (two 16-byte halves, a8_frag), or one contiguous block per lane group
static int pos_split(int S, int k) { const int HS = 16 * (64 / S); return 32 * ((k % HS) >> 4) + 16 * (k / HS) + (k & 15); }
static int pos_block(int, int k) { return k; }

template <int S>
static int byte_map() {
    const int K = 2048 / S;
    int* kmap = S == 32 ? kmap32 : kmap16;
    int bad = 0, split = 1, block = 1;
    static LaneIn h[64];
    printf("(a1) %dx%dx%d: FP6 weights one-hot (1.0 at k, every row), x[col][p] = e4m3(0x08 + (5 p + 3 col) %% 0x70) at position p = 32 * lane group + byte: the p whose value came out, per k\n", S, S, K);
    for (int k = 0; k < K; k++) {
        memset(h, 0, sizeof(h));
        for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
        for (int i = 0; i < S; i++) set_a(h, S, i, k, 0x08);
        for (int j = 0; j < S; j++)
            for (int p = 0; p < K; p++) set_b_pos(h, S, j, p, xcode(j, p));
        run<S>(h);
        int found = -2;  // the p every output agrees on, -1 where they disagree or match none
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                int f = -1;
                for (int p = 0; p < K; p++)
                    if ((double)h_out[i * S + j] == e4m3(xcode(j, p))) f = p;
                if (found == -2) found = f;
                else if (f != found) found = -1;
            }
        if (k % 32 == 0) printf("  k-block %d:", k / 32);
        printf(" %d", found);
        if (k % 32 == 31) printf("\n");
        kmap[k] = found < 0 ? 0 : found;
        if (found < 0) bad++;
        if (found != pos_split(S, k)) split = 0;
        if (found != pos_block(S, k)) block = 0;
    }
    if (!split && !block) bad++;
    printf("%dx%d B byte map: %s\n\n", S, S,
           bad ? "NEITHER candidate" : split ? "SPLIT HALVES as with an FP4 partner (group g: k = 16 g .. + 15 in bytes 0 .. 15, k = 16 G + 16 g .. + 15 in bytes 16 .. 31)"
                                             : "ONE BLOCK per lane group (group g: k = 32 g + byte)");
    return bad;
}

static int acode(int row, int j) { return (j * 5 + row * 11) % 63 + 1; }  // 1 .. 63, distinct over the j of one row

template <int S>
static int bit_order() {
    const int K = 2048 / S;
    int bad = 0;
    static LaneIn h[64];
    printf("(a2) %dx%dx%d: FP6 code (5 j + 11 row) %% 63 + 1 at bits 6 j .. 6 j + 5 of every lane group, x one-hot 2^(col %% 4) at k: the j whose value came out, per k\n", S, S, K);
    for (int k = 0; k < K; k++) {
        memset(h, 0, sizeof(h));
        for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
        for (int i = 0; i < S; i++)
            for (int kk = 0; kk < K; kk++) set_a(h, S, i, kk, acode(i, kk & 31));
        for (int j = 0; j < S; j++) set_b(h, S, j, k, 0x38 + 8 * (j & 3));
        run<S>(h);
        int found = -2;
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                int f = -1;
                for (int jj = 0; jj < 32; jj++)
                    if ((double)h_out[i * S + j] == e2m3(acode(i, jj)) * (1 << (j & 3))) f = jj;
                if (found == -2) found = f;
                else if (f != found) found = -1;
            }
        if (k % 32 == 0) printf("  k-block %d:", k / 32);
        printf(" %d", found);
        if (k % 32 == 31) printf("\n");
        if (found != (k & 31)) bad++;
    }
    printf("%dx%d FP6 bit order and C/D map: %s (expected j = k %% 32: element j at bits 6 j .. 6 j + 5, little-endian)\n\n", S, S, bad ? "DIFFERS" : "as expected");
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
                for (int k = 32 * kb; k < 32 * kb + 32; k++) set_a(h, S, i, k, 0x08);  // 1.0 over the whole block
            for (int j = 0; j < S; j++) set_b(h, S, j, 32 * kb, 0x38);                  // 1.0 at the block's first value only
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

// mode 0: every code random (no NaN code); mode 1: large positive magnitudes (weights 6 .. 7.5, x in the top binades) with a few tiny
// values, so the exact sum needs far more than 24 bits
template <int S>
static double accumulate(int mode, int trials, long* inexact, long* total) {
    const int K = 2048 / S;
    static LaneIn h[64];
    static int A[32][128], B[32][128];
    double worst = 0.0;
    for (int t = 0; t < trials; t++) {
        memset(h, 0, sizeof(h));
        for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
        for (int i = 0; i < S; i++)
            for (int k = 0; k < K; k++) {
                int a, b;
                if (mode == 0) {
                    a = rnd() & 63;
                    do b = rnd() & 255; while ((b & 0x7f) == 0x7f);
                } else {
                    a = 0x1c + (rnd() & 3);
                    b = (rnd() & 7) == 0 ? 1 + (rnd() & 7) : 0x70 + (rnd() % 15);
                }
                A[i][k] = a;
                B[i][k] = b;
                set_a(h, S, i, k, a);
                set_b(h, S, i, k, b);
            }
        run<S>(h);
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                double sum = 0.0, asum = 0.0;  // exact in float64: every product is a multiple of 2^-12 below 2^12
                for (int k = 0; k < K; k++) {
                    const double p = e2m3(A[i][k]) * e4m3(B[j][k]);
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
    for (int mode = 0; mode < 2; mode++) {
        long inexact = 0, total = 0;
        const double e = accumulate<S>(mode, 64, &inexact, &total);
        printf("(c) %dx%dx%d %s: %ld of %ld exact sums are not fp32 values; largest |D - exact| = %.4f fp32 ulps of sum |products|\n", S, S, 2048 / S,
               mode ? "large positive products with a few tiny ones" : "random codes", inexact, total, e);
        if (e > w) w = e;
    }
    return w;
}

int main() {
    CK(hipMalloc(&d_in, 64 * sizeof(LaneIn)));
    CK(hipMalloc(&d_out, sizeof(h_out)));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("device: %s\nA = FP6 E2M3 (cbsz 2), B = E4M3 (blgp 0), byte selects 0\n\n", p.gcnArchName);
    int bad = 0;
    bad += byte_map<32>();
    bad += byte_map<16>();
    if (bad) {
        printf("summary: the E4M3 operand's k map was not found; parts (a2), (b), (c) not run\n");
        return 1;
    }
    bad += bit_order<32>();
    bad += bit_order<16>();
    bad += scale_map<32>();
    bad += scale_map<16>();
    const double w32 = accumulation<32>(), w16 = accumulation<16>();
    printf("\nsummary: %s; worst accumulation error of one instruction %.4f fp32 ulps of sum |products| (32x32x64: %.4f over 64 products, 16x16x128: %.4f over 128)\n",
           bad ? "the operands are NOT read as assumed" : "bit order, lane map and scale map as assumed", w32 > w16 ? w32 : w16, w32, w16);
    return bad ? 1 : 0;
}
