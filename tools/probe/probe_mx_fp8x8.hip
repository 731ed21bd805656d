// How v_mfma_scale_f32_32x32x64_f8f6f4 / v_mfma_scale_f32_16x16x128_f8f6f4 read an FP8 x FP8 pair of operands on gfx950: A = E4M3
// (cbsz 0, eight VGPRs), B = E4M3 (blgp 0, eight VGPRs).  profiles/mxfp4_a8_probe.txt and profiles/mxfp6_a8_probe.txt pinned the E4M3
// operand as B beside an FP4 / FP6 A only.  With two byte operands no side has a known map, so nothing is assumed: a position is
// p = 32 * lane group + byte (byte j of a lane's 32 operand bytes, little-endian over its eight registers), and for both shapes
//   (a1) for every B position, the A position whose value it multiplies: B one-hot there (2^(col % 4 - 1), every column), A codes
//        distinct per (row, byte) in ONE lane group at a time and zeros elsewhere; -1 where no A position or several answer
//   (a2) the mirror image: A one-hot per position, B distinct codes: the B position per A position
//   (b)  for every position, the lane whose scale byte applies to it, on either operand (every lane's scale a distinct power of two),
//        printed as the k-block = (lane - (row | column)) / S, and whether the lane is (row | column) + S * k-block throughout.
//        The hypothesis (a8_frag of csrc/mxfp4_a8_common.cuh, there with an FP4 partner): with G = 2 / 4 lane groups, group g holds
//        k = 16 g .. + 15 in bytes 0 .. 15 and k = 16 G + 16 g .. + 15 in bytes 16 .. 31, so that its bytes 0 .. 15 lie in block g / 2
//        and its bytes 16 .. 31 in block G / 2 + g / 2, and the scale byte of lane group g applies to block g.  Only a position's
//        partner (a) and its block (b) can be observed: the order of k inside a block has no effect on D
//   (c)  the accumulation error of ONE instruction against the exact sum (128-bit integers), in fp32 ulps of sum |products|: on codes
//        of 0.25 .. 7.5 under one scale, where every exact sum is an fp32 value (products on a 2^-10 grid below 2^6, so 128 of them
//        need 23 bits), on every non-NaN code under one scale, and on every non-NaN code under random block scales
//   (d)  what an E4M3 NaN code (0x7F / 0xFF) in the A operand (the weights of csrc/mxfp8_a8.hip) does to D, against a non-zero and a
//        zero partner, and the same in the B operand
//   hipcc --offload-arch=gfx950 -O2 -o probe_mx_fp8x8 probe_mx_fp8x8.hip && ./probe_mx_fp8x8 > profiles/mxfp8_a8_probe.txt
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

struct LaneIn { int a[8], b[8], sa, sb; };

__global__ __launch_bounds__(64) void k32(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], v.a[4], v.a[5], v.a[6], v.a[7]}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], v.b[6], v.b[7]};
    v16f c;
    for (int r = 0; r < 16; r++) c[r] = 0.f;
    c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, v.sa, 0, v.sb);
    // C/D: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    for (int r = 0; r < 16; r++) out[((r & 3) + 8 * (r >> 2) + 4 * (threadIdx.x >> 5)) * 32 + (threadIdx.x & 31)] = c[r];
}
__global__ __launch_bounds__(64) void k16(const LaneIn* in, float* out) {
    const LaneIn v = in[threadIdx.x];
    const v8i a = {v.a[0], v.a[1], v.a[2], v.a[3], v.a[4], v.a[5], v.a[6], v.a[7]}, b = {v.b[0], v.b[1], v.b[2], v.b[3], v.b[4], v.b[5], v.b[6], v.b[7]};
    v4f c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, v.sa, 0, v.sb);
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

// OCP e4m3fn: bit 7 sign, bits 6:3 exponent (bias 7), bits 2:0 mantissa; 0x7F / 0xFF are NaN, no infinity.  value = mant * 2^ex
static void e4m3_parts(int c, int* mant, int* ex) {
    const int e = (c >> 3) & 15, m = c & 7;
    *mant = (e ? 8 + m : m) * ((c & 0x80) ? -1 : 1);
    *ex = (e ? e : 1) - 10;
}
static double e4m3(int c) {
    int m, e;
    e4m3_parts(c, &m, &e);
    return ldexp((double)m, e);
}
static int all4(int c) { return c | c << 8 | c << 16 | c << 24; }
static int expo(float v) { return (v > 0.f && isfinite(v)) ? (int)lrintf(log2f(v)) : -9999; }

static void set_byte(int* regs, int j, int code) { reinterpret_cast<uint32_t*>(regs)[j >> 2] |= (uint32_t)code << (8 * (j & 3)); }
// either operand by position p = 32 * lane group + byte; idx = row of A / column of B
static void set_a(LaneIn* h, int S, int idx, int p, int code) { set_byte(h[idx + S * (p >> 5)].a, p & 31, code); }
static void set_b(LaneIn* h, int S, int idx, int p, int code) { set_byte(h[idx + S * (p >> 5)].b, p & 31, code); }
static void set_op(LaneIn* h, int S, int which, int idx, int p, int code) { which ? set_b(h, S, idx, p, code) : set_a(h, S, idx, p, code); }

static int dcode(int idx, int j) { return (j * 5 + idx * 11) % 119 + 1; }  // 0x01 .. 0x77, distinct over the j of one row: distinct positive values
static int hcode(int idx) { static const int c[4] = {0x30, 0x38, 0x40, 0x48}; return c[idx & 3]; }  // 0.5, 1, 2, 4

// hot = 1: B one-hot, A distinct (a1); hot = 0: A one-hot, B distinct (a2)
template <int S>
static int pair_map(int hot) {
    const int K = 2048 / S, KB = K / 32;
    int bad = 0;
    static LaneIn h[64];
    const char* H = hot ? "B" : "A";
    const char* D = hot ? "A" : "B";
    printf("(a%d) %dx%dx%d: %s one-hot 2^(%s %% 4 - 1) at byte j of lane group g, %s code (5 j' + 11 %s) %% 119 + 1 at byte j' of one lane group g' at a time: %s position 32 g' + j' whose value came out, per %s byte\n",
           hot ? 1 : 2, S, S, K, H, hot ? "col" : "row", D, hot ? "row" : "col", D, H);
    for (int p = 0; p < K; p++) {
        int found = -2;
        for (int gd = 0; gd < KB; gd++) {
            memset(h, 0, sizeof(h));
            for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
            for (int i = 0; i < S; i++)
                for (int j = 0; j < 32; j++) set_op(h, S, 1 - hot, i, 32 * gd + j, dcode(i, j));
            for (int c = 0; c < S; c++) set_op(h, S, hot, c, p, hcode(c));
            run<S>(h);
            int zero = 1, here = -2;
            for (int i = 0; i < S * S; i++)
                if (h_out[i] != 0.0f) zero = 0;
            if (zero) continue;
            for (int i = 0; i < S; i++)      // index of the operand with distinct codes
                for (int c = 0; c < S; c++) {  // index of the one-hot operand
                    const float v = hot ? h_out[i * S + c] : h_out[c * S + i];  // D[row of A][column of B]
                    int f = -1;
                    for (int jj = 0; jj < 32; jj++)
                        if ((double)v == e4m3(dcode(i, jj)) * e4m3(hcode(c))) f = jj;
                    if (here == -2) here = f;
                    else if (f != here) here = -1;
                }
            found = (found == -2 && here >= 0) ? 32 * gd + here : -1;
        }
        if (found == -2) found = -1;
        if (p % 32 == 0) printf("  lane group %d:", p / 32);
        printf(" %d", found);
        if (p % 32 == 31) printf("\n");
        if (found != p) bad++;
    }
    printf("%dx%d %s byte map and C/D map: %s (expected %s position = %s position: byte j of lane group g meets byte j of lane group g)\n\n", S, S, H,
           bad ? "DIFFERS" : "as expected", D, H);
    return bad;
}

static int blk32[64], blk16[128];  // position -> k-block, as part (b) found it (the same on both operands, or part (b) fails)

template <int S>
static int scale_map() {
    const int K = 2048 / S, G = K / 32;
    int* blk = S == 32 ? blk32 : blk16;
    int bad = 0;
    static LaneIn h[64];
    for (int which = 0; which < 2; which++) {  // 0: scale A carries the lane tag, 1: scale B
        printf("(b) %dx%dx%d, scale %c = 2^(lane - 32) in all four bytes, the other scale 2^0, 1.0 at one position of both operands: k-block = (the lane whose byte scaled it - (row|col)) / %d, per byte\n",
               S, S, K, which ? 'B' : 'A', S);
        for (int p = 0; p < K; p++) {
            memset(h, 0, sizeof(h));
            for (int l = 0; l < 64; l++) {
                h[l].sa = all4(which == 0 ? 95 + l : 127);
                h[l].sb = all4(which == 1 ? 95 + l : 127);
            }
            for (int i = 0; i < S; i++) {
                set_a(h, S, i, p, 0x38);
                set_b(h, S, i, p, 0x38);
            }
            run<S>(h);
            int kb = -2;
            for (int i = 0; i < S; i++)
                for (int j = 0; j < S; j++) {
                    const float v = which == 0 ? h_out[i * S + j] : h_out[j * S + i];  // A tags rows of D, B tags columns
                    const int l = expo(v) + 32 - i;
                    const int b = (l >= 0 && l % S == 0 && l / S < G) ? l / S : -1;
                    if (kb == -2) kb = b;
                    else if (b != kb) kb = -1;
                }
            const int g = p >> 5, j = p & 31;
            const int want = j < 16 ? g / 2 : G / 2 + g / 2;
            if (p % 32 == 0) printf("  lane group %d:", g);
            printf(" %d", kb);
            if (p % 32 == 31) printf("\n");
            if (kb != want) bad++;
            if (which == 0) blk[p] = kb < 0 ? 0 : kb;
            else if (blk[p] != kb) bad++;
        }
    }
    printf("%dx%d scale map: %s (expected bytes 0 .. 15 of lane group g in k-block g / 2 and bytes 16 .. 31 in k-block %d + g / 2, i.e. k = 16 g + j and k = %d + 16 g + j - 16; the scale of k-block b from lane (row|col) + %d b; the same on A and B)\n\n",
           S, S, bad ? "DIFFERS" : "as expected", G / 2, 16 * G, S);
    return bad;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static int any_code() {  // every code but the two NaN codes
    int c;
    do c = rnd() & 255; while ((c & 0x7f) == 0x7f);
    return c;
}

// mode 0: codes of magnitude 0.25 .. 7.5 (exponent fields 5 .. 9), random signs; mode 1: large positive magnitudes (6 .. 7.5) with a few
// of 0.25 .. 0.47; both under scale 2^0, where every exact sum is an fp32 value.  mode 2: every non-NaN code (2^-9 .. 448) under scale
// 2^0.  mode 3: every non-NaN code, every block's scale random in 2^-8 .. 2^8 on either operand.  Exact sums in units of 2^-52 in
// 128-bit integers (the smallest product is 2^-18 * 2^-16, the largest sum below 2^42)
template <int S>
static double accumulate(int mode, int trials, long* inexact, long* total) {
    const int K = 2048 / S;
    const int* blk = S == 32 ? blk32 : blk16;
    static LaneIn h[64];
    static int A[32][128], B[32][128], SA[32][4], SB[32][4];
    double worst = 0.0;
    for (int t = 0; t < trials; t++) {
        memset(h, 0, sizeof(h));
        for (int i = 0; i < S; i++)
            for (int kb = 0; kb < K / 32; kb++) {  // the scale byte of lane group kb applies to block kb on either operand: part (b)
                SA[i][kb] = mode == 3 ? 119 + (int)(rnd() % 17) : 127;
                SB[i][kb] = mode == 3 ? 119 + (int)(rnd() % 17) : 127;
                h[i + S * kb].sa = all4(SA[i][kb]);
                h[i + S * kb].sb = all4(SB[i][kb]);
            }
        for (int i = 0; i < S; i++)
            for (int p = 0; p < K; p++) {
                int a, b;
                if (mode == 0) {
                    a = (rnd() & 0x80) | ((5 + rnd() % 5) << 3) | (rnd() & 7);
                    b = (rnd() & 0x80) | ((5 + rnd() % 5) << 3) | (rnd() & 7);
                } else if (mode == 1) {
                    a = 0x4c + (rnd() & 3);
                    b = (rnd() & 7) == 0 ? 0x28 + (rnd() & 7) : 0x4c + (rnd() & 3);
                } else {
                    a = any_code();
                    b = any_code();
                }
                A[i][p] = a;
                B[i][p] = b;
                set_a(h, S, i, p, a);
                set_b(h, S, i, p, b);
            }
        run<S>(h);
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                __int128 sum = 0, asum = 0;  // units of 2^-52
                for (int p = 0; p < K; p++) {
                    int ma, ea, mb, eb;
                    e4m3_parts(A[i][p], &ma, &ea);
                    e4m3_parts(B[j][p], &mb, &eb);
                    const int sh = ea + eb + SA[i][blk[p]] + SB[j][blk[p]] - 254 + 52;  // >= 52 - 18 - 16
                    const __int128 pr = (__int128)(ma * mb) << sh;
                    sum += pr;
                    asum += pr < 0 ? -pr : pr;
                }
                (*total)++;
                const double ds = (double)sum;
                if ((__int128)(double)(float)ds != sum) (*inexact)++;
                if (asum == 0) continue;
                const double dd = ldexp((double)h_out[i * S + j], 52);  // exact: a power-of-two multiple of an fp32 value
                double diff;
                if (isfinite(dd) && dd == floor(dd) && fabs(dd) < ldexp(1.0, 120)) {
                    const __int128 e = (__int128)dd - sum;
                    diff = (double)(e < 0 ? -e : e);
                } else {
                    diff = fabs(dd - ds);
                }
                const double ulp = ldexp(1.0, (int)floor(log2((double)asum)) - 23);
                const double err = diff / ulp;
                if (!(err <= worst)) worst = err;  // a NaN in D is carried out as the worst
            }
    }
    return worst;
}

template <int S>
static double accumulation() {
    static const char* names[4] = {"codes of 0.25 .. 7.5, scales 2^0", "large positive products with a few tiny ones, scales 2^0", "every non-NaN code, scales 2^0",
                                   "every non-NaN code, random block scales 2^-8 .. 2^8"};
    double w = 0.0;
    for (int mode = 0; mode < 4; mode++) {
        long inexact = 0, total = 0;
        const double e = accumulate<S>(mode, 64, &inexact, &total);
        printf("(c) %dx%dx%d %s: %ld of %ld exact sums are not fp32 values; largest |D - exact| = %.4f fp32 ulps of sum |products|\n", S, S, 2048 / S, names[mode],
               inexact, total, e);
        if (!(e <= w)) w = e;
    }
    return w;
}

// Row 3 of A (or column 3 of B) holds the NaN code at position 5 and 1.0 elsewhere; the other operand holds 1.0 everywhere, or 1.0
// with 0.0 at position 5.  Printed: how many of the S outputs of that row (column) are NaN, and how many of the other outputs are
template <int S>
static void nan_codes() {
    const int K = 2048 / S;
    static LaneIn h[64];
    for (int which = 0; which < 2; which++)
        for (int code = 0x7f; code <= 0xff; code += 0x80)
            for (int zero = 0; zero < 2; zero++) {
                memset(h, 0, sizeof(h));
                for (int l = 0; l < 64; l++) h[l].sa = h[l].sb = all4(127);
                for (int i = 0; i < S; i++)
                    for (int p = 0; p < K; p++) {
                        set_op(h, S, which, i, p, (i == 3 && p == 5) ? code : 0x38);
                        set_op(h, S, 1 - which, i, p, (zero && p == 5) ? 0x00 : 0x38);
                    }
                run<S>(h);
                int in_nan = 0, out_nan = 0, out_ok = 0;
                for (int i = 0; i < S; i++)
                    for (int j = 0; j < S; j++) {
                        const float v = h_out[i * S + j];
                        const bool mine = (which == 0 ? i : j) == 3;
                        if (mine) in_nan += isnan(v) ? 1 : 0;
                        else if (isnan(v)) out_nan++;
                        else if (v == (float)(zero ? K - 1 : K)) out_ok++;
                    }
                printf("(d) %dx%dx%d code 0x%02X at one position of %s 3 of %c, the partner %s there: %d of the %d outputs of that %s are NaN; of the other %d, %d are NaN and %d are the exact sum\n",
                       S, S, K, code, which ? "column" : "row", which ? 'B' : 'A', zero ? "0.0" : "1.0", in_nan, S, which ? "column" : "row", S * S - S, out_nan, out_ok);
            }
}

int main() {
    CK(hipMalloc(&d_in, 64 * sizeof(LaneIn)));
    CK(hipMalloc(&d_out, sizeof(h_out)));
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    printf("device: %s\nA = FP8 E4M3 (cbsz 0), B = FP8 E4M3 (blgp 0), byte selects 0\n\n", p.gcnArchName);
    int bad = 0;
    bad += pair_map<32>(1);
    bad += pair_map<16>(1);
    bad += pair_map<32>(0);
    bad += pair_map<16>(0);
    bad += scale_map<32>();
    bad += scale_map<16>();
    const double w32 = accumulation<32>(), w16 = accumulation<16>();
    printf("\n");
    nan_codes<32>();
    nan_codes<16>();
    printf("\nsummary: %s; worst accumulation error of one instruction %.4f fp32 ulps of sum |products| (32x32x64: %.4f over 64 products, 16x16x128: %.4f over 128)\n",
           bad ? "the operands are NOT read as assumed" : "byte pairing, block map and scale map as assumed", w32 > w16 ? w32 : w16, w32, w16);
    return bad ? 1 : 0;
}
