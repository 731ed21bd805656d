// What the translation units on the block-scaled matrix instructions share (gfx950; mxfp4_a4 / _a6 / _a8, mxfp6_a6 / _a8, mxfp8_a8 and
// the grouped mxfp4_moe_a4 / _a6 / _a8, mxfp6_moe_a6 / _a8): the instructions' operand types, the three operand formats (FP4 E2M1, FP6
// E2M3, FP8 E4M3) as the facts in which a kernel's handling of them differs, the store of four consecutive columns of one row of y, and
// the one prefill tile body on v_mfma_scale_f32_32x32x64_f8f6f4 (mx_scaled_gemm_tile), parameterised on the formats of its two operands.
// The decode bodies on v_mfma_scale_f32_16x16x128_f8f6f4 are in mx_scaled_decode.cuh, on the same three format types.  The quantisers'
// units and rows stay with their formats (mxfp4_a4_common.cuh, mxfp4_a8_common.cuh, mxfp6_common.cuh).
#pragma once
#include "mxfp4_common.cuh"

namespace bie {

typedef int mxa4_v8i __attribute__((ext_vector_type(8)));
typedef float mxa4_v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float a4_nan() { return __uint_as_float(0x7fc00000u); }

// ---- a lane's operand of the instructions, per format ---------------------------------------------------------------------------------------
// In every pair of formats the scale byte of lane group g applies to block g (k = 32 g .. 32 g + 31 of the instruction's K) on either
// operand, and byte j of a lane group of A meets byte j of that lane group of B; what differs is which k a lane group's registers hold.

// FP4: four of the eight registers, lane group g holds block g as its 16 bytes in memory (code j in bits 4 j .. 4 j + 3), whatever the
// partner's format (profiles/mxfp4_a4_scale_probe.txt, mxfp4_a8_probe.txt, mxfp4_a6_probe.txt).
__device__ __forceinline__ mxa4_v8i a4_frag(const uint4_t& v) { return mxa4_v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0}; }

// FP6: six of the eight registers from a block's three 8-byte pieces.  Lane group g holds block g as its 24 bytes in memory (code j in
// bits 6 j .. 6 j + 5 of the block's little-endian 192-bit integer), with an E4M3, an FP6 or an FP4 partner (tools/probe/probe_mx_fp6.hip
// part (a2), probe_mx_fp6x6.hip part (a), probe_mx_fp4x6.hip; profiles/mxfp6_a8_probe.txt, mxfp6_a6_probe.txt, mxfp4_a6_probe.txt).
__device__ __forceinline__ mxa4_v8i a6_frag(const uint2_t& p0, const uint2_t& p1, const uint2_t& p2) {
    return mxa4_v8i{(int)p0.x, (int)p0.y, (int)p1.x, (int)p1.y, (int)p2.x, (int)p2.y, 0, 0};
}

// E4M3: all eight registers from two 16-byte halves that are NOT one block of 32 (tools/probe/probe_mx_a8.hip, profiles/mxfp4_a8_probe.txt;
// the same with an FP6 partner, profiles/mxfp6_a8_probe.txt part (a1), and with an E4M3 one on both sides, tools/probe/probe_mx_fp8x8.hip,
// profiles/mxfp8_a8_probe.txt): of the G = 2 (32x32x64) or 4 (16x16x128) lane groups, group g holds in bytes 0 .. 15 the elements
// k = 16 g .. 16 g + 15 of the instruction's K and in bytes 16 .. 31 the elements k = 16 G + 16 g .. + 15.  The row stays row-major in
// memory: a lane takes its halves from two places of the row, nothing is permuted in registers.
__device__ __forceinline__ mxa4_v8i a8_frag(const uint4_t& lo, const uint4_t& hi) {
    return mxa4_v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// a load of the weight stream (NT: non-temporal, every byte is read once) or of x
template <bool NT, class T>
__device__ __forceinline__ T mx_ld(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// ---- the three operand formats ----------------------------------------------------------------------------------------------------------------
// What the tile needs to know of an operand's format: the bytes of a block of 32 (BLOCK), the widest aligned piece a row can be copied
// in (piece_t, PIECE bytes), the pitch of a row of a BK-k stage in LDS with the reason for its pad, how lane group hh's fragment of
// k-step ks (64 k) is read from such a row, and the instruction's format code (cbsz for A, blgp for B).  The decode kernels
// (mx_scaled_decode.cuh, 16x16x128: lane group kq of four, 128-k step s of a row held in memory) need which runs of the row make up a
// lane's fragment: PARTS runs of part_t, run i in block part_block(s, kq, i) at byte part_off(kq) of that block.  The scale byte is
// always that of block 4 s + kq.
struct mx_op_fp4 {
    static constexpr int BLOCK = 16, PIECE = 16, CODE = 4;
    typedef uint4_t piece_t;
    // 80 bytes (20 dwords) at 128 k: the 16-byte fragment reads of 16 consecutive rows fall on distinct banks
    static constexpr int pitch(int BK) { return BK / 2 + 16; }
    static __device__ __forceinline__ mxa4_v8i frag(const unsigned char* row, int ks, int hh) {
        return a4_frag(*reinterpret_cast<const uint4_t*>(row + (ks * 2 + hh) * 16));
    }
    static constexpr int PARTS = 1;  // block 4 s + kq, whole
    typedef uint4_t part_t;
    static __device__ __forceinline__ int part_block(int s, int kq, int) { return 4 * s + kq; }
    static __device__ __forceinline__ int part_off(int) { return 0; }
    template <bool NT>
    static __device__ __forceinline__ part_t part_load(const uint8_t* p) { return mx_ld<NT>(reinterpret_cast<const uint4_t*>(p)); }
    static __device__ __forceinline__ mxa4_v8i lane_frag(const part_t (&v)[1]) { return a4_frag(v[0]); }
};

struct mx_op_fp6 {
    static constexpr int BLOCK = 24, PIECE = 8, CODE = 2;  // a row is 24 K / 32 bytes: nothing wider than 8 bytes is aligned, in memory or in LDS
    typedef uint2_t piece_t;
    // 104 bytes (26 dwords) at 128 k.  A lane's fragment is the 24 bytes at row * 104 + 24 * block, three 8-byte reads.  The lanes of a
    // half-wave read the same block of rows r = 0 .. 31: per piece the dwords 26 r + c and 26 r + c + 1.  As ds_read_b64 (served per 32
    // lanes, bank = dword mod 64): 26 r mod 64 = 2 (13 r mod 32) takes 32 distinct even values, so the 32 dword pairs tile all 64 banks.
    // As ds_read2_b64, which the compiler emits for two of the three pieces (each piece served per 16 consecutive lanes, bank = dword
    // mod 32): 26 r mod 32 = 2 (13 r mod 16) takes 16 distinct even values over 16 consecutive r, so the 16 pairs tile all 32 banks.  No
    // conflict either way.  (96 + 16 = 112 bytes, FP4's and E4M3's pad, would put the two buffers of a 128 x 128 FP6 x E4M3 tile at
    // 67584 bytes, over the 64 KiB of static LDS; with 104 they are exactly 65536.)
    static constexpr int pitch(int BK) { return BK / 32 * 24 + 8; }
    static __device__ __forceinline__ mxa4_v8i frag(const unsigned char* row, int ks, int hh) {
        const uint2_t* p = reinterpret_cast<const uint2_t*>(row + (ks * 2 + hh) * 24);
        return a6_frag(p[0], p[1], p[2]);
    }
    static constexpr int PARTS = 1;  // block 4 s + kq, whole, in its three 8-byte pieces
    struct part_t { uint2_t p0, p1, p2; };
    static __device__ __forceinline__ int part_block(int s, int kq, int) { return 4 * s + kq; }
    static __device__ __forceinline__ int part_off(int) { return 0; }
    template <bool NT>
    static __device__ __forceinline__ part_t part_load(const uint8_t* p) {
        const uint2_t* q = reinterpret_cast<const uint2_t*>(p);
        return part_t{mx_ld<NT>(q), mx_ld<NT>(q + 1), mx_ld<NT>(q + 2)};
    }
    static __device__ __forceinline__ mxa4_v8i lane_frag(const part_t (&v)[1]) { return a6_frag(v[0].p0, v[0].p1, v[0].p2); }
};

struct mx_op_e4m3 {
    static constexpr int BLOCK = 32, PIECE = 16, CODE = 0;
    typedef uint4_t piece_t;
    // 144 bytes (36 dwords) at 128 k and 80 bytes (20 dwords) at 64 k: the 16-byte fragment reads of 16 consecutive rows fall on distinct banks
    static constexpr int pitch(int BK) { return BK + 16; }
    static __device__ __forceinline__ mxa4_v8i frag(const unsigned char* row, int ks, int hh) {
        const uint4_t* p = reinterpret_cast<const uint4_t*>(row + ks * 64 + hh * 16);
        return a8_frag(p[0], p[2]);  // bytes 16 hh .. + 15 of the step's first block and of its second (a8_frag)
    }
    static constexpr int PARTS = 2;  // bytes 16 (kq & 1) .. + 15 of blocks 4 s + (kq >> 1) and + 2: each half has its own in-range test
    typedef uint4_t part_t;
    static __device__ __forceinline__ int part_block(int s, int kq, int i) { return 4 * s + (kq >> 1) + 2 * i; }
    static __device__ __forceinline__ int part_off(int kq) { return 16 * (kq & 1); }
    template <bool NT>
    static __device__ __forceinline__ part_t part_load(const uint8_t* p) { return mx_ld<NT>(reinterpret_cast<const uint4_t*>(p)); }
    static __device__ __forceinline__ mxa4_v8i lane_frag(const part_t (&v)[2]) { return a8_frag(v[0], v[1]); }
};

// ---- four consecutive columns of one row of y -------------------------------------------------------------------------------------------------
// v[0 .. 3] are columns n .. n + 3 (n < N, n a multiple of 4) of the row of y at yr; c is the index of column n in ecol / bias.  A
// flagged row of x and a column with e_col = 255 are NaN; the bias is added after that.  One 8-byte store where N allows it.
template <int DT>
__device__ __forceinline__ void mx_store4(float (&v)[4], bool rbad, const uint8_t* __restrict__ ecol, const void* __restrict__ bias, long c,
                                          uint16_t* __restrict__ yr, int n, int N) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (n + r < N) {
            if (rbad || ecol[c + r] == 255u) v[r] = a4_nan();
            if (bias) v[r] += dt_traits<DT>::load(bias, c + r);
        }
    }
    if ((N & 3) == 0) {
        uint16_t h[4];
        dt_traits<DT>::store(h, 0, v[0]); dt_traits<DT>::store(h, 1, v[1]);
        dt_traits<DT>::store(h, 2, v[2]); dt_traits<DT>::store(h, 3, v[3]);
        uint2_t o;
        o.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
        o.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
        *reinterpret_cast<uint2_t*>(yr + n) = o;
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (n + r < N) dt_traits<DT>::store(yr, n + r, v[r]);
    }
}

// ---- the prefill tile ---------------------------------------------------------------------------------------------------------------------------
// One operand's NR rows of a BK-k stage, from memory through registers to LDS.  A row's stage is a contiguous run of BK / 32 blocks in
// memory and is copied as it stands, in pieces t, t + 256, ... of the NR rows (row = piece / pieces per row); a piece is live when its
// row is and its block lies below K / 32, and zero otherwise.
template <class Op, int NR, int BK>
struct mx_stage_rows {
    static constexpr int RB = BK / 32 * Op::BLOCK, PPR = RB / Op::PIECE, LD = NR * PPR / 256, PITCH = Op::pitch(BK);
    static_assert(Op::BLOCK % Op::PIECE == 0 && NR * PPR % 256 == 0, "whole pieces per block, whole slots per thread");
    const uint8_t* src[LD];
    int blk[LD], dst[LD];
    bool ok[LD];
    typename Op::piece_t r[LD];

    // source(row, ok) -> the row of `base` that stage row `row` reads (a valid one also when ok comes back false)
    template <class Source>
    __device__ __forceinline__ void init(int t, const uint8_t* __restrict__ base, int KB, const Source& source) {
#pragma unroll
        for (int i = 0; i < LD; i++) {
            const int p = t + 256 * i, row = p / PPR, off = (p - row * PPR) * Op::PIECE;
            blk[i] = off / Op::BLOCK;
            dst[i] = row * PITCH + off;
            src[i] = base + source(row, ok[i]) * ((long)KB * Op::BLOCK) + off;
        }
    }
    // stage kt, with src at that stage: the stages are loaded in order, advance() between two loads
    __device__ __forceinline__ void load(int kt, int KB) {
#pragma unroll
        for (int i = 0; i < LD; i++)
            r[i] = (ok[i] && kt * (BK / 32) + blk[i] < KB) ? *reinterpret_cast<const typename Op::piece_t*>(src[i]) : typename Op::piece_t{};
    }
    __device__ __forceinline__ void advance() {
#pragma unroll
        for (int i = 0; i < LD; i++) src[i] += RB;
    }
    __device__ __forceinline__ void store(unsigned char* st) const {
#pragma unroll
        for (int i = 0; i < LD; i++) *reinterpret_cast<typename Op::piece_t*>(st + dst[i]) = r[i];
    }
};

// One (64 WM rows) x (64 WN columns) tile of y = x . W^T (+ bias) with block-scaled weights of format OpW (the A operand) and block-scaled
// activations of format OpX (the B operand).  Tile rows from `rows` (mxfp4_common.cuh; they index xq / xs / row_flag), columns n0 .. of
// the N weight rows that start at row r0 of qw / sc / ecol / bias (0, or (long)e * N for an expert e).  4 waves as 2 x 2; per 64 k a wave
// reads WM x fragments and WN weight fragments with as many scale bytes and issues WM * WN MFMAs.  The weight fragment is the A operand,
// so a lane's accumulator holds 4 consecutive columns of one row of y.  LDS stage, double-buffered and filled through registers:
// x codes [64 WM][OpX::pitch], weight codes [64 WN][OpW::pitch], both row-major as in memory, then one scale dword per row, x rows first
// (byte j of a row's dword = the scale of the stage's block j).  Dead rows and whatever lies past N / K: zero codes under scale 2^0.
// BK is the k per stage: 128, but 64 for the 128 x 128 tile of two E4M3 operands, whose two buffers at 128 would need 2 x 37888 = 75776
// bytes, over the 65536 of static LDS (2 x 21504 = 43008 at 64).  All 256 threads must call it together.
template <int DT, int WM, int WN, class OpW, class OpX, class Rows, int BK = 128>
__device__ __forceinline__ void mx_scaled_gemm_tile(const Rows& rows, const uint8_t* __restrict__ xq, const uint8_t* __restrict__ xs,
                                                    const uint8_t* __restrict__ row_flag, const uint8_t* __restrict__ qw, const uint8_t* __restrict__ sc,
                                                    const uint8_t* __restrict__ ecol, const void* __restrict__ bias, void* __restrict__ y, long r0, int n0,
                                                    int N, int K) {
    static_assert(BK == 64 || BK == 128, "a stage is one or two 64-k steps");
    constexpr int BM = 64 * WM, BN = 64 * WN, ROWS = BM + BN, SB = BK / 32;
    constexpr int XPITCH = OpX::pitch(BK), WPITCH = OpW::pitch(BK);
    constexpr int WOFF = BM * XPITCH, SOFF = WOFF + BN * WPITCH;
    constexpr int STAGE = SOFF + ROWS * 4;
    static_assert(ROWS <= 256, "at most one scale dword per thread and stage");
    static_assert(WOFF % 16 == 0 && SOFF % 16 == 0 && STAGE % 16 == 0, "16-byte pieces, dword scales");
    static_assert(2 * STAGE <= 65536, "two stages must fit the static LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wy = wave >> 1, wx = wave & 1;
    const int KB = K >> 5, KT = (K + BK - 1) / BK;

    // load slots: x pieces, then weight pieces; thread t < ROWS also loads the scales of row t of the stage image (rows 0 .. BM - 1 = x,
    // BM .. = weights)
    auto xsource = [&](int row, bool& ok) -> long {
        ok = rows.live(row);
        return ok ? rows.src(row) : 0L;
    };
    auto wsource = [&](int row, bool& ok) -> long {
        ok = n0 + row < N;
        return r0 + min(n0 + row, N - 1);
    };
    mx_stage_rows<OpX, BM, BK> lx;
    mx_stage_rows<OpW, BN, BK> lw;
    lx.init(t, xq, KB, xsource);
    lw.init(t, qw, KB, wsource);
    const bool s_thread = ROWS == 256 || t < ROWS;
    bool sok = false;
    const uint8_t* ssrc = xs;
    if (s_thread) ssrc = t < BM ? xs + xsource(t, sok) * KB : sc + wsource(t - BM, sok) * KB;
    uint32_t rs = 0x7f7f7f7fu;
    auto load = [&](int kt) {
        lx.load(kt, KB);
        lw.load(kt, KB);
        if (s_thread) {
            rs = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int kb = kt * SB + j;
                const uint32_t s = (j < SB && sok && kb < KB) ? (uint32_t)ssrc[kb] : 127u;
                rs |= s << (8 * j);
            }
        }
    };
    // src walks along the rows here and not in load(): a load's address is then ready a stage ahead, and the adds stay off the path from
    // the loads to their use (a workgroup with few live rows runs at that path's latency)
    auto store = [&](int buf) {
        lx.advance();
        lw.advance();
        unsigned char* st = lds + buf * STAGE;
        lx.store(st);
        lw.store(st + WOFF);
        if (s_thread) reinterpret_cast<uint32_t*>(st + SOFF)[t] = rs;
    };

    float16_t acc[WN][WM];  // [weight row block j][x row block i]: D rows = columns n of y, D columns = rows of the tile
#pragma unroll
    for (int j = 0; j < WN; j++)
#pragma unroll
        for (int i = 0; i < WM; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[j][i][r] = 0.0f;

    const int rl = lane & 31, hh = lane >> 5;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < KT; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < KT) load(kt + 1);
        const unsigned char* st = lds + buf * STAGE;
        const uint32_t* ss = reinterpret_cast<const uint32_t*>(st + SOFF);
        uint32_t sxa[WM], swa[WN];  // the row's scale bytes, shifted so that this lane's block of k-step ks sits in byte 2 ks
#pragma unroll
        for (int i = 0; i < WM; i++) sxa[i] = ss[wy * 32 * WM + i * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int j = 0; j < WN; j++) swa[j] = ss[BM + wx * 32 * WN + j * 32 + rl] >> (8 * hh);
#pragma unroll
        for (int ks = 0; ks < BK / 64; ks++) {
            mxa4_v8i fx[WM], fw[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) fx[i] = OpX::frag(st + (wy * 32 * WM + i * 32 + rl) * XPITCH, ks, hh);
#pragma unroll
            for (int j = 0; j < WN; j++) fw[j] = OpW::frag(st + WOFF + (wx * 32 * WN + j * 32 + rl) * WPITCH, ks, hh);
#pragma unroll
            for (int j = 0; j < WN; j++)
#pragma unroll
                for (int i = 0; i < WM; i++)
                    acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[j][i], OpW::CODE, OpX::CODE, 0,
                                                                                (int)((swa[j] >> (16 * ks)) & 0xffu), 0, (int)((sxa[i] >> (16 * ks)) & 0xffu));
        }
        if (kt + 1 < KT) store(buf ^ 1);
        __syncthreads();
    }

    // C/D: D column (= tile row) = lane & 31, D row (= column n of y) = (r & 3) + 8 (r >> 2) + 4 hh: registers 4q .. 4q + 3 are four
    // consecutive n of one row (mx_store4).
#pragma unroll
    for (int i = 0; i < WM; i++) {
        const int row = wy * 32 * WM + i * 32 + rl;
        if (!rows.live(row)) continue;
        const bool rbad = row_flag[rows.src(row)] != 0;
        uint16_t* yr = reinterpret_cast<uint16_t*>(y) + rows.dst(row) * N;
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int n = n0 + wx * 32 * WN + j * 32 + 8 * q + 4 * hh;
                if (n >= N) continue;
                float v[4] = {acc[j][i][4 * q], acc[j][i][4 * q + 1], acc[j][i][4 * q + 2], acc[j][i][4 * q + 3]};
                mx_store4<DT>(v, rbad, ecol, bias, r0 + n, yr, n, N);
            }
    }
}

}  // namespace bie
