// ONE launch, MANY layers: the decode GEMV (M <= 2) of a LIST of W4 / W2 layers -- the MI355X answer to the reference's
// "one default-stream quant_mm_kernel launch per layer" (layers/qlinear/nbit/cuda/mpq_linear_cuda_kernel.cu:482-577).
//
// Why.  A 4096x4096 W4 layer is 8.9 MB: 1.1 us of HBM time, less than a kernel boundary.  A lone launch of that size spends
// its life in ramp-up, one load -> compute -> reduce round and drain (profiles/r02_lut_timeline.txt: HBM idle while the
// VALU works and vice versa; 0.18 of the roofline).  With the column tiles of MANY layers in one grid the phases of
// different workgroups overlap -- while one workgroup looks up and multiplies, its CU neighbours' rows are in flight -- and
// the launch reaches the steady-state rate of the kernel instead of its start-up transient.
//
// What an entry is: x[M, K] -> y[M, N] through (qweight, scales, zeros | qzeros, bias) exactly as bie_mpq_forward takes
// them (implicit groups).  Entries may differ in K, N and x; w_bit, group size, dtype and zero mode are common to a list.
// Entry e may name ONE earlier entry it DEPENDS on (its x is that entry's y, or is derived from it by the caller's own
// kernels -- no: only direct y -> x chains are supported): its workgroups request their weight rows first and only then
// wait for the producer's completion count, so layer l+1's weight stream runs under layer l's compute and reduction.
//
// Kernel = the table-lookup dequantisation of mpq_gemv_lut.hip (see its header for the arithmetic: the 16 doubly-rounded
// reference values of a (group, column) live in LDS as fp32, one v_perm_b32 + ds_read_b32 + FMA per weight), with
//   * weight rows, scales and zeros through BUFFER loads: the row offset is a scalar register (one s_add per row) and the
//     column offset one shared VGPR -- the 64-bit per-row VALU address arithmetic of the pointer form (0.33 VALU per
//     weight, 42 v_lshl_add_u64 per group) is gone;
//   * FMAs issued as v_pk_fma_f32 pairs with the activation pair in an SGPR pair (two weights per VALU slot);
//   * a device-resident descriptor table (entries, block -> (entry, tile, slice) records) instead of kernel arguments, so
//     a list is not bounded by the 4 KiB of kernarg space and a captured launch keeps working when the caller updates x / y
//     contents (never the pointers);
//   * the tagged-granule cross-workgroup reduction of the lookup GEMV, now FAILING LOUDLY: a reducer whose granules do not
//     arrive within the spin bound stores NaN and raises a bit in the host-visible status page (bie_device_status).
#include "mpq_dequant.cuh"
#include "mpq_list.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace bie {

unsigned* device_status_word();  // status.hip: device pointer of the host-mapped status page (NULL before bie_status_init)
void test_forge_get(unsigned* tag_skew, int* spin_limit);
int test_forge_dep_get();
int mpq_lutm_list_launch(const ListEntry* ent, const uint2_t* blk, unsigned grid, int M, int rpg, int zm, int dtype, int nw, hipStream_t st);  // mpq_gemv_lut.hip
int mpq_lutm_list_nw(int M);
int mpq_lutm_xs_list_launch(const ListEntry* ent, const uint2_t* blk, unsigned grid, int M, int rpg, int zm, int dtype, int nw, hipStream_t st);  // x-sharing form

struct ListArgs {
    const ListEntry* ent;
    const uint2_t* blk;   // per block: {entry, tile | slice << 20}
    unsigned* status;     // host-visible status word (may be NULL)
    unsigned epoch;       // (launch-call number mod 2^24) << 8
    unsigned tag_skew;    // testing aid: the reducer expects tag ^ tag_skew (forges a stale granule)
    int spin_limit;
    int M;
    int dep_extra;        // testing aid (bie_test_forge_dependency): dependent entries wait for this many tiles more than exist
};

// Inline form (bie_mpq_forward / bie_mpq_forward_grouped on the decode path): up to 8 entries that share K live in the KERNEL ARGUMENTS
// (their x / y pointers change from call to call, so no device-resident plan), and a block finds its (entry, tile, slice) by
// arithmetic: grid = S x tiles_total, slice-major; entry i owns the tiles [tile_begin_i, tile_begin_{i+1}) (tile_begin in pad0).
constexpr int LIST_MAX_INLINE = 8;
struct ListArgsInl : ListArgs {
    int n_inl, tiles_total;
    ListEntry inl[LIST_MAX_INLINE];
};

typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef const __attribute__((address_space(4))) uint32_t cu32_t;
typedef const __attribute__((address_space(4))) ListEntry cent_t;
typedef const __attribute__((address_space(4))) uint2_t cu2_t;

template <int BYTE>
__device__ __forceinline__ uint32_t list_lut_addr(uint32_t lane_addr, uint32_t w) {
    return __builtin_amdgcn_perm(w, lane_addr, 0x0c0c0400u + ((uint32_t)BYTE << 8));
}
__device__ __forceinline__ float list_lds_f32(uint32_t byte_addr) {
    return __uint_as_float(*reinterpret_cast<const lds_u32_t*>(byte_addr));
}
template <int DT, int ZM>
__device__ __forceinline__ float list_lut_entry(uint32_t q, float s, float z, int zq1) {
    if constexpr (ZM == ZM_ASYM) return dequant_scalar_asym<DT>(q, s, zq1);
    else if constexpr (ZM == ZM_FUSED) return dt_traits<DT>::round(__builtin_fmaf((float)q, s, -z));
    else return dequant_scalar_sym<DT>(q, s, z);
}

constexpr unsigned BIE_STATUS_REDUCER_TIMEOUT = 1u, BIE_STATUS_DEP_TIMEOUT = 2u;

#ifdef BIE_LAB_BUILD
// LAB builds only (make lab; tools/list_timeline.py): per wave {start, first rows landed, lookups done, end, xcc << 32 | hw id, entry << 32 | tile}
__device__ unsigned long long g_list_stamps[65536 * 6];
#define BIE_LIST_STAMP(...) __VA_ARGS__
#else
#define BIE_LIST_STAMP(...)
#endif

// VAR bit 0: v_pk_fma_f32 pairs; bit 1 (tuning aid): stream only -- rows, constants and x are loaded, nothing is looked up;
// bit 2: registers capped at 64 (four workgroups = 32 waves per CU instead of three); bit 3: four waves per workgroup instead of eight
// bit 6: D16 form (W4, M = 1, bf16) -- 16-bit table entries, two tables per wave (the units of a pair) in the halves of one 4 KiB block,
//        looked up with ds_read_u16_d16_hi (the load zeroes the low half: the register IS the fp32 value of the bf16 weight), both tables
//        built before the pair's rows are needed, lookups pipelined in half-row chunks with counted lgkmcnt (three chunks in flight)
// bit 12: ALGEBRAIC form (fp16, W4 and W2, one or two rows; independent entries).  The reference's own decode kernels accumulate in fp16
//        without materialising rounded weights (exl2/q_gemm_kernel.cuh:16-62; quant_mm_kernel :273-331 multiplies fl(q*s - z) ...), and the
//        mixed-bit lists of this library already run this way (mbwq.hip: 0.73-0.81 of HBM).  Per packed word: the nibble pairs become the
//        fp16 pairs (1024 + q[2j], 64 + q[2j+1]) with one v_perm_b32 + one v_and_or_b32 each -- the field stays where it is, the exponent is
//        chosen so that its lowest bit weighs 1 -- and go straight into v_dot2_f32_f16 against the activation pair in an SGPR: 1.5 VALU per
//        weight, NO table and NO LDS read (the table form: 2.3 VALU + one LDS read per weight, LDS-array-bound).  Per unit, in fp32:
//            y += s * (sum_k T_k x_k - sum_k c_k x_k) - z * sum_k x_k        (asym: s * (... - (zq + 1) * sum_k x_k))
//        with the two column-independent sums computed once per unit by the wave (one x dword per lane, DPP tree).  The per-weight fp16
//        roundings of the reference's CPU path (fl(fl(q*s) - z)) are NOT applied: the result is the exact products' sum (within one output ulp of the
//        float64 product), which the CPU restatement of the reference is 6-8e-4 of max|y| away from on the bench's layers (its fl(q*s) is a 1e-3
//        noise on every weight) -- inside north_star's 1e-3 norm-wise, not element by element.  Hence OPT-IN (BIE_LIST_ALG);
//        bf16 -- one output ulp is 4e-3 -- has no such form at all.
template <int DT, int ZM, int MT, int RPG, int WB, int VAR, bool INL = false>
__global__ __launch_bounds__(((VAR & 8) ? 256 : ((VAR & 16) ? 128 : ((VAR & 32) ? 64 : 512))), ((VAR & 4) ? 8 : ((VAR & 128) ? 7 : 1))) void mpq_list_kernel(const std::conditional_t<INL, ListArgsInl, ListArgs> a) {
    constexpr int NW = (VAR & 8) ? 4 : ((VAR & 16) ? 2 : ((VAR & 32) ? 1 : 8));  // bits 4 / 5 (tuning aids): two / one wave per workgroup
    constexpr int NB = 32 / WB;      // weights per packed word
    constexpr int XD = NB / 2;       // x dwords (16-bit pairs) per packed word
    constexpr bool PK = (VAR & 1) != 0 && WB == 4 && DT == BIE_BF16;
    constexpr bool STREAM_ONLY = (VAR & 2) != 0;
    constexpr bool D16 = (VAR & 64) != 0 && WB == 4 && MT == 1 && (DT == BIE_BF16 || DT == BIE_F16) && !STREAM_ONLY;
    constexpr bool ALG = (VAR & 4096) != 0 && DT == BIE_F16 && !STREAM_ONLY;  // bit 12: fp16, algebraic form (no table, no LDS in the loop) -- see process_group
    __shared__ __attribute__((aligned(4096))) uint32_t tab[NW * 16 * 64];  // the only LDS object: starts at LDS address 0

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint2_t rec;
    cent_t* e;
    int tile, slice;
    if constexpr (INL) {
        const int tcat = (int)(blockIdx.x % (unsigned)a.tiles_total);
        slice = (int)(blockIdx.x / (unsigned)a.tiles_total);
        int si = 0;
#pragma unroll
        for (int i = 1; i < LIST_MAX_INLINE; i++)
            if (i < a.n_inl && tcat >= (int)a.inl[i].pad0) si = i;
        // the entry is read with scalar loads straight from the kernel-argument segment (constant address space)
        const __attribute__((address_space(4))) char* kp = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
        e = (cent_t*)(kp + __builtin_offsetof(ListArgsInl, inl) + (size_t)si * sizeof(ListEntry));
        tile = tcat - (int)e->pad0;
        rec = uint2_t{(uint32_t)si, (uint32_t)tile};
    } else {
        rec = *((cu2_t*)(uintptr_t)(a.blk + blockIdx.x));
        e = (cent_t*)(uintptr_t)(a.ent + rec.x);
        tile = (int)(rec.y & 0xfffffu);
        slice = (int)(rec.y >> 20);
    }
    const int N = e->N, K = e->K, G = e->G, gpw = e->gpw, S = e->S, hshift = e->hshift;
    const int n = tile * 64 + lane;
    const int nl = n < N ? n : N - 1;  // clamp: out-of-range lanes load valid memory and are never stored
    const int g0 = (slice * NW + wave) * gpw;
    int g1 = g0 + gpw;
    if (g1 > G) g1 = G;
    unsigned* gen = e->gen;
    unsigned tag = 0, gen_next = 0;
    if (S > 1) {  // uniform; the generation only changes when this launch's reducer is done
        gen_next = gen[tile] + 1u;
        tag = a.epoch | (gen_next & 0xffu);
    }

    // weight rows / group constants through buffer descriptors: scalar row offset + one shared column offset register
    const auto rq = __builtin_amdgcn_make_buffer_rsrc((void*)e->qw, 0, (int)e->qw_bytes, 0x00020000);
    const unsigned col4 = (unsigned)nl * 4u;
    const uint16_t* scol = e->scales + nl;  // group constants: plain pointers (two 64-bit address adds per unit are noise, two more
    const void* zbase = e->zeros;           // buffer descriptors = 8 SGPRs in a kernel that spills SGPRs are not)
    const unsigned row_bytes = (unsigned)N * 4u;
    auto load_group = [&](uint32_t (&dst)[RPG], int unit) {
        // the row stride is made opaque at every call: otherwise the sixteen multiples u * row_bytes become loop invariants, live
        // (and spilled to VGPR lanes) across the whole lookup phase instead of fifteen s_add_u32 right here
        unsigned rb = row_bytes;
        asm volatile("" : "+s"(rb));
        unsigned soff = (unsigned)(unit * RPG) * rb;
#pragma unroll
        for (int u = 0; u < RPG; u++) {
            dst[u] = __builtin_amdgcn_raw_buffer_load_b32(rq, col4, soff, 2);  // aux 2 = nt: every weight byte is read once
            soff += rb;
        }
    };
    auto load_params = [&](int unit, uint32_t& sb, uint32_t& zb) {
        const int g = unit >> hshift;  // a group may be split into H units of RPG rows, each with its own wave (and table)
        sb = scol[(long)g * N];
        if constexpr (ZM == ZM_ASYM) {
            const uint32_t zw = reinterpret_cast<const uint32_t*>(zbase)[(long)g * (N / NB) + nl / NB];
            zb = ((zw >> ((nl % NB) * WB)) & ((1u << WB) - 1u)) + 1u;
        } else {
            zb = reinterpret_cast<const uint16_t*>(zbase)[(long)g * N + nl];
        }
    };

    float acc[MT][2];  // even / odd nibbles: two independent FMA chains (one v_pk_fma_f32 chain in the PK form)
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m][0] = acc[m][1] = 0.0f;

    // LDS byte address of tab[wave][q][lane] = ((wave * 16 + q) << 8) | (lane << 2): byte 1 carries (wave, q)
    const uint32_t lane_addr = lane * 4;
    const uint32_t wavepat = (uint32_t)wave * 0x10101010u;
    uint32_t* mytab = tab + wave * (16 * 64) + lane;
    uint32_t m0f;  // VOP3 takes no 32-bit literal: the nibble mask lives in a register
    asm("v_mov_b32 %0, 0x0f0f0f0f" : "=v"(m0f));
    const uint16_t* xbase = e->x;

    auto process_group = [&](const uint32_t (&w)[RPG], int g, uint32_t sb, uint32_t zb) {
        // the activations of the unit are wave-uniform: scalar loads, issued before the table is built so that nothing
        // but LDS traffic is pending in the lookup phase
        uint32_t xs[MT][RPG * XD];
#pragma unroll
        for (int m = 0; m < MT; m++) {
            cu32_t* xd = (cu32_t*)(uintptr_t)(xbase + (long)m * K + (long)g * (RPG * NB));
#pragma unroll
            for (int i = 0; i < RPG * XD; i++) xs[m][i] = xd[i];
        }
        if constexpr (ALG) {
            // ---- the two column-independent sums of the unit: lane i takes x dword i (pairs (x[2i], x[2i+1])), DPP tree, lane 63 holds the totals
            constexpr int ND = RPG * XD;  // x dwords of the unit
            float cu[MT], xu[MT];
            // W4: every pair carries (1024, 64); W2: the pairs of a byte alternate (1024, 256) / (64, 16)
            uint32_t cpair = 0x54006400u;
            if constexpr (WB == 2) cpair = (lane & 1) ? 0x4c005400u : 0x5c006400u;
            const uint32_t ones = 0x3c003c00u;
#pragma unroll
            for (int m = 0; m < MT; m++) {
                const uint32_t* xv = reinterpret_cast<const uint32_t*>(xbase + (long)m * K + (long)g * (RPG * NB));
                float c = 0.0f, t1 = 0.0f;
#pragma unroll
                for (int b = 0; b < ND; b += 64) {
                    const uint32_t xd = (b + lane < ND) ? xv[b + lane] : 0u;
                    c = dot2_acc<BIE_F16>(cpair, xd, c);
                    t1 = dot2_acc<BIE_F16>(ones, xd, t1);
                }
                auto tree = [](float v) -> float {
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));  // row_half_mirror
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));  // row_mirror
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false));  // row_bcast15 into rows 1 and 3
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false));  // row_bcast31 into rows 2 and 3
                    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
                };
                cu[m] = tree(c);
                xu[m] = tree(t1);
            }
            // ---- sum_k T_k x_k: per pair one v_perm_b32 (the byte into both halves) + one v_and_or_b32 (mask, exponents) + one dot2 per row of x
            float aq[MT];
#pragma unroll
            for (int m = 0; m < MT; m++) aq[m] = 0.0f;
            uint32_t mA, mB, eA, eB;  // VOP3 takes no literal: masks and exponent pairs live in registers
            if constexpr (WB == 4) {
                asm("v_mov_b32 %0, 0x00f0000f" : "=v"(mA));
                asm("v_mov_b32 %0, 0x54006400" : "=v"(eA));
                mB = mA; eB = eA;
            } else {
                asm("v_mov_b32 %0, 0x000c0003" : "=v"(mA));
                asm("v_mov_b32 %0, 0x5c006400" : "=v"(eA));
                asm("v_mov_b32 %0, 0x00c00030" : "=v"(mB));
                asm("v_mov_b32 %0, 0x4c005400" : "=v"(eB));
            }
#pragma unroll
            for (int u = 0; u < RPG; u++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t t = __builtin_amdgcn_perm(0u, w[u], 0x0c000c00u | ((uint32_t)j << 16) | (uint32_t)j);  // [byte j, 0, byte j, 0]
                    uint32_t pa;
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(pa) : "v"(t), "v"(mA), "v"(eA));
                    if constexpr (WB == 4) {
#pragma unroll
                        for (int m = 0; m < MT; m++) aq[m] = dot2_acc<BIE_F16>(pa, xs[m][u * 4 + j], aq[m]);
                    } else {
                        uint32_t pb;
                        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(pb) : "v"(t), "v"(mB), "v"(eB));
#pragma unroll
                        for (int m = 0; m < MT; m++) {
                            aq[m] = dot2_acc<BIE_F16>(pa, xs[m][u * 8 + 2 * j], aq[m]);
                            aq[m] = dot2_acc<BIE_F16>(pb, xs[m][u * 8 + 2 * j + 1], aq[m]);
                        }
                    }
                }
            }
            const float sc = f16_bits_to_f32(sb);
#pragma unroll
            for (int m = 0; m < MT; m++) {
                if constexpr (ZM == ZM_ASYM) acc[m][0] += sc * ((aq[m] - cu[m]) - (float)zb * xu[m]);
                else acc[m][0] += sc * (aq[m] - cu[m]) - f16_bits_to_f32(zb) * xu[m];
            }
            return;
        }
        // ---- the 16-entry table of this (group, column)
        if constexpr (STREAM_ONLY) {
#pragma unroll
            for (int u = 0; u < RPG; u++) acc[0][0] += __uint_as_float(w[u] & 0x3f7fffffu) + __uint_as_float(sb << 16) + __uint_as_float(zb << 16) + __uint_as_float(xs[0][u]);
            return;
        } else if constexpr (WB == 2) {
            float s, z = 0.0f;
            int zq1 = 0;
            if constexpr (DT == BIE_BF16) s = bf16_bits_to_f32(sb); else s = f16_bits_to_f32(sb);
            if constexpr (ZM == ZM_ASYM) zq1 = (int)zb;
            else if constexpr (DT == BIE_BF16) z = bf16_bits_to_f32(zb); else z = f16_bits_to_f32(zb);
            uint32_t v[4];  // the four dequantised values as 16-bit patterns
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float t = list_lut_entry<DT, ZM>((uint32_t)q, s, z, zq1);
                if constexpr (DT == BIE_BF16) v[q] = __float_as_uint(t) >> 16; else v[q] = f32_to_f16_bits(t);
            }
#pragma unroll
            for (int p2 = 0; p2 < 16; p2++) mytab[p2 * 64] = v[p2 & 3] | (v[p2 >> 2] << 16);
        } else if constexpr (DT == BIE_BF16 && ZM == ZM_SYM) {
            // a_q = fl(q*s): v_mul_f32 (exact) + v_cvt_pk_bf16_f32; T_q = fl(a_q - z): unpack-and-subtract on the dot unit
            // (bf16_pairs_sub) + v_cvt_pk_bf16_f32; the entry is the fp32 value of the bf16 weight (bf16 << 16)
            const float s = bf16_bits_to_f32(sb), nz = -bf16_bits_to_f32(zb);
            const uint32_t sel0 = sel_lo_hi<0>(), sel1 = sel_lo_hi<1>();
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t A0 = pack_bf16x2((float)(4 * j) * s, (float)(4 * j + 1) * s);
                const uint32_t A1 = pack_bf16x2((float)(4 * j + 2) * s, (float)(4 * j + 3) * s);
                float d[4];
                bf16_pairs_sub(A0, A1, sel0, sel1, nz, d);
                const uint32_t T0 = pack_bf16x2(d[0], d[1]), T1 = pack_bf16x2(d[2], d[3]);
                mytab[(4 * j + 0) * 64] = T0 << 16;
                mytab[(4 * j + 1) * 64] = T0 & 0xffff0000u;
                mytab[(4 * j + 2) * 64] = T1 << 16;
                mytab[(4 * j + 3) * 64] = T1 & 0xffff0000u;
            }
        } else {
            float s, z = 0.0f;
            int zq1 = 0;
            if constexpr (DT == BIE_BF16) s = bf16_bits_to_f32(sb); else s = f16_bits_to_f32(sb);
            if constexpr (ZM == ZM_ASYM) zq1 = (int)zb;
            else if constexpr (DT == BIE_BF16) z = bf16_bits_to_f32(zb); else z = f16_bits_to_f32(zb);
#pragma unroll
            for (int q = 0; q < 16; q++) mytab[q * 64] = __float_as_uint(list_lut_entry<DT, ZM>((uint32_t)q, s, z, zq1));
        }
        // the activations have landed (in SGPRs) before the first lookup is issued: no scalar load is pending in the lookup
        // phase, so the LDS reads can be waited for with counted lgkmcnt
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int i = 0; i < RPG * XD; i += 8)
                asm volatile("" ::"s"(xs[m][i]), "s"(xs[m][i + 1]), "s"(xs[m][i + 2]), "s"(xs[m][i + 3]), "s"(xs[m][i + 4]), "s"(xs[m][i + 5]),
                             "s"(xs[m][i + 6]), "s"(xs[m][i + 7]));
        // ---- 8 lookups + FMAs per packed word, one row ahead (lgkmcnt is a 4-bit counter: at most 15 LDS reads can be
        // waited for individually)
        auto lookup = [&](float (&t)[8], int u) {
            uint32_t we, wo;  // bytes (wave, q) of the even / odd nibbles: (w & 0x0f0f0f0f) | wavepat in ONE v_and_or_b32
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(we) : "v"(w[u]), "v"(m0f), "s"(wavepat));
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(wo) : "v"(w[u] >> 4), "v"(m0f), "s"(wavepat));
            t[0] = list_lds_f32(list_lut_addr<0>(lane_addr, we));
            t[1] = list_lds_f32(list_lut_addr<0>(lane_addr, wo));
            t[2] = list_lds_f32(list_lut_addr<1>(lane_addr, we));
            t[3] = list_lds_f32(list_lut_addr<1>(lane_addr, wo));
            t[4] = list_lds_f32(list_lut_addr<2>(lane_addr, we));
            t[5] = list_lds_f32(list_lut_addr<2>(lane_addr, wo));
            t[6] = list_lds_f32(list_lut_addr<3>(lane_addr, we));
            t[7] = list_lds_f32(list_lut_addr<3>(lane_addr, wo));
        };
        auto fmas = [&](const float (&t)[8], int u) {
            if constexpr (WB == 2) {  // t[i] = the packed pair (w[2i], w[2i+1]) of nibble i; x dword i of the word = (x[2i], x[2i+1])
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        acc[m][i & 1] = dot2_acc<DT>(__float_as_uint(t[i]), xs[m][u * 8 + i], acc[m][i & 1]);
                return;
            } else if constexpr (DT == BIE_F16) {  // fp16 x straight from the SGPR pair: v_fma_mix_f32 converts the selected half on the fly
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t p = xs[m][u * 4 + i];
                        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[0,1,0]" : "+v"(acc[m][0]) : "v"(t[2 * i]), "s"(p));
                        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(acc[m][1]) : "v"(t[2 * i + 1]), "s"(p));
                    }
                return;
            } else {
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t p = xs[m][u * 4 + i];
                        const float xlo = __uint_as_float(p << 16), xhi = __uint_as_float(p & 0xffff0000u);
                        if constexpr (PK) {  // (acc0, acc1) += (t[2i], t[2i+1]) * (xlo, xhi): one VALU slot for two weights
                            const float2_t tt = {t[2 * i], t[2 * i + 1]}, xx = {xlo, xhi};
                            float2_t aa = {acc[m][0], acc[m][1]};
                            aa = __builtin_elementwise_fma(tt, xx, aa);
                            acc[m][0] = aa.x;
                            acc[m][1] = aa.y;
                        } else {
                            acc[m][0] = __builtin_fmaf(xlo, t[2 * i], acc[m][0]);
                            acc[m][1] = __builtin_fmaf(xhi, t[2 * i + 1], acc[m][1]);
                        }
                    }
            }
        };
        // pin(): the DAG linearisation is free to sink the (unchained) FMAs below every later LDS read; a volatile asm that
        // consumes the accumulators keeps row u's FMAs between the reads of row u+1 and those of row u+2
        auto pin = [&]() {
#pragma unroll
            for (int m = 0; m < MT; m++) asm volatile("" : "+v"(acc[m][0]), "+v"(acc[m][1]));
        };
        // software pipeline, one row ahead: the eight reads of row u+1 are in flight while row u's FMAs issue.  hipcc's scheduler
        // undoes the interleave (it sinks every lookup next to its FMAs: reads, s_waitcnt lgkmcnt(0), FMAs, row after row -- the
        // LDS latency exposed sixteen times per unit), so the phases are fenced with sched_barrier
        float ta[8], tb[8];
        lookup(ta, 0);
#pragma unroll
        for (int u = 0; u < RPG; u += 2) {
            if (u + 1 < RPG) lookup(tb, u + 1);
            __builtin_amdgcn_sched_barrier(0);
            fmas(ta, u);
            pin();
            __builtin_amdgcn_sched_barrier(0);
            if (u + 1 < RPG) {
                if (u + 2 < RPG) lookup(ta, u + 2);
                __builtin_amdgcn_sched_barrier(0);
                fmas(tb, u + 1);
                pin();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    BIE_LIST_STAMP(unsigned long long st0 = wall_clock64(); unsigned long long st1 = 0;)
    uint32_t wa[RPG], wb[RPG];
    uint32_t sa = 0, za = 0, sb2 = 0, zb2 = 0;
    if (g0 < g1) {
        // the group constants are requested BEFORE the weight rows (loads return in order): the table is built while the
        // rows are still in flight instead of after the last of them has landed
        load_params(g0, sa, za);
        if (g0 + 1 < g1) load_params(g0 + 1, sb2, zb2);
        asm volatile("" ::: "memory");
        load_group(wa, g0);
        if (g0 + 1 < g1) load_group(wb, g0 + 1);
    }
    // ---- a dependent entry: the weight rows are in flight; now wait for the producer (x = its y).  ONE lane polls the producer's
    // tile count (relaxed, device scope, s_sleep between polls: 2048 polling waves would eat the weight stream's bandwidth), the
    // barrier releases the other waves, and every wave invalidates the SCALAR cache: x is read through it only (never through the
    // vector L1, so no agent-scope buffer_inv and its ~1.7 us are needed; the XCD L2s are kept coherent for device-local memory
    // by the fabric's probes), and the buffer may have been cached there by an earlier workgroup of this launch.
    const unsigned* dep = e->dep_done;
    bool dep_poison = false;  // workgroup-uniform: the producer never finished -> NaN in y, the completion count still moves
    if (dep != nullptr) {
        if (threadIdx.x == 0) {
            const unsigned target = (unsigned)(e->dep_tiles + a.dep_extra);  // the counters are zeroed by a memset node before every launch
            int spins = 0;
            unsigned seen;
            do {
                seen = __hip_atomic_load(dep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (seen >= target) break;
                __builtin_amdgcn_s_sleep(8);
            } while (++spins < a.spin_limit);
            // NaN marks a poisoned producer (its y is NaN already); a timeout is reported and poisons this entry too, so that a C-ABI
            // caller without a status page still gets no number
            if (seen < target && a.status) __hip_atomic_fetch_or(a.status, BIE_STATUS_DEP_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            tab[0] = seen < target ? 1u : 0u;  // the tables are not built yet: word 0 carries the verdict through the barrier
        }
        __syncthreads();
        dep_poison = __builtin_amdgcn_readfirstlane((int)tab[0]) != 0;
        __syncthreads();  // every wave has read the verdict before any wave writes its table
        asm volatile("s_dcache_inv\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
    }
    BIE_LIST_STAMP(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st1 = wall_clock64();)  // the wave's first two units have landed
    if constexpr (D16) {
        // ---- D16 form: see the template's header comment.  Requests in flight at any time: the rows of the current pair of units and
        // the group constants of this pair and the next (requested before the rows, so a table never waits behind rows it does not need)
        uint32_t tabw = (uint32_t)wave * 4096u + lane_addr;  // LDS byte address of (this wave, q = 0, this lane)
        const uint32_t sel0 = sel_lo_hi<0>(), sel1 = sel_lo_hi<1>();
        // Tables of a PAIR of units, built together: dword (q, lane) = T_A[q] | T_B[q] << 16, so the 32 entries go out as 8 x
        // ds_write2st64_b32 (rows q, q + 1 are 64 dwords apart) instead of 32 sixteen-bit stores -- the launch is bound by the LDS array
        // (one read per weight; profiles/r04_e_*), a store instruction costs what two reads cost.  ZM_SYM: fl(q*s) of both units in one
        // v_cvt_pk_bf16_f32, the second rounding's subtraction per half on the dot unit (selector (1,0) with -z_A, (0,1) with -z_B).
        auto build_tables = [&](uint32_t sbA, uint32_t zbA, uint32_t sbB, uint32_t zbB) {
            const uint32_t tw = tabw + 0u;  // (a plain use: clang does not capture a variable a lambda names in asm operands only)
            uint32_t D[16];
            if constexpr (DT == BIE_F16) {
                // fp16: both units' entries in ONE packed-fp16 pass -- fl(q * s) is v_pk_mul_f16, fl(. - z) v_pk_add_f16 (sym, the reference's two
                // roundings); asym: the exact integer difference (q - zq1) times s, one rounding.  Entry = (T_A[q], T_B[q]).
                const half2_t s2 = half2_t{__builtin_bit_cast(half_t, (uint16_t)sbA), __builtin_bit_cast(half_t, (uint16_t)sbB)};
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    half2_t r;
                    if constexpr (ZM == ZM_ASYM) {
                        r = half2_t{(half_t)(float)(q - (int)zbA), (half_t)(float)(q - (int)zbB)} * s2;
                    } else {
                        const half2_t z2 = half2_t{__builtin_bit_cast(half_t, (uint16_t)zbA), __builtin_bit_cast(half_t, (uint16_t)zbB)};
                        r = half2_t{(half_t)(float)q, (half_t)(float)q} * s2;
                        if constexpr (ZM == ZM_FUSED) r = __builtin_elementwise_fma(half2_t{(half_t)(float)q, (half_t)(float)q}, s2, -z2);
                        else r = r - z2;
                    }
                    D[q] = __builtin_bit_cast(uint32_t, r);
                }
            } else if constexpr (ZM == ZM_SYM) {
                const float sA = bf16_bits_to_f32(sbA), sB = bf16_bits_to_f32(sbB), nzA = -bf16_bits_to_f32(zbA), nzB = -bf16_bits_to_f32(zbB);
#pragma unroll
                for (int q = 0; q < 16; q += 2) {
                    const uint32_t A0 = pack_bf16x2((float)q * sA, (float)q * sB), A1 = pack_bf16x2((float)(q + 1) * sA, (float)(q + 1) * sB);
                    float d0, d1, d2, d3;
                    asm("v_dot2_f32_bf16 %0, %4, %6, %8\n\t"
                        "v_dot2_f32_bf16 %1, %4, %7, %9\n\t"
                        "v_dot2_f32_bf16 %2, %5, %6, %8\n\t"
                        "v_dot2_f32_bf16 %3, %5, %7, %9\n\t"
                        "s_nop 2"
                        : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)
                        : "v"(A0), "v"(A1), "v"(sel0), "v"(sel1), "v"(nzA), "v"(nzB));
                    D[q] = pack_bf16x2(d0, d1);
                    D[q + 1] = pack_bf16x2(d2, d3);
                }
            } else {
                const float sA = bf16_bits_to_f32(sbA), sB = bf16_bits_to_f32(sbB);
                float zA = 0.0f, zB = 0.0f;
                int zqA = 0, zqB = 0;
                if constexpr (ZM == ZM_ASYM) { zqA = (int)zbA; zqB = (int)zbB; } else { zA = bf16_bits_to_f32(zbA); zB = bf16_bits_to_f32(zbB); }
#pragma unroll
                for (int q = 0; q < 16; q++)  // the entries are bf16 values: their fp32 patterns have empty low halves
                    D[q] = (__float_as_uint(list_lut_entry<DT, ZM>((uint32_t)q, sA, zA, zqA)) >> 16) |
                           (__float_as_uint(list_lut_entry<DT, ZM>((uint32_t)q, sB, zB, zqB)) & 0xffff0000u);
            }
#pragma unroll
            for (int q = 0; q < 16; q += 2)
                asm volatile("ds_write2st64_b32 %0, %1, %2 offset0:%3 offset1:%4" ::"v"(tw), "v"(D[q]), "v"(D[q + 1]), "n"(q), "n"(q + 1));
        };
        float2_t accE = {0.0f, 0.0f}, accO = {0.0f, 0.0f}, accE2 = {0.0f, 0.0f}, accO2 = {0.0f, 0.0f};
        auto process_unit = [&](auto half_c, const uint32_t (&w)[RPG], int g) {
            constexpr int HALF = decltype(half_c)::value;
            const uint32_t mask = m0f + 0u, wpat = wavepat + 0u, la = lane_addr + 0u;  // plain uses (see build_table)
            uint32_t xs[RPG * 4];
            {
                cu32_t* xd = (cu32_t*)(uintptr_t)(xbase + (long)g * (RPG * 8));
#pragma unroll
                for (int i = 0; i < RPG * 4; i++) xs[i] = xd[i];
            }
#pragma unroll
            for (int i = 0; i < RPG * 4; i += 8)  // landed in SGPRs before the first lookup: nothing but LDS traffic is counted by lgkmcnt below
                asm volatile("" ::"s"(xs[i]), "s"(xs[i + 1]), "s"(xs[i + 2]), "s"(xs[i + 3]), "s"(xs[i + 4]), "s"(xs[i + 5]), "s"(xs[i + 6]), "s"(xs[i + 7]));
            constexpr int NC = 2 * RPG;  // chunks: (row, even nibbles), (row, odd nibbles)
            constexpr int RING = (VAR & 2048) ? 2 : 3;  // chunks of lookups in flight (bit 11, lab: two -- 4 registers less)
            float t[RING][4];
            uint32_t wprep[2] = {0, 0};  // even / odd prepared word of the row being issued
            auto issue = [&](int c, float (&tt)[4]) {  // c is a compile-time value after unrolling
                const int u = c >> 1;
                if ((c & 1) == 0) {
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(wprep[0]) : "v"(w[u]), "v"(mask), "s"(wpat));
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(wprep[1]) : "v"(w[u] >> 4), "v"(mask), "s"(wpat));
                }
                const uint32_t wp = wprep[c & 1];
                const uint32_t a0 = list_lut_addr<0>(la, wp), a1 = list_lut_addr<1>(la, wp), a2 = list_lut_addr<2>(la, wp), a3 = list_lut_addr<3>(la, wp);
                if constexpr ((VAR & 256) != 0) {  // ablation (lab): no LDS reads -- the address registers stand in for the looked-up values
                    tt[0] = __uint_as_float(a0); tt[1] = __uint_as_float(a1); tt[2] = __uint_as_float(a2); tt[3] = __uint_as_float(a3);
                    asm volatile("" : "+v"(tt[0]), "+v"(tt[1]), "+v"(tt[2]), "+v"(tt[3]));
                } else {
                asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(tt[0]) : "v"(a0), "n"(2 * HALF));
                asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(tt[1]) : "v"(a1), "n"(2 * HALF));
                asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(tt[2]) : "v"(a2), "n"(2 * HALF));
                asm volatile("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(tt[3]) : "v"(a3), "n"(2 * HALF));
                }
            };
            issue(0, t[0]);
            if constexpr (RING == 3) issue(1, t[1]);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if (c + RING - 1 < NC) issue(c + RING - 1, t[(c + RING - 1) % RING]);
                __builtin_amdgcn_sched_barrier(0);
                float(&tc)[4] = t[c % RING];
                // the four activations of this chunk, bf16 -> fp32 on the scalar unit, HERE: as plain expressions the DAG linearisation hoists
                // all 8 x RPG of them to the top of the unit, where they do not fit in SGPRs (112 spilled to VGPR lanes: a v_readlane per use)
                uint32_t xu[4] = {0, 0, 0, 0};
                if constexpr (DT == BIE_BF16) {
                    const int u = c >> 1;
                    if ((c & 1) == 0)
                        asm volatile("s_lshl_b32 %0, %4, 16\n\ts_lshl_b32 %1, %5, 16\n\ts_lshl_b32 %2, %6, 16\n\ts_lshl_b32 %3, %7, 16"
                                     : "=&s"(xu[0]), "=&s"(xu[1]), "=&s"(xu[2]), "=&s"(xu[3])
                                     : "s"(xs[u * 4 + 0]), "s"(xs[u * 4 + 1]), "s"(xs[u * 4 + 2]), "s"(xs[u * 4 + 3])
                                     : "scc");
                    else
                        asm volatile("s_and_b32 %0, %4, 0xffff0000\n\ts_and_b32 %1, %5, 0xffff0000\n\ts_and_b32 %2, %6, 0xffff0000\n\ts_and_b32 %3, %7, 0xffff0000"
                                     : "=&s"(xu[0]), "=&s"(xu[1]), "=&s"(xu[2]), "=&s"(xu[3])
                                     : "s"(xs[u * 4 + 0]), "s"(xs[u * 4 + 1]), "s"(xs[u * 4 + 2]), "s"(xs[u * 4 + 3])
                                     : "scc");
                }
                const int behind = (NC - 1 - c) < RING - 1 ? (NC - 1 - c) : RING - 1;  // chunks issued after chunk c
                if (behind == 2) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(tc[0]), "+v"(tc[1]), "+v"(tc[2]), "+v"(tc[3]));
                else if (behind == 1) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(tc[0]), "+v"(tc[1]), "+v"(tc[2]), "+v"(tc[3]));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tc[0]), "+v"(tc[1]), "+v"(tc[2]), "+v"(tc[3]));
                if constexpr (DT == BIE_F16) {
                    // the looked-up entry is an fp16 value in the HIGH half of its register, the activation an fp16 half of an SGPR dword: v_fma_mix_f32
                    // converts both on the fly (one VALU per weight; four independent chains)
                    const int u = c >> 1;
                    if ((c & 1) == 0) {
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "+v"(accE.x) : "v"(tc[0]), "s"(xs[u * 4 + 0]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "+v"(accE.y) : "v"(tc[1]), "s"(xs[u * 4 + 1]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "+v"(accO.x) : "v"(tc[2]), "s"(xs[u * 4 + 2]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "+v"(accO.y) : "v"(tc[3]), "s"(xs[u * 4 + 3]));
                    } else {
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(accE.x) : "v"(tc[0]), "s"(xs[u * 4 + 0]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(accE.y) : "v"(tc[1]), "s"(xs[u * 4 + 1]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(accO.x) : "v"(tc[2]), "s"(xs[u * 4 + 2]));
                        asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(accO.y) : "v"(tc[3]), "s"(xs[u * 4 + 3]));
                    }
                } else if constexpr ((VAR & 512) != 0) {  // ablation (lab): no FMAs -- the looked-up values are only consumed
                    asm volatile("" ::"v"(tc[0]), "v"(tc[1]), "v"(tc[2]), "v"(tc[3]), "s"(xu[0]), "s"(xu[1]), "s"(xu[2]), "s"(xu[3]));
                } else if ((c & 1) == 0) {  // even nibbles k = 8u + 2i: the low halves of the x dwords
                    // four chains (E, E2, O, O2): two v_pk_fma_f32 on ONE accumulator back to back cost a wait state each (the hazard recogniser's s_nop)
                    accE = __builtin_elementwise_fma(float2_t{tc[0], tc[1]}, float2_t{__uint_as_float(xu[0]), __uint_as_float(xu[1])}, accE);
                    accE2 = __builtin_elementwise_fma(float2_t{tc[2], tc[3]}, float2_t{__uint_as_float(xu[2]), __uint_as_float(xu[3])}, accE2);
                    asm volatile("" : "+v"(accE), "+v"(accE2));
                } else {
                    accO = __builtin_elementwise_fma(float2_t{tc[0], tc[1]}, float2_t{__uint_as_float(xu[0]), __uint_as_float(xu[1])}, accO);
                    accO2 = __builtin_elementwise_fma(float2_t{tc[2], tc[3]}, float2_t{__uint_as_float(xu[2]), __uint_as_float(xu[3])}, accO2);
                    asm volatile("" : "+v"(accO), "+v"(accO2));
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        uint32_t sC = 0, zC = 0, sD = 0, zD = 0;  // group constants of the NEXT pair of units
        if (g0 + 2 < g1) load_params(g0 + 2, sC, zC);
        if (g0 + 3 < g1) load_params(g0 + 3, sD, zD);
        for (int g = g0; g < g1; g += 2) {
            if constexpr ((VAR & 1024) == 0) build_tables(sa, za, sb2, zb2);  // (an odd tail builds its second table from the constants of the unit before: never read; bit 10: ablation, no tables)
            process_unit(std::integral_constant<int, 0>{}, wa, g);
            if (g + 2 < g1) load_group(wa, g + 2);
            if (g + 1 < g1) {
                process_unit(std::integral_constant<int, 1>{}, wb, g + 1);
                if (g + 3 < g1) load_group(wb, g + 3);
            }
            sa = sC; za = zC; sb2 = sD; zb2 = zD;
            if (g + 4 < g1) load_params(g + 4, sC, zC);
            if (g + 5 < g1) load_params(g + 5, sD, zD);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every table access of this wave is done before the table block is reused below
        acc[0][0] = (accE.x + accE2.x) + (accO.x + accO2.x);
        acc[0][1] = (accE.y + accE2.y) + (accO.y + accO2.y);
    } else {
        for (int g = g0; g < g1; g += 2) {
            process_group(wa, g, sa, za);
            if (g + 2 < g1) { load_params(g + 2, sa, za); load_group(wa, g + 2); }
            if (g + 1 < g1) {
                process_group(wb, g + 1, sb2, zb2);
                if (g + 3 < g1) { load_params(g + 3, sb2, zb2); load_group(wb, g + 3); }
            }
        }
    }

    BIE_LIST_STAMP(
        asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]));
        {
            const unsigned long long st2 = wall_clock64();
            const long wid = (long)blockIdx.x * NW + wave;
            if (lane == 0 && wid < 65536) {
                unsigned xcc, hwid;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
                g_list_stamps[wid * 6 + 0] = st0;
                g_list_stamps[wid * 6 + 1] = st1;
                g_list_stamps[wid * 6 + 2] = st2;
                g_list_stamps[wid * 6 + 4] = ((unsigned long long)xcc << 32) | hwid;
                g_list_stamps[wid * 6 + 5] = ((unsigned long long)rec.x << 32) | (unsigned)tile;
            }
        })
    // ---- workgroup reduction through LDS (the tables are dead), wave order --------------------------------------
    // the epilogue's fields of the entry record are read HERE (an opaque copy of its address: loads from the constant address
    // space would otherwise be hoisted to the top and occupy ~20 SGPRs through the main loop, which spills SGPRs as it is)
    cent_t* e2 = e;
    asm volatile("" : "+s"(e2));
    float tot[MT];
    __syncthreads();
    float* red = reinterpret_cast<float*>(tab);
#pragma unroll
    for (int m = 0; m < MT; m++) red[(wave * MT + m) * 64 + lane] = acc[m][0] + acc[m][1];
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int m = 0; m < MT; m++) {
        float v = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; w++) v += red[(w * MT + m) * 64 + lane];
        tot[m] = dep_poison ? __uint_as_float(0x7fc00000u) : v;  // a poisoned partial sum poisons the reducer's total as well
    }

    // ---- cross-workgroup reduction (wave 0 only): slices 0 .. S-2 publish {fp32, tag} granules, the last slice adds them in
    // slice order (deterministic) once every tag matches
    const bool owner = n < N;
    const long ncat = (long)e2->tiles * 64;
    const long col = (long)tile * 64 + lane;
    unsigned long long* gran = e2->gran;
    bool poisoned = dep_poison, red_timeout = false;
    if (S > 1) {
        if (slice != S - 1) {  // publisher: one 8-byte write-through store per column, no drain, no atomic
#pragma unroll
            for (int m = 0; m < MT; m++) {
                const unsigned long long gval = ((unsigned long long)tag << 32) | __float_as_uint(tot[m]);
                __hip_atomic_store(gran + ((long)slice * MT + m) * ncat + col, gval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        const unsigned want = tag ^ a.tag_skew;
#pragma unroll
        for (int m = 0; m < MT; m++) {
            float v = 0.0f;
            for (int s0 = 0; s0 < S - 1; s0 += 8) {
                unsigned long long gv[8];
                bool ready;
                int spins = 0;
                do {
#pragma unroll
                    for (int jj = 0; jj < 8; jj++) {
                        const int sidx = (s0 + jj < S - 1) ? s0 + jj : S - 2;
                        gv[jj] = __hip_atomic_load(gran + ((long)sidx * MT + m) * ncat + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    ready = true;
#pragma unroll
                    for (int jj = 0; jj < 8; jj++) ready = ready && ((unsigned)(gv[jj] >> 32) == want);
                    ready = __builtin_amdgcn_ballot_w64(!ready) == 0;  // wave-uniform: every lane's granules are in
                    if (!ready) __builtin_amdgcn_s_sleep(2);
                } while (!ready && ++spins < a.spin_limit);
                if (!ready) poisoned = red_timeout = true;  // wave-uniform
#pragma unroll
                for (int jj = 0; jj < 8; jj++)
                    if (s0 + jj < S - 1) v += __uint_as_float((unsigned)gv[jj]);
            }
            tot[m] = v + tot[m];
        }
        if (lane == 0) e2->gen[tile] = gen_next;  // a replay of this launch gets a different tag; visible at the kernel boundary
        if (red_timeout) {  // never a silent number: NaN in y and a bit in the status page the next C-ABI call reports
#pragma unroll
            for (int m = 0; m < MT; m++) tot[m] = __uint_as_float(0x7fc00000u);
            if (lane == 0 && a.status) __hip_atomic_fetch_or(a.status, BIE_STATUS_REDUCER_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    unsigned* done = e2->done;
    if (owner) {
#pragma unroll
        for (int m = 0; m < MT; m++) {
            float o = dt_traits<DT>::round(tot[m]);
            if (e2->bias && !poisoned) o = o + dt_traits<DT>::load(e2->bias, n);
            const long yi = (long)m * N + n;
            if (done == nullptr) {
                dt_traits<DT>::store(e2->y, yi, o);
            } else {  // a dependent entry of this launch reads y: write-through store (sc0 sc1), visible device-wide without a release fence
                uint16_t bits;
                if constexpr (DT == BIE_BF16) bits = (uint16_t)f32_to_bf16_bits(o); else bits = (uint16_t)f32_to_f16_bits(o);
                uint16_t* yp = e2->y + yi;
                asm volatile("global_store_short %0, %1, off sc0 sc1" ::"v"(yp), "v"((uint32_t)bits) : "memory");
            }
        }
    }
    // completion count of this entry (consumed by dependent entries of the same launch): this wave's write-through stores have
    // left the CU (vmcnt(0)) before the count moves -- no release fence, no L2 write-back sweep
    if (done != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    BIE_LIST_STAMP(if (lane == 0 && (long)blockIdx.x * NW < 65536) g_list_stamps[(long)blockIdx.x * NW * 6 + 3] = wall_clock64();)
}

#ifdef BIE_LAB_BUILD
extern "C" int bie_debug_list_stamps(unsigned long long* out, int n_waves) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_list_stamps), (size_t)n_waves * 6 * sizeof(unsigned long long));
}
#endif


// ---- host side ---------------------------------------------------------------------------------------------------
int status_report(const char* fn);  // splitk.hip

struct ListPlanEntry { int rpg, G, gpw, S, H, tiles, tpb; };  // tpb: column tiles per workgroup (4: the x-sharing matrix-pipe form)

struct MpqList {
    int n = 0, M = 1, w_bit = 4, group_size = 128, zm = 0, dtype = BIE_BF16;
    int rpg = 16;              // rows per unit (common to the list: one kernel instance)
    int nw = 8;                // waves per workgroup
    unsigned grid = 0;
    bool has_deps = false;
    bool lutm = false;         // the lookup / matrix-pipe kernel (mpq_gemv_lut.hip) instead of the lookup / FMA kernel below
    bool xs = false;           // ... in its x-sharing form (four column tiles per workgroup, x staged once per workgroup)
    ListEntry* d_ent = nullptr;
    uint2_t* d_blk = nullptr;
    unsigned* d_done = nullptr;
    size_t done_bytes = 0;
};

// The plan.  A wave takes `gpw` consecutive UNITS (a unit = RPG packed rows with one table: a whole quantisation group, or 1/H
// of one when the list is too small to fill the chip); 8 waves per workgroup; a column tile's K range is split over S
// workgroups.  Big lists: S = 1 (no cross-workgroup reduction at all), every wave walks several units with the next unit's
// rows in flight.  Small lists: units are split (H) and K is sliced (S) until ~`want` waves exist.
// Waves per workgroup.  W4 at M = 1: FOUR (a wave then walks twice as many units: the per-wave prologue -- descriptor loads, first
// table -- and the workgroup barriers are amortised over more weights; measured 2.02-2.04 us per 4096x4096 layer against 2.09-2.15
// with eight, 2.2 / 2.1 with two / one: profiles/r03_p_list_nw.txt).  Everything else: eight.  BIE_LIST_NW (tuning aid, lab
// configuration only) overrides.
static int list_nw(int M, int w_bit) {
    static const int nw = env_int("BIE_LIST_NW", 0);
    if (nw == 8 || nw == 4 || nw == 2 || nw == 1) return nw;
    return (M == 1 && w_bit == 4) ? 4 : 8;
}

static void list_plan(int n, const bie_mpq_list_entry* ent, int w_bit, int group_size, int* rpg_out, std::vector<ListPlanEntry>& pe, int nw = 8, int max_gpw_plan = 0,
                      int want_plan = 0) {
    static const int want_env = env_int("BIE_LIST_WANT_WAVES", 6144);
    const int want = want_plan > 0 ? want_plan : want_env;
    static const int force_h = env_int("BIE_LIST_H", 0);
    static const int max_gpw_env = env_int("BIE_LIST_MAX_GPW", 0);
    const int max_gpw = max_gpw_env > 0 ? max_gpw_env : (max_gpw_plan > 0 ? max_gpw_plan : 16);
    const int NB = 32 / w_bit;
    long units = 0;  // at H = 1
    int min_gs = group_size;
    for (int i = 0; i < n; i++) {
        const int gs = group_size > ent[i].K ? ent[i].K : group_size;
        if (gs < min_gs) min_gs = gs;
        units += (long)cdiv(ent[i].N, 64) * (ent[i].K / gs);
    }
    int rpg = min_gs / NB;  // every entry's group must be a whole number of units: validated by the caller (gs uniform or K < gs)
    int H = 1;
    if (force_h > 0) H = force_h;
    else
        while (H < 4 && rpg / (2 * H) >= 4 && units * H < want) H *= 2;
    while (H > 1 && (rpg % H || rpg / H < 4)) H /= 2;
    rpg /= H;
    units *= H;
    long gpw_global = units / want;
    if (gpw_global < 1) gpw_global = 1;
    if (gpw_global > max_gpw) gpw_global = max_gpw;
    pe.resize(n);
    for (int i = 0; i < n; i++) {
        const int gs = group_size > ent[i].K ? ent[i].K : group_size;
        ListPlanEntry& p = pe[i];
        p.rpg = rpg;
        p.H = (gs / NB) / rpg;          // units per group of THIS entry
        p.G = (ent[i].K / gs) * p.H;
        p.tiles = cdiv(ent[i].N, 64);
        int gpw = (int)gpw_global;
        const int per_wave_all = cdiv(p.G, nw);  // S = 1
        if (gpw > per_wave_all) gpw = per_wave_all;
        p.S = cdiv(p.G, gpw * nw);
        p.gpw = cdiv(p.G, p.S * nw);     // even out
        p.S = cdiv(p.G, p.gpw * nw);
        p.tpb = 1;
    }
    *rpg_out = rpg;
}

// BIE_LIST_ALG (the opt-in algebraic fp16 form, mpq_list_forward): read once per process; under BIE_TUNING per call (bench.py times both forms in one process)
static int list_alg_choice() {
    return BIE_KNOB("BIE_LIST_ALG", 0);
}

// The x-sharing matrix-pipe form (lutm_xs_body, mpq_gemv_lut.hip): a workgroup = four adjacent column tiles over the same `gpw` units, so K is
// sliced over workgroups only (nw = 1 in the arithmetic above).  Taken when the list fills the chip that way with at most XS_MAX_S slices per
// tile (each slice is a granule round of the reducer); smaller lists keep the k-split form, whose workgroup sums its four waves in LDS.
static bool list_xs_plan(int n, const bie_mpq_list_entry* ent, int M, int w_bit, int group_size, int dtype, int* rpg_out, std::vector<ListPlanEntry>& pe) {
    // plan knobs: read once per process -- per call under BIE_TUNING (tests force the form onto small lists, sweep tools change them between plans)
    struct Knobs { int min_m_f16, min_m_bf16, max_s, max_gpw, want, bf16_whole_pct, nw; };
    auto read_knobs = [] {
        return Knobs{env_int("BIE_LUTM_XS_MIN_M", 1), env_int("BIE_LUTM_XS_MIN_M_BF16", 12), env_int("BIE_LUTM_XS_MAX_S", 4),
                     env_int("BIE_LUTM_XS_MAX_GPW", 48), env_int("BIE_LUTM_XS_WANT_WAVES", 5120), env_int("BIE_LUTM_XS_BF16_WHOLE_PCT", 50), env_int("BIE_LUTM_XS_NW", 4)};
    };
    static const Knobs once = read_knobs();
    const Knobs kn = tuning() ? read_knobs() : once;
    const int min_m_f16 = kn.min_m_f16, min_m_bf16 = kn.min_m_bf16, max_s = kn.max_s, max_gpw = kn.max_gpw, want = kn.want;
    const int min_m = dtype == BIE_F16 ? min_m_f16 : (min_m_f16 <= 0 ? 0 : min_m_bf16);
    // waves wanted: 5120 makes two slices of a K = 11008 layer (43 units each) where the k-split plans' 6144 makes three; measured over 40 layers
    // of 11008x4096 at 16 / 32 rows, fp16: 4.93 / 6.23 us per layer with two slices, 5.08 / 6.54 with three, 5.02 / 6.07 with one
    // (profiles/r06_lutm_xs.txt)
    if (w_bit != 4 || M < min_m || min_m <= 0) return false;
    if (M <= 2 && dtype == BIE_F16 && list_alg_choice()) return false;  // the caller asked for the algebraic form of the one / two-row kernel
    std::vector<ListPlanEntry> px;
    int rpg;
    list_plan(n, ent, w_bit, group_size, &rpg, px, 1, max_gpw, want);
    double whole = 0.0, all = 0.0;
    for (int i = 0; i < n; i++) {
        if (px[i].S > max_s) return false;
        px[i].tpb = kn.nw == 8 ? 8 : 4;
        const double b = (double)ent[i].K * ent[i].N;
        all += b;
        if (px[i].S == 1) whole += b;
    }
    // bf16 (table form: instruction-bound, the shared x is worth 4-9 %): only from 12 rows, and only when the layers whose K one workgroup
    // walks whole hold at least half of the weights -- a sliced K = 11008 layer is 3-4 % SLOWER than in the k-split form, whose workgroup
    // of 4 x 24 units takes it whole (profiles/r06_lutm_xs.txt).  fp16 (arithmetic form): 6-27 % faster at every row count (from ONE row: 4.12 against the lookup + FMA kernel's 4.41 us per 4096x11008 layer) and shape measured
    if (dtype != BIE_F16 && whole * 100.0 < all * kn.bf16_whole_pct) return false;
    pe = px;
    *rpg_out = rpg;
    return true;
}

static bool list_shape_ok(int n, const bie_mpq_list_entry* ent, int M, int w_bit, int group_size) {
    if (n <= 0 || !ent || M < 1 || M > 32 || (w_bit != 4 && w_bit != 2)) return false;
    if (M > 2 && w_bit != 4) return false;  // 3 <= M <= 32: the matrix-pipe list kernel (mpq_gemv_lut.hip; 17 .. 32 rows: two row blocks per pass), W4 only
    const int NB = 32 / w_bit;
    int gs0 = -1;
    for (int i = 0; i < n; i++) {
        if (ent[i].K <= 0 || ent[i].N <= 0) return false;
        const int gs = group_size > ent[i].K ? ent[i].K : group_size;
        if (w_bit == 4 && gs != 32 && gs != 64 && gs != 128 && gs != 256) return false;
        if (w_bit == 2 && gs != 64 && gs != 128 && gs != 256) return false;
        if (ent[i].K % gs) return false;
        if (gs0 < 0) gs0 = gs;
        if (gs != gs0) return false;  // one kernel instance per list
        if ((long)ent[i].K * ent[i].N * w_bit / 8 > 0xfffffff0L) return false;  // 32-bit buffer offsets
        if (cdiv(ent[i].N, 64) >= (1 << 20)) return false;
        (void)NB;
    }
    return true;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct ListLayout { size_t ent, blk, gen, done, gran, total; unsigned grid; long tiles; };

static ListLayout list_layout(int n, const std::vector<ListPlanEntry>& pe, int M) {
    ListLayout L;
    long tiles = 0, blocks = 0;
    size_t gran = 0;
    for (int i = 0; i < n; i++) {
        tiles += pe[i].tiles;
        blocks += (long)cdiv(pe[i].tiles, pe[i].tpb) * pe[i].S;
        if (pe[i].S > 1) gran += (size_t)(pe[i].S - 1) * M * pe[i].tiles * 64 * 8;
    }
    L.tiles = tiles;
    L.grid = (unsigned)blocks;
    L.ent = 0;
    L.blk = align_up((size_t)n * sizeof(ListEntry), 256);
    L.gen = align_up(L.blk + (size_t)blocks * 8, 256);
    L.done = align_up(L.gen + (size_t)tiles * 4, 256);
    L.gran = align_up(L.done + (size_t)n * 4, 256);
    L.total = L.gran + gran;
    return L;
}

size_t mpq_list_device_bytes(int n, const bie_mpq_list_entry* ent, int M, int w_bit, int group_size) {
    if (!list_shape_ok(n, ent, M, w_bit, group_size)) return 0;
    std::vector<ListPlanEntry> pe;
    int rpg;
    size_t need = 0;
    // the dtype / zero mode decide the plan (tuning overrides apply to one configuration only): size for the largest of EVERY (waves, units per
    // wave) pair mpq_list_create can choose -- including the matrix-pipe form's (4, 24), which used to be planned there only (the two
    // must never be able to disagree)
    const int plans[][2] = {{8, 0}, {4, 0}, {2, 0}, {1, 0}, {4, 24}, {8, 24}};
    for (const auto& pl : plans) {
        list_plan(n, ent, w_bit, group_size, &rpg, pe, pl[0], pl[1]);
        const size_t b = list_layout(n, pe, M).total;
        if (b > need) need = b;
    }
    if (list_xs_plan(n, ent, M, w_bit, group_size, BIE_F16, &rpg, pe)) {  // the x-sharing matrix-pipe form: the plan create takes for fp16 (bf16: the same or none)
        const size_t b = list_layout(n, pe, M).total;
        if (b > need) need = b;
    }
    return need;
}

int mpq_list_create(MpqList** out, int n, const bie_mpq_list_entry* ent, int M, int w_bit, int group_size, int asym, int dtype,
                    void* device_mem, size_t device_bytes) {
    BIE_REQUIRE(out && ent && device_mem, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: NULL argument");
    BIE_REQUIRE(dtype == BIE_F16 || dtype == BIE_BF16, BIE_ERR_UNSUPPORTED, "bie_mpq_list_create: dtype %d (fp16 / bf16 only)", dtype);
    BIE_REQUIRE(list_shape_ok(n, ent, M, w_bit, group_size), BIE_ERR_UNSUPPORTED,
                "bie_mpq_list_create: a list takes 1 <= M <= 2 (w_bit 4: up to 16), w_bit 4 (groups of 32/64/128/256) or 2 (64/128/256), K a multiple of ONE common group size");
    for (int i = 0; i < n; i++) {
        BIE_REQUIRE(ent[i].x && ent[i].qweight && ent[i].scales && ent[i].zeros && ent[i].y, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: NULL tensor pointer in entry %d", i);
        BIE_REQUIRE(ent[i].depends_on < i, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: entry %d depends on entry %d, which is not EARLIER in the list", i, ent[i].depends_on);
        if (ent[i].depends_on >= 0) {
            const bie_mpq_list_entry& d = ent[ent[i].depends_on];
            BIE_REQUIRE(d.y == ent[i].x && d.N == ent[i].K, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: entry %d depends on entry %d but does not read its y (x != y or K != N)", i, ent[i].depends_on);
        }
        if (asym) BIE_REQUIRE(ent[i].N % (32 / w_bit) == 0, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: asym needs N %% %d == 0 (entry %d)", 32 / w_bit, i);
        if (M > 2) {
            BIE_REQUIRE(ent[i].depends_on < 0, BIE_ERR_UNSUPPORTED, "bie_mpq_list_create: dependent entries need M <= 2 (entry %d, M = %d)", i, M);
            BIE_REQUIRE(ent[i].N % 4 == 0, BIE_ERR_UNSUPPORTED, "bie_mpq_list_create: 3 <= M <= 32 needs N %% 4 == 0 (entry %d)", i);
            BIE_REQUIRE((reinterpret_cast<uintptr_t>(ent[i].x) & 15) == 0 && ent[i].K % 8 == 0, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: 3 <= M <= 32 needs a 16-byte aligned x and K %% 8 == 0 (entry %d)", i);
        }
        BIE_REQUIRE((reinterpret_cast<uintptr_t>(ent[i].x) & 3) == 0, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: x of entry %d must be 4-byte aligned", i);
    }
    std::vector<ListPlanEntry> pe;
    int rpg;
    list_plan(n, ent, w_bit, group_size, &rpg, pe);
    int nw = (M == 1 && w_bit == 4) ? 4 : 8;
    // W2 at one row: four waves as well (+1-2 % on three shapes in both dtypes, profiles/r06_w2_nw_ab.txt); BIE_LIST_W2_NW=8: the eight-wave arm
    static const int w2_nw = env_int("BIE_LIST_W2_NW", 4);
    if (M == 1 && w_bit == 2 && w2_nw == 4) nw = 4;
    if (dtype == BIE_BF16 && !asym && M == 1 && rpg == 16 && w_bit == 4) nw = list_nw(M, w_bit);  // the lab configuration takes the override
    // Two rows of W4 also go to the matrix-pipe kernel when the entries allow it (independent, N % 4 == 0, 16-byte aligned x): measured
    // 6.6 against 7.5 us per 4096x11008 layer for the two-row FMA form (profiles/r03_z_lutm_list_ab.txt).  BIE_LIST_M2_MFMA=0: FMA form.
    static const int m2_mfma = env_int("BIE_LIST_M2_MFMA", 1);
    bool lutm = M > 2;
    bool mfma_ok = w_bit == 4;  // what the matrix-pipe kernels ask of the entries (validated above for M > 2)
    for (int i = 0; i < n; i++)
        if (ent[i].depends_on >= 0 || ent[i].N % 4 || (reinterpret_cast<uintptr_t>(ent[i].x) & 15) || ent[i].K % 8) mfma_ok = false;
    if (M == 2 && mfma_ok && m2_mfma) lutm = true;
    if (lutm) nw = mpq_lutm_list_nw(M);  // the matrix-pipe kernel: eight waves (four at 17 <= M <= 32), each with its own 8 KiB table
    // the matrix-pipe form with four-wave workgroups: up to 24 units per wave before K is sliced over workgroups (K = 11008 stays whole:
    // 8.56 -> 7.60 us per 11008x4096 layer at 32 rows, profiles/r05_lutm_list_nw_ab.txt)
    list_plan(n, ent, w_bit, group_size, &rpg, pe, nw, (lutm && nw == 4) ? 24 : 0);
    // the x-sharing matrix-pipe form replaces the plan when the list is big enough (list_xs_plan) -- fp16 from ONE row: its arithmetic
    // dequantisation feeding the matrix pipe is faster than the lookup + FMA kernel even with fifteen of sixteen rows empty
    const bool xs = mfma_ok && list_xs_plan(n, ent, M, w_bit, group_size, dtype, &rpg, pe);
    if (xs) {
        lutm = true;
        nw = pe[0].tpb;
    }
    const ListLayout L = list_layout(n, pe, M);
    BIE_REQUIRE(device_bytes >= L.total, BIE_ERR_WORKSPACE, "bie_mpq_list_create: device buffer of %zu bytes required, got %zu", L.total, device_bytes);
    BIE_REQUIRE((reinterpret_cast<uintptr_t>(device_mem) & 255) == 0, BIE_ERR_INVALID_ARG, "bie_mpq_list_create: the device buffer must be 256-byte aligned");

    char* base = static_cast<char*>(device_mem);
    std::vector<ListEntry> he(n);
    std::vector<uint2_t> hb(L.grid);
    size_t gran_off = L.gran;
    long tile0 = 0;
    size_t b = 0;
    bool has_deps = false;
    const int esz = 2;
    for (int i = 0; i < n; i++) {
        ListEntry& e = he[i];
        memset(&e, 0, sizeof(e));
        const ListPlanEntry& p = pe[i];
        const int gs = group_size > ent[i].K ? ent[i].K : group_size;
        const long Gq = ent[i].K / gs;
        e.qw = reinterpret_cast<const uint32_t*>(ent[i].qweight);
        e.scales = reinterpret_cast<const uint16_t*>(ent[i].scales);
        e.zeros = ent[i].zeros;
        e.bias = reinterpret_cast<const uint16_t*>(ent[i].bias);
        e.x = reinterpret_cast<const uint16_t*>(ent[i].x);
        e.y = reinterpret_cast<uint16_t*>(ent[i].y);
        e.gran = p.S > 1 ? reinterpret_cast<unsigned long long*>(base + gran_off) : nullptr;
        if (p.S > 1) gran_off += (size_t)(p.S - 1) * M * p.tiles * 64 * 8;
        e.gen = reinterpret_cast<unsigned*>(base + L.gen) + tile0;
        e.done = nullptr;
        e.dep_done = nullptr;
        e.N = ent[i].N;
        e.K = ent[i].K;
        e.G = p.G;
        e.gpw = p.gpw;
        e.S = p.S;
        e.hshift = p.H == 4 ? 2 : (p.H == 2 ? 1 : 0);
        e.tiles = p.tiles;
        e.qw_bytes = (unsigned)((long)ent[i].K * w_bit / 32 * ent[i].N * 4);
        e.sc_bytes = (unsigned)(Gq * ent[i].N * esz);
        e.ze_bytes = asym ? (unsigned)(Gq * (ent[i].N * w_bit / 32) * 4) : (unsigned)(Gq * ent[i].N * esz);
        if (ent[i].depends_on >= 0) {
            has_deps = true;
            ListEntry& d = he[ent[i].depends_on];
            d.done = reinterpret_cast<unsigned*>(base + L.done) + ent[i].depends_on;
            e.dep_done = d.done;
            e.dep_tiles = d.tiles;
        }
        for (int sl = 0; sl < p.S; sl++)      // slice-major inside an entry: a tile's reducer (last slice) comes after its publishers
            for (int t = 0; t < p.tiles; t += p.tpb) hb[b++] = uint2_t{(uint32_t)i, (uint32_t)t | ((uint32_t)sl << 20)};
        BIE_REQUIRE(p.S < 4096, BIE_ERR_UNSUPPORTED, "bie_mpq_list_create: entry %d needs %d K slices (< 4096)", i, p.S);
        tile0 += p.tiles;
    }
    hipError_t err = hipMemset(base + L.gen, 0, L.total - L.gen);  // generation words, counters, granule tags: zero once
    if (err == hipSuccess) err = hipMemcpy(base + L.ent, he.data(), (size_t)n * sizeof(ListEntry), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(base + L.blk, hb.data(), (size_t)L.grid * 8, hipMemcpyHostToDevice);
    BIE_REQUIRE(err == hipSuccess, BIE_ERR_HIP, "bie_mpq_list_create: uploading the plan: %s", hipGetErrorString(err));

    MpqList* pl = new MpqList();
    pl->n = n; pl->M = M; pl->w_bit = w_bit; pl->group_size = group_size; pl->zm = asym ? ZM_ASYM : ZM_SYM; pl->dtype = dtype;
    pl->rpg = rpg;
    pl->nw = nw;
    pl->grid = L.grid;
    pl->has_deps = has_deps;
    pl->lutm = lutm;
    pl->xs = xs;
    pl->d_ent = reinterpret_cast<ListEntry*>(base + L.ent);
    pl->d_blk = reinterpret_cast<uint2_t*>(base + L.blk);
    pl->d_done = reinterpret_cast<unsigned*>(base + L.done);
    pl->done_bytes = (size_t)n * 4;
    *out = pl;
    return BIE_OK;
}

void mpq_list_destroy(MpqList* p) { delete p; }
int mpq_list_launches(const MpqList* p) { return p ? (p->has_deps ? 2 : 1) : 0; }
int mpq_list_form(const MpqList* p) { return p ? (p->xs ? 2 : (p->lutm ? 1 : 0)) : -1; }

template <int DT, int ZM, int MT, int WB, int VAR0>
static void list_launch_rpg(const ListArgs& a, int rpg, unsigned grid, hipStream_t st) {
    constexpr int VAR = VAR0 | ((MT == 1 && WB == 4) ? 8 : 0);  // W4, M = 1: four waves per workgroup (list_nw)
    constexpr int T = (VAR & 8) ? 256 : 512;
    switch (rpg) {
        case 4: hipLaunchKernelGGL((mpq_list_kernel<DT, ZM, MT, 4, WB, VAR>), dim3(grid), dim3(T), 0, st, a); break;
        case 8: hipLaunchKernelGGL((mpq_list_kernel<DT, ZM, MT, 8, WB, VAR>), dim3(grid), dim3(T), 0, st, a); break;
        case 16: hipLaunchKernelGGL((mpq_list_kernel<DT, ZM, MT, 16, WB, VAR>), dim3(grid), dim3(T), 0, st, a); break;
        default:
            if constexpr (WB == 4) hipLaunchKernelGGL((mpq_list_kernel<DT, ZM, MT, 32, WB, VAR>), dim3(grid), dim3(T), 0, st, a);
            else hipLaunchKernelGGL((mpq_list_kernel<DT, ZM, MT, 16, WB, VAR>), dim3(grid), dim3(T), 0, st, a);
            break;
    }
}
template <int DT, int WB, int VAR>
static void list_launch_zm(const ListArgs& a, int rpg, unsigned grid, int M, int zm, hipStream_t st) {
    if (M == 1) {
        if (zm == ZM_ASYM) list_launch_rpg<DT, ZM_ASYM, 1, WB, VAR>(a, rpg, grid, st);
        else list_launch_rpg<DT, ZM_SYM, 1, WB, VAR>(a, rpg, grid, st);
    } else {
        if (zm == ZM_ASYM) list_launch_rpg<DT, ZM_ASYM, 2, WB, VAR>(a, rpg, grid, st);
        else list_launch_rpg<DT, ZM_SYM, 2, WB, VAR>(a, rpg, grid, st);
    }
}

int mpq_list_forward(MpqList* p, hipStream_t st) {
    BIE_REQUIRE(p, BIE_ERR_INVALID_ARG, "bie_mpq_list_forward: NULL plan");
    int rc = status_report("bie_mpq_list_forward");
    if (rc) return rc;
    if (p->has_deps) {  // completion counters: zero before EVERY launch (a memset node, replayed with the graph)
        const hipError_t e = hipMemsetAsync(p->d_done, 0, p->done_bytes, st);
        BIE_REQUIRE(e == hipSuccess, BIE_ERR_HIP, "bie_mpq_list_forward: hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (p->xs) return mpq_lutm_xs_list_launch(p->d_ent, p->d_blk, p->grid, p->M, p->rpg, p->zm, p->dtype, p->nw, st);
    if (p->lutm)  // 2 / 3 <= M <= 32: lookups feeding v_mfma_f32_16x16x32 (mpq_gemv_lut.hip), same entries and block table
        return mpq_lutm_list_launch(p->d_ent, p->d_blk, p->grid, p->M, p->rpg, p->zm, p->dtype, p->nw, st);
    ListArgs a;
    a.ent = p->d_ent;
    a.blk = p->d_blk;
    a.status = device_status_word();
    a.epoch = next_launch_epoch();
    test_forge_get(&a.tag_skew, &a.spin_limit);
    a.M = p->M;
    a.dep_extra = test_forge_dep_get();
    static const int var = env_int("BIE_LIST_VAR", 1);  // tuning aid: 0 = scalar FMAs, 1 = v_pk_fma_f32 pairs, 2 / 3 = stream only
    const bool lab_ok = p->dtype == BIE_BF16 && p->zm == ZM_SYM && p->M == 1 && p->rpg == 16 && p->w_bit == 4;
    if (lab_ok && p->nw != 4) {
        if (p->nw == 8) hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 1>), dim3(p->grid), dim3(512), 0, st, a);
        else if (p->nw == 2) hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 17>), dim3(p->grid), dim3(128), 0, st, a);
        else hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 33>), dim3(p->grid), dim3(64), 0, st, a);
        return check_launch("mpq_list_kernel<nw>");
    }
    if (lab_ok && var != 1) {  // tuning variants (four-wave plan): scalar FMAs / stream only
        if (var == 0) hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 8>), dim3(p->grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 11>), dim3(p->grid), dim3(256), 0, st, a);
        return check_launch("mpq_list_kernel<lab>");
    }
    static const int d16 = env_int("BIE_LIST_D16", 1);  // the 16-bit-table form of the W4 / M = 1 kernel (0: the fp32-table form)
    // fp16, independent entries: BIE_LIST_ALG=1 selects the ALGEBRAIC form (template bit 12) -- 0.79-0.82 of HBM on the bench's W4 lists against
    // 0.64-0.7 for the table forms, but its results are the EXACT products' sums, 6-8e-4 of max|y| away from the reference's doubly rounded
    // weights (profiles/r05_list_alg_ab_a.txt, gpurun_out/rel_err_report.txt): inside north_star's 1e-3 norm-wise, not element by element, so
    // it is the caller's choice, not the default.  2: also W2 at one row (no faster than its pair table).
    const int alg = list_alg_choice();
    if (alg && p->dtype == BIE_F16 && !p->has_deps && (p->w_bit == 4 || p->M == 2 || alg == 2)) {
        if (p->w_bit == 2) list_launch_zm<BIE_F16, 2, 4096>(a, p->rpg, p->grid, p->M, p->zm, st);
        else list_launch_zm<BIE_F16, 4, 4096>(a, p->rpg, p->grid, p->M, p->zm, st);
        return check_launch("mpq_list_kernel<alg>");
    }
    if (d16 && p->w_bit == 4 && p->dtype == BIE_F16 && p->M == 1 && p->nw == 4) {
        list_launch_zm<BIE_F16, 4, 64>(a, p->rpg, p->grid, 1, p->zm, st);
        return check_launch("mpq_list_kernel<d16,f16>");
    }
    if (d16 && p->w_bit == 4 && p->dtype == BIE_BF16 && p->M == 1 && p->nw == 4) {
#ifdef BIE_LAB_BUILD
        static const int ring2 = env_int("BIE_LIST_RING2", 0);  // lab builds: two lookup chunks in flight, 1 = default registers, 7 = 7 waves per SIMD forced
        if (ring2 && p->rpg == 16 && p->zm == ZM_SYM) {
            if (ring2 == 7) hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 1 | 8 | 64 | 2048 | 128>), dim3(p->grid), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 1 | 8 | 64 | 2048>), dim3(p->grid), dim3(256), 0, st, a);
            return check_launch("mpq_list_kernel<d16,ring2>");
        }
        static const int abl = env_int("BIE_LIST_ABL", 0);  // lab builds: 1 no LDS reads, 2 no FMAs, 4 no table build (sums allowed: 3, 5, 6, 7)
        if (abl && p->rpg == 16 && p->zm == ZM_SYM) {
#define BIE_ABL(A) case A: hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM_SYM, 1, 16, 4, 1 | 8 | 64 | (A << 8)>), dim3(p->grid), dim3(256), 0, st, a); break;
            switch (abl) { BIE_ABL(1) BIE_ABL(2) BIE_ABL(3) BIE_ABL(4) BIE_ABL(5) BIE_ABL(6) BIE_ABL(7) default: break; }
#undef BIE_ABL
            return check_launch("mpq_list_kernel<d16,ablation>");
        }
#endif
        list_launch_zm<BIE_BF16, 4, 1 | 64>(a, p->rpg, p->grid, 1, p->zm, st);
        return check_launch("mpq_list_kernel<d16>");
    }
    if (p->w_bit == 2 && p->nw == 4 && p->M == 1) {
        if (p->dtype == BIE_F16) list_launch_zm<BIE_F16, 2, 8>(a, p->rpg, p->grid, 1, p->zm, st);
        else list_launch_zm<BIE_BF16, 2, 8>(a, p->rpg, p->grid, 1, p->zm, st);
    } else if (p->w_bit == 2) {
        if (p->dtype == BIE_F16) list_launch_zm<BIE_F16, 2, 0>(a, p->rpg, p->grid, p->M, p->zm, st);
        else list_launch_zm<BIE_BF16, 2, 0>(a, p->rpg, p->grid, p->M, p->zm, st);
    } else {
        if (p->dtype == BIE_F16) list_launch_zm<BIE_F16, 4, 0>(a, p->rpg, p->grid, p->M, p->zm, st);
        else list_launch_zm<BIE_BF16, 4, 1>(a, p->rpg, p->grid, p->M, p->zm, st);
    }
    return check_launch("mpq_list_kernel");
}

// ---- inline form: bie_mpq_forward / bie_mpq_forward_grouped on the decode path (W4, M = 1, bf16) -------------------------------
// The same kernel as the list launch (D16 form) with the entries in the kernel arguments.  Plan of a LONE launch: every wave gets
// `gpw` consecutive units of one 64-column tile (a unit = a quantisation group, or 1 / H of one when the layer is too small to fill
// the chip); about `want` waves in all, four per workgroup; K sliced over S workgroups per tile (tagged granules in the caller's
// workspace, generation words in its head).
struct InlinePlan { int rpg, G, H, gpw, S, nw; };

static InlinePlan inline_plan(int K, int group_size, int tiles_total) {
    static const int want = env_int("BIE_INL_WANT_WAVES", 4096);
    static const int max_waves = env_int("BIE_INL_MAX_WAVES", 16384);  // more waves than are resident at once: the second round starts staggered (117 MB: 29.3 against 31.0 us at 6144, 250 MB: 52.4 against 56.3; profiles/r04_t_inl_big_sweep.txt)
    static const int force_h = env_int("BIE_INL_H", 0);
    static const int force_gpw = env_int("BIE_INL_GPW", 0);
    static const int nw_env = env_int("BIE_INL_NW", 4);
    InlinePlan p;
    p.nw = nw_env == 4 ? 4 : 8;
    const int gs = group_size > K ? K : group_size;
    int rpg = gs / 8, G = K / gs, H = 1;
    if (force_h > 0) H = force_h;
    else
        while (H < 4 && rpg / (2 * H) >= 4 && (long)tiles_total * G * H < want) H *= 2;
    while (H > 1 && (rpg % H || rpg / H < 4)) H /= 2;
    p.H = H;
    p.rpg = rpg / H;
    p.G = G * H;
    int gpw = force_gpw > 0 ? force_gpw : (int)cdivl((long)tiles_total * p.G, max_waves);
    if (gpw < 1) gpw = 1;
    if (gpw > p.G) gpw = p.G;
    p.S = cdiv(p.G, gpw * p.nw);
    p.gpw = cdiv(p.G, p.S * p.nw);  // even out
    p.S = cdiv(p.G, p.gpw * p.nw);
    return p;
}

// Measured (profiles/r04_h_inl_sweep.txt, us per lone launch, per-layer lookup kernel of mpq_gemv_lut.hip against this form): 4096x4096 5.9 / 6.6,
// 4096x11008 9.7 / 10.1, q/k/v 9.8 / 10.1, gate/up 15.2 / 15.7, 8192x28672 31.3 / 29.9 -- a lone launch of a Llama-7B-sized layer is bound
// by its ramp, its per-wave latency chain and the cross-workgroup reduction, not by instruction count, and the older kernel's 8 waves per
// SIMD hide that chain better; the list form's leaner stream only pays from ~96 MB of packed weights per launch.
bool mpq_list_inline_ok(int M, int K, long n_total, int w_bit, int group_size, int zm, int dtype) {
    static const int enabled = env_int("BIE_DECODE_INLINE", 1);  // 0: never; 2: always (tuning)
    static const long min_mb = env_int("BIE_DECODE_INLINE_MIN_MB", 40);  // round 6: 96 -> 40 (gate/up of a 7B layer, 45 MB: 16.1 -> 15.5 us; profiles/r06_lone_plan_sweeps.txt)
    if (!enabled || M != 1 || w_bit != 4 || dtype != BIE_BF16 || (zm != ZM_SYM && zm != ZM_ASYM)) return false;
    const int gs = group_size > K ? K : group_size;
    if (!((gs == 32 || gs == 64 || gs == 128 || gs == 256) && K % gs == 0)) return false;
    if ((long)K / 2 * n_total > 0xfffffff0L) return false;  // 32-bit buffer offsets (per set; the sum is a safe upper bound)
    return enabled == 2 || (long)K / 2 * n_total >= min_mb * (1L << 20);
}

size_t mpq_list_inline_part_floats(int M, int K, int group_size, int tiles_total, int w_bit) {
    if (M != 1 || w_bit != 4) return 0;
    const int gs = group_size > K ? K : group_size;
    if (!(gs == 32 || gs == 64 || gs == 128 || gs == 256) || K % gs) return 0;
    const InlinePlan p = inline_plan(K, group_size, tiles_total);
    return p.S > 1 ? (size_t)(p.S - 1) * M * tiles_total * 64 * 2 : 0;
}

template <int ZM, int NWV>
static void inline_launch_rpg(const ListArgsInl& a, int rpg, unsigned grid, hipStream_t st) {
    constexpr int VAR = 1 | (NWV == 4 ? 8 : 0) | 64;
    constexpr int T = NWV * 64;
    switch (rpg) {
        case 4: hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM, 1, 4, 4, VAR, true>), dim3(grid), dim3(T), 0, st, a); break;
        case 8: hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM, 1, 8, 4, VAR, true>), dim3(grid), dim3(T), 0, st, a); break;
        case 16: hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM, 1, 16, 4, VAR, true>), dim3(grid), dim3(T), 0, st, a); break;
        default: hipLaunchKernelGGL((mpq_list_kernel<BIE_BF16, ZM, 1, 32, 4, VAR, true>), dim3(grid), dim3(T), 0, st, a); break;
    }
}

int mpq_list_inline_launch(int nsets, const int32_t* const* qw, const void* const* scales, const void* const* zeros, const void* const* bias,
                           void* const* y, const int* N, const void* x, unsigned* gen, float* gran, int K, int group_size, int zm, hipStream_t st) {
    BIE_REQUIRE(nsets >= 1 && nsets <= LIST_MAX_INLINE, BIE_ERR_INVALID_ARG, "mpq_list_inline_launch: %d sets", nsets);
    ListArgsInl a;
    memset(&a, 0, sizeof(a));
    int tiles = 0;
    for (int i = 0; i < nsets; i++) tiles += cdiv(N[i], 64);
    const InlinePlan p = inline_plan(K, group_size, tiles);
    const int gs = group_size > K ? K : group_size;
    const long Gq = K / gs;
    unsigned long long* g8 = reinterpret_cast<unsigned long long*>(gran);
    int tile0 = 0;
    for (int i = 0; i < nsets; i++) {
        ListEntry& e = a.inl[i];
        const int t = cdiv(N[i], 64);
        e.qw = reinterpret_cast<const uint32_t*>(qw[i]);
        e.scales = reinterpret_cast<const uint16_t*>(scales[i]);
        e.zeros = zeros[i];
        e.bias = bias ? reinterpret_cast<const uint16_t*>(bias[i]) : nullptr;
        e.x = reinterpret_cast<const uint16_t*>(x);
        e.y = reinterpret_cast<uint16_t*>(y[i]);
        e.gran = p.S > 1 ? g8 : nullptr;
        if (p.S > 1) g8 += (size_t)(p.S - 1) * t * 64;
        e.gen = gen + tile0;
        e.N = N[i];
        e.K = K;
        e.G = p.G;
        e.gpw = p.gpw;
        e.S = p.S;
        e.hshift = p.H == 4 ? 2 : (p.H == 2 ? 1 : 0);
        e.tiles = t;
        e.qw_bytes = (unsigned)((long)K / 8 * N[i] * 4);
        e.sc_bytes = (unsigned)(Gq * N[i] * 2);
        e.ze_bytes = zm == ZM_ASYM ? (unsigned)(Gq * (N[i] / 8) * 4) : (unsigned)(Gq * N[i] * 2);
        e.pad0 = (unsigned)tile0;  // tile_begin of this entry in the concatenated grid
        tile0 += t;
    }
    a.n_inl = nsets;
    a.tiles_total = tiles;
    a.status = device_status_word();
    a.epoch = next_launch_epoch();
    test_forge_get(&a.tag_skew, &a.spin_limit);
    a.M = 1;
    const unsigned grid = (unsigned)tiles * (unsigned)p.S;
    if (p.nw == 4) {
        if (zm == ZM_ASYM) inline_launch_rpg<ZM_ASYM, 4>(a, p.rpg, grid, st);
        else inline_launch_rpg<ZM_SYM, 4>(a, p.rpg, grid, st);
    } else {
        if (zm == ZM_ASYM) inline_launch_rpg<ZM_ASYM, 8>(a, p.rpg, grid, st);
        else inline_launch_rpg<ZM_SYM, 8>(a, p.rpg, grid, st);
    }
    return check_launch("mpq_list_kernel<inline>");
}

}  // namespace bie
