// Which kernel serves an MPQ (W{1,2,4,8}A16) forward call: decided once on the host (mpq_plan.hip), then launched as decided.
#pragma once
#include "bie_common.h"

namespace bie {

// the codes bie_test_mpq_forward_plan returns
enum class MpqForm : int {
    Lut = 0,         // the table-lookup / matrix-pipe decode kernels (mpq_gemv_lut.hip)
    InlineList = 1,  // the list kernel with its entries in the kernel arguments (mpq_list.hip)
    Gemv3 = 2,       // the dot2 GEMV (mpq_gemv.hip)
    Gemv = 3,        // the older GEMV: any perm, any group alignment (mpq_gemv.hip)
    GemmFused = 4,   // the MFMA GEMM with the dequantisation beside the MFMAs (mpq_gemm.hip)
    GemmDense = 5,   // dequantise once + the dense MFMA GEMM (mpq_dense.hip)
    GidxDense = 6,   // explicit irregular g_idx, per-k dequantise + the dense GEMM (mpq_dense.hip)
    Generic = 7,     // one column per lane, any shape, fp32 too (mpq_gemv.hip)
};

constexpr int GENERIC_M_CHUNK = 32;  // rows per launch of the generic kernel (its partial sums: cdiv(K, 512) x rows x N floats)

struct MpqPlan {
    MpqForm form;
    size_t workspace_bytes;  // what this form uses, head included
};

// lut_max_m: rows up to which the decode kernels are tried before everything else (0: only as the GEMV's form);
// gemv_max_m: rows up to which the GEMV is taken over the MFMA GEMM (at most 8).
MpqPlan mpq_forward_plan(int M, int K, int N, int w_bit, int group_size, int zm, int dtype, bool has_gidx, bool has_perm,
                         size_t workspace_bytes, int lut_max_m, int gemv_max_m);
// the bounds bie_mpq_forward passes: BIE_LUT_MAX_M (raw, default 16: 17 .. 32 rows on measured shapes; the decode-first bound is 32
// then) and BIE_GEMV_MAX_M (default 2), each read once per process
int mpq_lut_max_m();
int mpq_lut_first_rows();
int mpq_gemv_max_m();
bool mpq_decode_first(int M, int K, int N, int w_bit, int group_size, int dtype);
// explicit g_idx that is not a permutation of k // group_size, prefill: per-k dequantise into the fragment image + the dense GEMM
bool gidx_dense_ok(int M, int K, int N, int dtype);
// dense or fused, for a call the MFMA GEMM takes
MpqForm mpq_gemm_form(int M, int K, int N, int zm, int dtype, bool has_perm);
// sibling sets sharing x: Lut / InlineList for one grouped launch, Generic for one bie_mpq_forward per set
MpqForm mpq_grouped_form(int n_sets, const int* N, int M, int K, int w_bit, int group_size, int zm, int dtype);

// launchers: they launch the form they are given (workspace = the caller's, head first)
int mpq_forward_launch(MpqForm form, const void* x, const int32_t* qw, const void* scales, const void* zeros, const int32_t* g_idx,
                       const uint16_t* perm, const void* bias, void* y, void* workspace, int M, int K, int N, int w_bit, int group_size,
                       int zm, int dtype, hipStream_t st);
int mpq_gemv_lut_launch(MpqForm form, int nsets, const int32_t* const* qw, const void* const* scales, const void* const* zeros,
                        const void* const* bias, void* const* y, const int* N, const void* x, unsigned* counters, float* part,
                        int M, int K, int group_size, int zm, int dtype, hipStream_t st, int w_bit);
int mpq_gemm_launch_ld(MpqForm form, const void* x, const int32_t* qw, const void* scales, const void* zeros, const void* bias, void* y,
                       float* part, int M, int K, int N, int w_bit, int group_size, int zm, int dtype, const uint16_t* perm,
                       hipStream_t st, int ldy);

}  // namespace bie
