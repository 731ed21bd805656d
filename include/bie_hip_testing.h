/* bie_hip_testing.h -- fault-injection hooks of libbie_hip.so.  TEST INFRASTRUCTURE, not part of the drop-in boundary
 * (include/bie_hip.h): nothing under bitorch_engine/ calls these; tests/test_gpu_parity.py does, to prove that the in-kernel
 * hand-offs fail loudly. */
#ifndef BIE_HIP_TESTING_H
#define BIE_HIP_TESTING_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Make the split-K reducers of subsequent launches expect tag ^ tag_skew and give up after spin_limit polls; the dependency
 * waits of list launches give up after spin_limit polls too.  (0, 0) restores normal operation.  Forges a stale granule /
 * a producer that never finishes. */
void bie_test_forge_reducer(unsigned tag_skew, int spin_limit);
/* Make dependent list entries of subsequent launches wait for `extra` more producer tiles than exist (a producer that never
 * finishes); 0 restores normal operation. */
void bie_test_forge_dependency(int extra);
/* Which kernel bie_mpq_forward would launch for a call of this shape (sym, no perm; workspace_bytes as the caller passes it), and the
 * workspace that kernel uses in *need (when need is not NULL).  Host only.  Returns the form: 0 the decode (lookup) kernels, 1 the inline
 * list kernel, 2 the v3 GEMV, 3 the older GEMV, 4 the fused MFMA GEMM, 5 dequantise + dense GEMM, 6 the g_idx dense form, 7 generic. */
int bie_test_mpq_forward_plan(int M, int K, int N, int w_bit, int group_size, int dtype, int has_gidx, size_t workspace_bytes, size_t* need);
/* The launch shape the fused MFMA GEMM takes for (M, K, N) under the current knobs (BIE_GEMM_BM, BIE_GEMM_S, BIE_GEMM_PLAN_TABLE): tile
 * height, split-K factor and K tiles (of 64) per split, each written when its pointer is not NULL.  Host only.  Returns 1 when the plan is
 * a cell of the measured table (csrc/mpq_gemm_plan_table.inc), 0 when the cost model chose it, negative when K % 64 != 0. */
int bie_test_mpq_gemm_plan(int M, int K, int N, int* BM, int* S, int* tiles_per_split);

#ifdef __cplusplus
}
#endif
#endif
