// The MPQ forward dispatch: which kernel serves a call, and the workspace that kernel uses.  The kernels' own shape rules
// (mpq_*_ok) and the measured tables stay beside their kernels; this file is the one place that combines them.
#include "mpq_plan.h"

namespace bie {
// mpq_gemv.hip
bool mpq_gemv_fast_ok(int M, int K, int N, int w_bit, int group_size, int dtype, bool has_gidx);
bool mpq_gemv3_ok(int K, int w_bit, int group_size);
size_t mpq_gemv_form_bytes(bool v3, int M, int K, int N, int w_bit, int group_size);
int mpq_gemv_launch(bool v3, const void* x, const int32_t* qw, const void* scales, const void* zeros, const void* bias, void* y,
                    float* part, int M, int K, int N, int w_bit, int group_size, int zm, int dtype, const uint16_t* perm,
                    hipStream_t st);
int mpq_gemv_generic_launch(const void* x, const int32_t* qw, const void* scales, const void* zeros, const int32_t* g_idx,
                            const void* bias, void* y, float* part, int M, int K, int N, int w_bit, int group_size,
                            int asym, int dtype, hipStream_t st, const uint16_t* perm);
// mpq_gemv_lut.hip, mpq_list.hip
bool mpq_gemv_lut_ok(int M, int K, int w_bit, int group_size, int dtype, bool has_gidx, int N = 0);
bool mpq_lut_rb2_grouped_ok(int M, int K, long n_total, int dtype);
bool mpq_list_inline_ok(int M, int K, long n_total, int w_bit, int group_size, int zm, int dtype);
size_t mpq_gemv_lut_bytes(bool inline_list, int M, int K, int group_size, int tiles_total, int w_bit, int dtype);
// mpq_gemm.hip, mpq_dense.hip
bool mpq_gemm_ok(int M, int K, int N, int w_bit, int group_size, int dtype, bool has_gidx);
size_t mpq_gemm_form_bytes(bool dense, int M, int K, int N);
bool mpq_dense_ok(int M, int K, int N);
bool mpq_dense_shape_ok(int K, int N);
size_t mpq_dense_workspace_bytes(int K, int N);
int mpq_dense_gidx_launch(const void* x, const int32_t* qw, const void* scales, const void* zeros, const int32_t* g_idx, const void* bias, void* y, void* scratch,
                          int M, int K, int N, int w_bit, int asym, int dtype, hipStream_t st);

int mpq_lut_max_m() {
    static const int v = env_int("BIE_LUT_MAX_M", 16);
    return v;
}
int mpq_lut_first_rows() { return mpq_lut_max_m() >= 16 ? 32 : mpq_lut_max_m(); }
int mpq_gemv_max_m() {
    static const int v = env_int("BIE_GEMV_MAX_M", 2);  // tuning knob
    return v;
}

// the decode kernels' rule for a lone call: one ticket / generation word per 64-column tile, four adjacent columns per 16-byte load,
// and mpq_gemv_lut_ok (which rows each form takes; 17 .. 32 on measured shapes)
static bool decode_ok(int M, int K, int N, int w_bit, int group_size, int dtype, bool has_gidx) {
    return cdiv(N, 64) <= BIE_WS_COUNTERS && (N & 3) == 0 && mpq_gemv_lut_ok(M, K, w_bit, group_size, dtype, has_gidx, N);
}
bool mpq_decode_first(int M, int K, int N, int w_bit, int group_size, int dtype) {
    return M <= mpq_lut_first_rows() && decode_ok(M, K, N, w_bit, group_size, dtype, false);
}

bool gidx_dense_ok(int M, int K, int N, int dtype) { return M > 32 && (dtype == BIE_F16 || dtype == BIE_BF16) && mpq_dense_shape_ok(K, N); }

// large M: dequantise once, dense MFMA GEMM (its fused-rounding image is fp16 only)
MpqForm mpq_gemm_form(int M, int K, int N, int zm, int dtype, bool has_perm) {
    return !has_perm && mpq_dense_ok(M, K, N) && (zm != ZM_FUSED || dtype == BIE_F16) ? MpqForm::GemmDense : MpqForm::GemmFused;
}

static MpqForm decode_form(int M, int K, long n_total, int w_bit, int group_size, int zm, int dtype) {
    return mpq_list_inline_ok(M, K, n_total, w_bit, group_size, zm, dtype) ? MpqForm::InlineList : MpqForm::Lut;
}

MpqPlan mpq_forward_plan(int M, int K, int N, int w_bit, int group_size, int zm, int dtype, bool has_gidx, bool has_perm,
                         size_t workspace_bytes, int lut_max_m, int gemv_max_m) {
    const bool decode = !has_perm && decode_ok(M, K, N, w_bit, group_size, dtype, has_gidx);
    // M <= 2: the dot2 GEMV; 3 <= M: the MFMA kernel (its dequant cost does not grow with M; measured faster from M = 3).
    // The GEMV also serves M <= 8 for shapes the MFMA tiling cannot take.
    const bool gemm = mpq_gemm_ok(M, K, N, w_bit, group_size, dtype, has_gidx);
    MpqForm f = MpqForm::Generic;
    if (decode && M <= lut_max_m)  // W4 decode and small batches
        f = decode_form(M, K, N, w_bit, group_size, zm, dtype);
    else if (M <= 8 && (M <= gemv_max_m || !gemm) && mpq_gemv_fast_ok(M, K, N, w_bit, group_size, dtype, has_gidx))
        f = decode ? decode_form(M, K, N, w_bit, group_size, zm, dtype)
                   : (!has_perm && mpq_gemv3_ok(K, w_bit, group_size) ? MpqForm::Gemv3 : MpqForm::Gemv);
    else if (gemm)
        f = mpq_gemm_form(M, K, N, zm, dtype, has_perm);
    // explicit irregular g_idx, prefill: the reference materialises the dense weight and calls cuBLAS (mpq_layer.py:59-63); here the
    // per-k dequantise writes the MFMA fragment image and the dense kernel multiplies -- when the caller sized the workspace for it
    // (bie_mpq_workspace_bytes_gidx); a smaller workspace keeps the generic kernel
    else if (has_gidx && gidx_dense_ok(M, K, N, dtype) && workspace_bytes >= BIE_WS_HEAD_BYTES + mpq_dense_workspace_bytes(K, N))
        f = MpqForm::GidxDense;
    size_t need = BIE_WS_HEAD_BYTES;
    switch (f) {
        case MpqForm::Lut:
        case MpqForm::InlineList: need = mpq_gemv_lut_bytes(f == MpqForm::InlineList, M, K, group_size, cdiv(N, 64), w_bit, dtype); break;
        case MpqForm::Gemv3:
        case MpqForm::Gemv: need = mpq_gemv_form_bytes(f == MpqForm::Gemv3, M, K, N, w_bit, group_size); break;
        case MpqForm::GemmFused:
        case MpqForm::GemmDense: need = mpq_gemm_form_bytes(f == MpqForm::GemmDense, M, K, N); break;
        case MpqForm::GidxDense: need += mpq_dense_workspace_bytes(K, N); break;
        case MpqForm::Generic: need += (size_t)cdiv(K, 512) * (M < GENERIC_M_CHUNK ? M : GENERIC_M_CHUNK) * N * sizeof(float); break;
    }
    return MpqPlan{f, need};
}

MpqForm mpq_grouped_form(int n_sets, const int* N, int M, int K, int w_bit, int group_size, int zm, int dtype) {
    int tiles = 0;
    bool n4 = true;  // the matrix-pipe form loads four adjacent columns with one 16-byte load
    long n_total = 0;
    for (int i = 0; i < n_sets; i++) {
        tiles += cdiv(N[i], 64);
        n4 = n4 && (N[i] & 3) == 0;
        n_total += N[i];
    }
    // 17 .. 32 rows: the two-row-block instance where it measured ahead of the members' own calls (mpq_lut_rb2_grouped_ok); the shape checks are those of a 16-row call
    const bool rb2 = w_bit == 4 && M > 16 && M <= 32 && n_sets > 1 && mpq_lut_rb2_grouped_ok(M, K, n_total, dtype) && mpq_gemv_lut_ok(16, K, w_bit, group_size, dtype, false);
    if (n4 && tiles <= BIE_WS_COUNTERS && (rb2 || mpq_gemv_lut_ok(M, K, w_bit, group_size, dtype, false)))
        return decode_form(M, K, n_total, w_bit, group_size, zm, dtype);
    return MpqForm::Generic;
}

int mpq_forward_launch(MpqForm form, const void* x, const int32_t* qw, const void* scales, const void* zeros, const int32_t* g_idx,
                       const uint16_t* perm, const void* bias, void* y, void* workspace, int M, int K, int N, int w_bit, int group_size,
                       int zm, int dtype, hipStream_t st) {
    float* head = reinterpret_cast<float*>(workspace);
    float* part = head + BIE_WS_HEAD_BYTES / sizeof(float);
    switch (form) {
        case MpqForm::Lut:
        case MpqForm::InlineList: {
            const void* sc1[1] = {scales};
            const void* ze1[1] = {zeros};
            const void* bi1[1] = {bias};
            void* y1[1] = {y};
            return mpq_gemv_lut_launch(form, 1, &qw, sc1, ze1, bias ? bi1 : nullptr, y1, &N, x, reinterpret_cast<unsigned*>(head) + BIE_WS_GEN_OFFSET,
                                       part, M, K, group_size, zm, dtype, st, w_bit);
        }
        case MpqForm::Gemv3:
        case MpqForm::Gemv:
            return mpq_gemv_launch(form == MpqForm::Gemv3, x, qw, scales, zeros, bias, y, head, M, K, N, w_bit, group_size, zm, dtype, perm, st);
        case MpqForm::GemmFused:
        case MpqForm::GemmDense:
            return mpq_gemm_launch_ld(form, x, qw, scales, zeros, bias, y, part, M, K, N, w_bit, group_size, zm, dtype, perm, st, N);
        case MpqForm::GidxDense:
            return mpq_dense_gidx_launch(x, qw, scales, zeros, g_idx, bias, y, part, M, K, N, w_bit, zm, dtype, st);
        case MpqForm::Generic:
            break;
    }
    // explicit g_idx / odd shapes / fp32 / MBWQ shapes no tiling takes: GENERIC_M_CHUNK rows at a time
    const size_t esz = dtype == BIE_F32 ? 4 : 2;
    for (int m0 = 0; m0 < M; m0 += GENERIC_M_CHUNK) {
        const int mc = (M - m0) < GENERIC_M_CHUNK ? (M - m0) : GENERIC_M_CHUNK;
        const int rc = mpq_gemv_generic_launch((const char*)x + (size_t)m0 * K * esz, qw, scales, zeros, g_idx, bias, (char*)y + (size_t)m0 * N * esz,
                                               part, mc, K, N, w_bit, group_size, zm, dtype, st, perm);
        if (rc) return rc;
    }
    return BIE_OK;
}

}  // namespace bie
