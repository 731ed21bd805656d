// The host side of the block-scaled MX layers, written once: the plan, the workspace layout and the launchers of the six dense layers
// (W4A4, W4A6, W4A8, W6A6, W6A8, W8A8) and of the five grouped expert layers (W4A4, W4A6, W4A8, W6A6, W6A8).  A layer's .hip file keeps
// its kernels, its measured constants and a small traits type that names them; the templates below are instantiated there, once per
// layer, and the mxfp*_..._launch / _form / _decode_ok / _workspace_bytes symbols are one-line definitions over them.
//
// A knob's name reaches BIE_KNOB as a static member of the layer's type: the macro caches the value in a static of a captureless
// lambda, so every template instance (every layer) keeps a cache of its own.  Nothing here reads the environment otherwise, allocates,
// or dispatches through anything but a template parameter.
#pragma once
#include "bie_common.h"

namespace bie {

int mxfp4_a4_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st);  // mxfp4_a4.hip
int mxfp4_a8_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st);  // mxfp4_a8.hip
int mxfp6_a6_quantize_launch(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* row_flag, long M, long K, int dtype, hipStream_t st);  // mxfp6_a6.hip
// mxfp4_moe.hip: the routing region of the grouped form
size_t mxfp4_moe_workspace_bytes(long P, long E);
long mxfp4_moe_max_tiles(long P, long E);
int mxfp4_moe_route_launch(const int32_t* idx, void* workspace, long P, long E, hipStream_t st);

static inline size_t mx_al16(size_t v) { return (v + 15) / 16 * 16; }

// ---- activation formats -------------------------------------------------------------------------------------------------------------------
// row_bytes: the code bytes of a quantised row; dense_xs_offset: where xs starts in a dense layer's workspace (only the MXFP4 layout
// rounds it up to 16; 24 M K/32 and M K are multiples of 8 and of 32); quantize: the launcher that writes xq / xs / row_flag.
struct mx_act_fp4 {
    static long row_bytes(long K) { return K / 2; }
    static size_t dense_xs_offset(long M, long K) { return (size_t)((M * (K / 2) + 15) / 16 * 16); }
    static int quantize(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* rf, long M, long K, int dtype, hipStream_t st) {
        return mxfp4_a4_quantize_launch(x, xq, xs, rf, M, K, dtype, st);
    }
};
struct mx_act_fp6 {
    static long row_bytes(long K) { return K / 32 * 24; }
    static size_t dense_xs_offset(long M, long K) { return (size_t)(M * (K / 32) * 24); }
    static int quantize(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* rf, long M, long K, int dtype, hipStream_t st) {
        return mxfp6_a6_quantize_launch(x, xq, xs, rf, M, K, dtype, st);
    }
};
struct mx_act_e4m3 {
    static long row_bytes(long K) { return K; }
    static size_t dense_xs_offset(long M, long K) { return (size_t)(M * K); }
    static int quantize(const void* x, uint8_t* xq, uint8_t* xs, uint8_t* rf, long M, long K, int dtype, hipStream_t st) {
        return mxfp4_a8_quantize_launch(x, xq, xs, rf, M, K, dtype, st);
    }
};

// ---- dense layers -------------------------------------------------------------------------------------------------------------------------
// A dense layer L states: act (an activation format above); form_knob; decode_rows, plan_rows (the decode form exists for
// M <= decode_rows and the plan takes it for M <= plan_rows); decode_name, gemm_name (for check_launch); decode<DT, G>() (the decode
// kernel for 16 G rows) and gemm<DT, W>() (the prefill kernel on (64 W) x (64 W) tiles, W = 2 or 1; the rest of the tile is the layer's).
template <class L>
bool mx_dense_decode_ok(long M) { return M >= 1 && M <= L::decode_rows; }

template <class L>
int mx_dense_form(long M) {
    const int f = BIE_KNOB(L::form_knob, -1);
    if (f == 0 && M <= L::decode_rows) return 0;
    if (f == 1) return 1;
    return M <= L::plan_rows ? 0 : 1;
}

// Workspace of a dense forward: xq [M, row_bytes] (16-byte aligned), xs [M, K/32], row_flag [M]
template <class L>
size_t mx_dense_flag_offset(long M, long K) { return L::act::dense_xs_offset(M, K) + (size_t)(M * (K / 32)); }
template <class L>
size_t mx_dense_workspace_bytes(long M, long K) { return (mx_dense_flag_offset<L>(M, K) + (size_t)M + 15) / 16 * 16; }

template <class L, int DT>
static void mx_dense_launch_dt(const uint8_t* xq, const uint8_t* xs, const uint8_t* rf, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                               const void* bias, void* y, int M, int N, int K, int form, hipStream_t st) {
    if (form == 0) {
        const dim3 grid((unsigned)cdiv(N, 16));
        if (M <= 16) hipLaunchKernelGGL((L::template decode<DT, 1>()), grid, dim3(256), 0, st, xq, xs, rf, qw, sc, ecol, bias, y, M, N, K);
        else if (M <= 32) hipLaunchKernelGGL((L::template decode<DT, 2>()), grid, dim3(256), 0, st, xq, xs, rf, qw, sc, ecol, bias, y, M, N, K);
        else hipLaunchKernelGGL((L::template decode<DT, 4>()), grid, dim3(256), 0, st, xq, xs, rf, qw, sc, ecol, bias, y, M, N, K);
        return;
    }
    // 128 x 128 tiles where they give every CU of the card (256) at least two workgroups, else 64 x 64 tiles: four times the workgroups
    // for the small-M cells, at twice the LDS fragment reads per MFMA
    if ((long)cdiv(M, 128) * cdiv(N, 128) >= 512) {
        const int tn = cdiv(N, 128);
        hipLaunchKernelGGL((L::template gemm<DT, 2>()), dim3((unsigned)(cdiv(M, 128) * tn)), dim3(256), 0, st, xq, xs, rf, qw, sc, ecol, bias, y, M, N, K, tn);
    } else {
        const int tn = cdiv(N, 64);
        hipLaunchKernelGGL((L::template gemm<DT, 1>()), dim3((unsigned)(cdiv(M, 64) * tn)), dim3(256), 0, st, xq, xs, rf, qw, sc, ecol, bias, y, M, N, K, tn);
    }
}

// The contraction from quantised activations, form 0 (decode) or 1 (prefill).
template <class L>
int mx_dense_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* rf, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol,
                         const void* bias, void* y, long M, long N, long K, int dtype, int form, hipStream_t st) {
    if (dtype == BIE_F16) mx_dense_launch_dt<L, BIE_F16>(xq, xs, rf, qw, sc, ecol, bias, y, (int)M, (int)N, (int)K, form, st);
    else mx_dense_launch_dt<L, BIE_BF16>(xq, xs, rf, qw, sc, ecol, bias, y, (int)M, (int)N, (int)K, form, st);
    return check_launch(form == 0 ? L::decode_name : L::gemm_name);
}

// The whole layer from x: the quantise launch into the workspace, then the contraction.
template <class L>
int mx_dense_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, void* workspace, long M,
                            long N, long K, int dtype, int form, hipStream_t st) {
    uint8_t* xq = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* xs = xq + L::act::dense_xs_offset(M, K);
    uint8_t* rf = xq + mx_dense_flag_offset<L>(M, K);
    const int rc = L::act::quantize(x, xq, xs, rf, M, K, dtype, st);
    if (rc) return rc;
    return mx_dense_gemm_launch<L>(xq, xs, rf, qw, sc, ecol, bias, y, M, N, K, dtype, form, st);
}

// ---- grouped expert layers ----------------------------------------------------------------------------------------------------------------
// A grouped layer L states: act; form_knob; strip_knob and wn_knob (nullptr where the layer has no such knob); one_k (the largest K of
// the one-launch decode form); decode_pairs (the decode form exists for P <= decode_pairs); the plan constants plan_pairs,
// plan_pairs_sparse and plan_sparse_mul (the plan takes the decode form for P <= plan_pairs, and up to plan_pairs_sparse while
// plan_sparse_mul * P <= E); strip (C16 of the decode form) and wn (the column tile, 64 wn columns; the row tile is the routing's);
// decode_name, gemm_name; decode<DT, C16, FUSED>() and gemm<DT, WN>() (a layer with one tile width ignores WN).
template <class L>
bool mx_grouped_decode_ok(long P) { return P >= 1 && P <= L::decode_pairs; }
template <class L>
bool mx_grouped_one_launch_ok(long K) { return K <= L::one_k; }

template <class L>
int mx_grouped_form(long P, long E) {
    const int f = BIE_KNOB(L::form_knob, -1);
    if (f == 0 && P <= L::decode_pairs) return 0;
    if (f == 1) return 1;
    return (P <= L::plan_pairs || (P <= L::plan_pairs_sparse && L::plan_sparse_mul * P <= E)) ? 0 : 1;
}

// Workspace of a grouped forward, every region 16-byte aligned: xq [R, row_bytes], xs [R, K/32], row_flag [R] for the R stored rows of
// x (T, or P with x_per_pair), then for the grouped form the routing region of mxfp4_moe.hip.
static inline long mx_grouped_rows(long T, long S, int x_per_pair) { return x_per_pair ? T * S : T; }
template <class L>
size_t mx_grouped_xs_offset(long R, long K) { return mx_al16((size_t)R * (size_t)L::act::row_bytes(K)); }
template <class L>
size_t mx_grouped_flag_offset(long R, long K) { return mx_grouped_xs_offset<L>(R, K) + mx_al16((size_t)R * (size_t)(K / 32)); }
template <class L>
size_t mx_grouped_route_offset(long R, long K) { return mx_grouped_flag_offset<L>(R, K) + mx_al16((size_t)R); }

template <class L>
size_t mx_grouped_workspace_bytes(long T, long S, long E, long K, int x_per_pair, int form) {
    return mx_grouped_route_offset<L>(mx_grouped_rows(T, S, x_per_pair), K) + (form == 1 ? mxfp4_moe_workspace_bytes(T * S, E) : 0);
}

template <class L, int DT, int C16, bool FUSED>
static void mx_grouped_decode_launch_t(const void* xin, const uint8_t* xs, const uint8_t* rf, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                                       const uint8_t* ecol, const void* bias, void* y, long P, int S, int E, int N, int K, int xpp, hipStream_t st) {
    const dim3 grid((unsigned)cdivl(N, 16 * C16), (unsigned)P);
    hipLaunchKernelGGL((L::template decode<DT, C16, FUSED>()), grid, dim3(256), 0, st, xin, xs, rf, idx, qw, sc, ecol, bias, y, S, E, N, K, xpp);
}

// The routed decode kernel; xin is x (FUSED) or the quantised rows.
template <class L, int DT, bool FUSED>
static int mx_grouped_decode_launch(const void* xin, const uint8_t* xs, const uint8_t* rf, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                                    const uint8_t* ecol, const void* bias, void* y, long P, long S, long E, long N, long K, int xpp, hipStream_t st) {
    if constexpr (L::strip_knob != nullptr) {
        const int strip = BIE_KNOB(L::strip_knob, L::strip);
        if (strip >= 4) mx_grouped_decode_launch_t<L, DT, 4, FUSED>(xin, xs, rf, idx, qw, sc, ecol, bias, y, P, (int)S, (int)E, (int)N, (int)K, xpp, st);
        else if (strip >= 2) mx_grouped_decode_launch_t<L, DT, 2, FUSED>(xin, xs, rf, idx, qw, sc, ecol, bias, y, P, (int)S, (int)E, (int)N, (int)K, xpp, st);
        else mx_grouped_decode_launch_t<L, DT, 1, FUSED>(xin, xs, rf, idx, qw, sc, ecol, bias, y, P, (int)S, (int)E, (int)N, (int)K, xpp, st);
    } else {
        mx_grouped_decode_launch_t<L, DT, L::strip, FUSED>(xin, xs, rf, idx, qw, sc, ecol, bias, y, P, (int)S, (int)E, (int)N, (int)K, xpp, st);
    }
    return check_launch(L::decode_name);
}

template <class L, int DT, int WN>
static void mx_grouped_gemm_launch_t(const uint8_t* xq, const uint8_t* xs, const uint8_t* rf, const int32_t* ws, const uint8_t* qw, const uint8_t* sc,
                                     const uint8_t* ecol, const void* bias, void* y, long S, long E, long N, long K, int xpp, int max_tiles, hipStream_t st) {
    const dim3 grid((unsigned)(max_tiles * cdivl(N, 64 * WN)));
    hipLaunchKernelGGL((L::template gemm<DT, WN>()), grid, dim3(256), 0, st, xq, xs, rf, ws, qw, sc, ecol, bias, y, (int)S, (int)E, (int)N, (int)K, xpp,
                       max_tiles);
}

template <class L, int DT>
static void mx_grouped_gemm_launch_dt(const uint8_t* xq, const uint8_t* xs, const uint8_t* rf, const int32_t* ws, const uint8_t* qw, const uint8_t* sc,
                                      const uint8_t* ecol, const void* bias, void* y, long S, long E, long N, long K, int xpp, int max_tiles, hipStream_t st) {
    if constexpr (L::wn_knob != nullptr) {
        if (BIE_KNOB(L::wn_knob, L::wn) >= 2) mx_grouped_gemm_launch_t<L, DT, 2>(xq, xs, rf, ws, qw, sc, ecol, bias, y, S, E, N, K, xpp, max_tiles, st);
        else mx_grouped_gemm_launch_t<L, DT, 1>(xq, xs, rf, ws, qw, sc, ecol, bias, y, S, E, N, K, xpp, max_tiles, st);
    } else {
        mx_grouped_gemm_launch_t<L, DT, L::wn>(xq, xs, rf, ws, qw, sc, ecol, bias, y, S, E, N, K, xpp, max_tiles, st);
    }
}

// The contraction from quantised activations.  form 0: the routed kernel reading xq from memory (no workspace); form 1: routing into the
// workspace (the routing region alone), then the grouped GEMM.
template <class L>
int mx_grouped_gemm_launch(const uint8_t* xq, const uint8_t* xs, const uint8_t* rf, const int32_t* idx, const uint8_t* qw, const uint8_t* sc,
                           const uint8_t* ecol, const void* bias, void* y, void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype,
                           int form, hipStream_t st) {
    const long P = T * S;
    if (form == 0) {
        if (dtype == BIE_F16) return mx_grouped_decode_launch<L, BIE_F16, false>(xq, xs, rf, idx, qw, sc, ecol, bias, y, P, S, E, N, K, x_per_pair, st);
        return mx_grouped_decode_launch<L, BIE_BF16, false>(xq, xs, rf, idx, qw, sc, ecol, bias, y, P, S, E, N, K, x_per_pair, st);
    }
    const int rc = mxfp4_moe_route_launch(idx, workspace, P, E, st);
    if (rc) return rc;
    const int32_t* ws = reinterpret_cast<const int32_t*>(workspace);
    const int max_tiles = (int)mxfp4_moe_max_tiles(P, E);
    if (dtype == BIE_F16) mx_grouped_gemm_launch_dt<L, BIE_F16>(xq, xs, rf, ws, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair, max_tiles, st);
    else mx_grouped_gemm_launch_dt<L, BIE_BF16>(xq, xs, rf, ws, qw, sc, ecol, bias, y, S, E, N, K, x_per_pair, max_tiles, st);
    return check_launch(L::gemm_name);
}

// The whole layer from x.  form 0 with K <= one_k: one launch, the workspace is not touched.
template <class L>
int mx_grouped_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                              void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    const long P = T * S, R = mx_grouped_rows(T, S, x_per_pair);
    if (form == 0 && K <= L::one_k) {
        if (dtype == BIE_F16) return mx_grouped_decode_launch<L, BIE_F16, true>(x, nullptr, nullptr, idx, qw, sc, ecol, bias, y, P, S, E, N, K, x_per_pair, st);
        return mx_grouped_decode_launch<L, BIE_BF16, true>(x, nullptr, nullptr, idx, qw, sc, ecol, bias, y, P, S, E, N, K, x_per_pair, st);
    }
    uint8_t* xq = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* xs = xq + mx_grouped_xs_offset<L>(R, K);
    uint8_t* rf = xq + mx_grouped_flag_offset<L>(R, K);
    const int rc = L::act::quantize(x, xq, xs, rf, R, K, dtype, st);
    if (rc) return rc;
    return mx_grouped_gemm_launch<L>(xq, xs, rf, idx, qw, sc, ecol, bias, y, xq + mx_grouped_route_offset<L>(R, K), T, S, E, N, K, x_per_pair, dtype, form, st);
}

}  // namespace bie
