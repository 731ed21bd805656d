// The host side of the weight-only MX layers (MXFP4 and MXFP6 weights against fp16 / bf16 activations), written once: the plan and the
// launchers of the linear layers (mxfp4.hip, mxfp6.hip), the expert layers (mxfp4_moe.hip, mxfp6_moe.hip) and the input gradients
// (mxfp4_grad.hip, mxfp6_grad.hip).  A .hip file keeps its kernels and measured constants and names them in a small traits type; its
// mxfp*_ symbols are one call each of the templates below.  The arrangement, and why a knob's name reaches BIE_KNOB as a static member
// of the layer's type (every layer keeps its own once-per-process cache), are those of mx_scaled_launch.cuh.
#pragma once
#include "mxfp4_common.cuh"  // MX_BM, MX_BN: the prefill tile

namespace bie {

// mxfp4_moe.hip: the routing of the grouped forms
long mxfp4_moe_max_tiles(long P, long E);
int mxfp4_moe_route_launch(const int32_t* idx, void* workspace, long P, long E, hipStream_t st);

// ---- linear layers ------------------------------------------------------------------------------------------------------------------------
// A linear layer L states: form_knob; decode_rows, plan_rows (the decode form exists for M <= decode_rows, the plan takes it for
// M <= plan_rows); decode_name, gemm_name (for check_launch); decode<DT>(...), the decode launch; gemm<DT>(), the MX_BM x MX_BN tile kernel.
template <class L>
bool mx_w16_decode_ok(long M) { return M >= 1 && M <= L::decode_rows; }

template <class L>
int mx_w16_form(long M) {
    const int f = BIE_KNOB(L::form_knob, -1);
    if (f == 0 && M <= L::decode_rows) return 0;
    if (f == 1) return 1;
    return M <= L::plan_rows ? 0 : 1;
}

template <class L, int DT>
static void mx_w16_forward_dt(const uint16_t* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, long M, long N, long K,
                              int form, hipStream_t st) {
    if (form == 0) return L::template decode<DT>(x, qw, sc, bias, y, (int)M, (int)N, (int)K, st);
    const int tn = (int)cdivl(N, MX_BN);
    const dim3 grid((unsigned)(cdivl(M, MX_BM) * tn));
    hipLaunchKernelGGL((L::template gemm<DT>()), grid, dim3(256), 0, st, x, qw, sc, ecol, bias, y, (int)M, (int)N, (int)K, tn);
}

template <class L>
int mx_w16_forward_launch(const void* x, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y, long M, long N, long K,
                          int dtype, int form, hipStream_t st) {
    const uint16_t* xs = reinterpret_cast<const uint16_t*>(x);
    if (dtype == BIE_F16) mx_w16_forward_dt<L, BIE_F16>(xs, qw, sc, ecol, bias, y, M, N, K, form, st);
    else mx_w16_forward_dt<L, BIE_BF16>(xs, qw, sc, ecol, bias, y, M, N, K, form, st);
    return check_launch(form == 0 ? L::decode_name : L::gemm_name);
}

// ---- expert layers ------------------------------------------------------------------------------------------------------------------------
// An expert layer L states: form_knob; decode_pairs (the routed decode form exists for P <= decode_pairs, its grid's second dimension);
// plan_pairs, plan_pairs_sparse (the plan takes the decode form for P <= plan_pairs, and up to plan_pairs_sparse while P <= 2 E);
// decode_name, gemm_name; decode<DT>(...); gemm<DT>(), the grouped kernel on the routing's row tiles and MX_BN columns.
template <class L>
bool mx_w16_moe_decode_ok(long P) { return P >= 1 && P <= L::decode_pairs; }

template <class L>
int mx_w16_moe_form(long P, long E) {
    const int f = BIE_KNOB(L::form_knob, -1);
    if (f == 0 && P <= L::decode_pairs) return 0;
    if (f == 1) return 1;
    return (P <= L::plan_pairs || (P <= L::plan_pairs_sparse && P <= 2 * E)) ? 0 : 1;
}

// form 0: the routed decode kernel, no workspace; form 1: routing into the workspace, then the grouped GEMM.
template <class L>
int mx_w16_moe_forward_launch(const void* x, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* ecol, const void* bias, void* y,
                              void* workspace, long T, long S, long E, long N, long K, int x_per_pair, int dtype, int form, hipStream_t st) {
    const uint16_t* xs = reinterpret_cast<const uint16_t*>(x);
    const long P = T * S;
    if (form == 0) {
        if (dtype == BIE_F16) L::template decode<BIE_F16>(xs, idx, qw, sc, bias, y, (int)P, (int)S, (int)E, (int)N, (int)K, x_per_pair, st);
        else L::template decode<BIE_BF16>(xs, idx, qw, sc, bias, y, (int)P, (int)S, (int)E, (int)N, (int)K, x_per_pair, st);
        return check_launch(L::decode_name);
    }
    const int32_t* ws = reinterpret_cast<const int32_t*>(workspace);
    const int max_tiles = (int)mxfp4_moe_max_tiles(P, E);
    const int rc = mxfp4_moe_route_launch(idx, workspace, P, E, st);
    if (rc) return rc;
    const dim3 grid((unsigned)(max_tiles * cdivl(N, MX_BN)));
    if (dtype == BIE_F16)
        hipLaunchKernelGGL((L::template gemm<BIE_F16>()), grid, dim3(256), 0, st, xs, ws, qw, sc, ecol, bias, y, (int)S, (int)E, (int)N, (int)K, x_per_pair, max_tiles);
    else
        hipLaunchKernelGGL((L::template gemm<BIE_BF16>()), grid, dim3(256), 0, st, xs, ws, qw, sc, ecol, bias, y, (int)S, (int)E, (int)N, (int)K, x_per_pair, max_tiles);
    return check_launch(L::gemm_name);
}

// ---- input gradients ------------------------------------------------------------------------------------------------------------------------
// A gradient unit L states: BM, BK (the tile of gx); dense_name, grouped_name; dense<DT>() and grouped<DT, ODT>(), the kernels.
// gy rows in whole 16-byte pieces where every row starts on one
static inline int dgrad_vec(const void* gy, long N) { return (N % 8 == 0 && reinterpret_cast<uintptr_t>(gy) % 16 == 0) ? 1 : 0; }

template <class L>
int mx_w16_grad_input_launch(const void* gy, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, long M, long N, long K, int dtype,
                             hipStream_t st) {
    const uint16_t* g = reinterpret_cast<const uint16_t*>(gy);
    const int tk = (int)cdivl(K, L::BK), vec = dgrad_vec(gy, N);
    const dim3 grid((unsigned)(cdivl(M, L::BM) * tk));
    if (dtype == BIE_F16) hipLaunchKernelGGL((L::template dense<BIE_F16>()), grid, dim3(256), 0, st, g, qw, sc, eblk, gx, (int)M, (int)N, (int)K, tk, vec);
    else hipLaunchKernelGGL((L::template dense<BIE_BF16>()), grid, dim3(256), 0, st, g, qw, sc, eblk, gx, (int)M, (int)N, (int)K, tk, vec);
    return check_launch(L::dense_name);
}

template <class L, int DT, int ODT>
static void mx_w16_moe_grad_input_t(const uint16_t* g, const int32_t* ws, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, long E, long N,
                                    long K, int vec, int max_tiles, hipStream_t st) {
    const dim3 grid((unsigned)(max_tiles * cdivl(K, L::BK)));
    hipLaunchKernelGGL((L::template grouped<DT, ODT>()), grid, dim3(256), 0, st, g, ws, qw, sc, eblk, gx, (int)E, (int)N, (int)K, vec, max_tiles);
}

template <class L>
int mx_w16_moe_grad_input_launch(const void* gy, const int32_t* idx, const uint8_t* qw, const uint8_t* sc, const uint8_t* eblk, void* gx, void* workspace,
                                 long P, long E, long N, long K, int dtype, int out_fp32, hipStream_t st) {
    const uint16_t* g = reinterpret_cast<const uint16_t*>(gy);
    const int32_t* ws = reinterpret_cast<const int32_t*>(workspace);
    const int max_tiles = (int)mxfp4_moe_max_tiles(P, E), vec = dgrad_vec(gy, N);
    const int rc = mxfp4_moe_route_launch(idx, workspace, P, E, st);
    if (rc) return rc;
    if (dtype == BIE_F16) {
        if (out_fp32) mx_w16_moe_grad_input_t<L, BIE_F16, BIE_F32>(g, ws, qw, sc, eblk, gx, E, N, K, vec, max_tiles, st);
        else mx_w16_moe_grad_input_t<L, BIE_F16, BIE_F16>(g, ws, qw, sc, eblk, gx, E, N, K, vec, max_tiles, st);
    } else {
        if (out_fp32) mx_w16_moe_grad_input_t<L, BIE_BF16, BIE_F32>(g, ws, qw, sc, eblk, gx, E, N, K, vec, max_tiles, st);
        else mx_w16_moe_grad_input_t<L, BIE_BF16, BIE_BF16>(g, ws, qw, sc, eblk, gx, E, N, K, vec, max_tiles, st);
    }
    return check_launch(L::grouped_name);
}

}  // namespace bie
