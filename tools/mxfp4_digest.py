#!/usr/bin/env python
"""One SHA-256 of y's bytes per case for the MX layers, every form forced: the weight-only MXFP4 and MXFP6 layers and every layer on the shared
block-scaled tile (mx_scaled_gemm_tile: W4A4, W4A6, W4A8, W6A6, W6A8, W8A8 linear; W4A4, W4A6, W4A8, W6A6, W6A8 experts), whose decode
forms are on mx_scaled_decode_rows / mx_scaled_decode_pair or on bodies of their own.  Two builds of the library compute the same bits exactly when their listings are
equal line for line.

  python tools/mxfp4_digest.py > new.txt;  BIE_HIP_LIB=/path/to/other/libbie_hip.so python tools/mxfp4_digest.py > old.txt;  diff old.txt new.txt

Every input comes from numpy.random.default_rng(seed) on the host, so both runs see the same bytes.  Cases: fp16 and bf16, bias on and
off; the linear layers at M in {1, 16, 17, 33, 64, 65, 300} on 96 -> 130 and 2880 -> 2880 (M = 33: the 64-row decode instance with
three 16-row groups partly or wholly dead), and at M = 257 on 160 -> 21846 (the 128 x 128 tile instance with ragged M, N and K); the
expert layers with x per token and per pair at E = 3, S = 4, 96 -> 33 (T in {1, 17, 300}) and E = 32, S = 4, 2880 -> 2880 (T in
{16, 300}), and the two grouped A6 layers once more at E = 3, T = 300 under each value of their tile width knob (BIE_MXFP4_MOE_A6_WN,
BIE_MXFP6_MOE_A6_WN); the five expert A-layers' gemm entry at form 0 on the outputs of their quantize_act (the routed kernel that reads
xq from memory, which forward never runs at these K) at E = 3, T in {1, 17}, and forward and gemm at T = 17 under each strip width
of the three layers that have the knob (BIE_MXFP4_MOE_A4_STRIP, BIE_MXFP4_MOE_A8_STRIP, BIE_MXFP6_MOE_A8_STRIP = 1, 2, 4).  Last, on
streams of their own, gx of the four input-gradient entries (MXFP4 and MXFP6): dense at M in {1, 129, 300} on 96 -> 33 (N % 8 != 0: the
guarded 16-bit loads of gy) and 2880 -> 2880 (whole 16-byte pieces), grouped at E = 3, S = 4, T in {1, 17, 300} on both shapes with gx
in the dtype and in fp32."""
import hashlib
import importlib
import os
import sys

os.environ["BIE_TUNING"] = "1"  # read once, at the library's first call: the tile width knobs are then re-read on every call

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
DEV = "cuda"
DTS = ((torch.float16, "f16"), (torch.bfloat16, "bf16"))
DENSE = ((96, 130), (2880, 2880))
DENSE_M = (1, 16, 17, 33, 64, 65, 300)
# One stream per (K, N) feeds the weights, each dtype's bias and the x of every M in turn, so a new M drawn from it would shift every
# later draw and change the lines already recorded in profiles/.  An M added after the first listing therefore goes here as well as in
# DENSE_M, and draws its x from a stream seeded by (K, N, M) alone.
DENSE_M_OWN = (33,)
DENSE_TILE128 = (257, 160, 21846)  # M, K, N
EXPERTS = ((3, 4, 96, 33, (1, 17, 300)), (32, 4, 2880, 2880, (16, 300)))
# (extension, name in the listing, bits per weight code, largest M of the decode form)
LINEAR = (("mxfp4_linear_cuda", "linear", 4, 16), ("mxfp4_a4_linear_cuda", "linear_a4", 4, 64), ("mxfp4_a6_linear_cuda", "linear_a6", 4, 64),
          ("mxfp4_a8_linear_cuda", "linear_a8", 4, 64), ("mxfp6_a6_linear_cuda", "linear_w6a6", 6, 64), ("mxfp6_a8_linear_cuda", "linear_w6a8", 6, 64),
          ("mxfp8_a8_linear_cuda", "linear_w8a8", 8, 64), ("mxfp6_linear_cuda", "linear_w6", 6, 32))
# (extension, name in the listing, bits per weight code, tile width knob or None)
GROUPED = (("mxfp4_experts_cuda", "experts", 4, None), ("mxfp4_experts_a4_cuda", "experts_a4", 4, None),
           ("mxfp4_experts_a6_cuda", "experts_a6", 4, "BIE_MXFP4_MOE_A6_WN"), ("mxfp4_experts_a8_cuda", "experts_a8", 4, None),
           ("mxfp6_experts_a6_cuda", "experts_w6a6", 6, "BIE_MXFP6_MOE_A6_WN"), ("mxfp6_experts_a8_cuda", "experts_w6a8", 6, None),
           ("mxfp6_experts_cuda", "experts_w6", 6, None))
GRAD = ((96, 33), (2880, 2880))  # K, N
GRAD_M = (1, 129, 300)
GRAD_T = (1, 17, 300)
ROUTED_T = (1, 17)  # the gemm entry at form 0, at EXPERTS[0]'s shape
# the strip width knob of the routed decode form, for the layers that have one
STRIP = {"experts_a4": "BIE_MXFP4_MOE_A4_STRIP", "experts_a8": "BIE_MXFP4_MOE_A8_STRIP", "experts_w6a8": "BIE_MXFP6_MOE_A8_STRIP"}


def ext(name):
    return importlib.import_module("bitorch_engine.extensions." + name)


def sha(y):
    torch.cuda.synchronize()
    return hashlib.sha256(y.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def codes(rng, rows, K, bits):
    """rows x (K * bits / 8) random code bytes; no E4M3 NaN code (0x7f, 0xff), which would hide a whole row of y"""
    q = rng.integers(0, 256, (rows, K * bits // 8), dtype=np.uint8)
    if bits == 8:
        q[(q & 0x7F) == 0x7F] -= 1
    return torch.from_numpy(q).to(DEV)


def weights(rng, rows, K):
    q = codes(rng, rows, K, 4)
    s = torch.from_numpy(rng.integers(118, 131, (rows, K // 32), dtype=np.uint8)).to(DEV)
    return q, s


def normal(rng, shape, dt):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dt).to(DEV)


def dense(K, N, Ms):
    rng = np.random.default_rng(1000 + K + N)
    q4, s = weights(rng, N, K)
    rng_w = np.random.default_rng(3000 + K + N)  # the wider codes from a stream of their own: the draws above stay as they were
    q = {4: q4, 6: codes(rng_w, N, K, 6), 8: codes(rng_w, N, K, 8)}
    e_col = ext("mxfp4_linear_cuda").col_exp(s)
    for dt, dname in DTS:
        bias = normal(rng, (N,), dt)
        for M in Ms:
            # an M of DENSE_M_OWN must not draw from rng (see there); DENSE_TILE128's M is drawn from rng as it always was
            x = normal(np.random.default_rng(5000 + K + N + M) if M in DENSE_M_OWN else rng, (M, K), dt)
            for b, bname in ((None, "nobias"), (bias, "bias")):
                for mod, name, bits, decode_rows in LINEAR:
                    for form in (0, 1):
                        if form == 0 and M > decode_rows:
                            continue  # the decode form does not exist at this M
                        print(f"{name} {dname} {bname} K={K} N={N} M={M} form={form} {sha(ext(mod).forward(x, q[bits], s, b, e_col, form=form))}")


def grouped(E, S, K, N, Ts, knob_value=None):
    rng = np.random.default_rng(2000 + E + K + N)
    q4, s = weights(rng, E * N, K)
    q = {4: q4.reshape(E, N, K // 2), 6: codes(np.random.default_rng(4000 + E + K + N), E * N, K, 6).reshape(E, N, K // 32 * 24)}
    s = s.reshape(E, N, K // 32)
    e_col = ext("mxfp4_experts_cuda").col_exp(s)
    for dt, dname in DTS:
        bias = normal(rng, (E, N), dt)
        for T in Ts:
            idx = torch.from_numpy(rng.integers(-1, E + 1, (T, S)).astype(np.int32)).to(DEV)  # -1 and E: skipped slots
            xs = {0: normal(rng, (T, K), dt), 1: normal(rng, (T, S, K), dt)}
            for xpp in (0, 1):
                for b, bname in ((None, "nobias"), (bias, "bias")):
                    for mod, name, bits, knob in GROUPED:
                        if knob_value is not None:
                            if knob is None:
                                continue
                            os.environ[knob] = str(knob_value)
                            name = f"{name} wn={knob_value}"
                        for form in (0, 1):
                            if form == 0 and (T * S > 1024 or knob_value is not None):
                                continue  # the routed decode form does not exist at this P; the knob is the grouped form's
                            y = ext(mod).forward(xs[xpp], idx, q[bits], s, b, e_col, form=form)
                            print(f"{name} {dname} {bname} E={E} S={S} K={K} N={N} T={T} xpp={xpp} form={form} {sha(y)}")
                        if knob_value is not None:
                            del os.environ[knob]


def routed(E, S, K, N, Ts):
    """The routed decode kernels that read quantised rows from memory (gemm at form 0), then forward and gemm under every strip width."""
    rng = np.random.default_rng(6000 + E + K + N)
    q4, s = weights(rng, E * N, K)
    q = {4: q4.reshape(E, N, K // 2), 6: codes(rng, E * N, K, 6).reshape(E, N, K // 32 * 24)}
    s = s.reshape(E, N, K // 32)
    e_col = ext("mxfp4_experts_cuda").col_exp(s)
    for dt, dname in DTS:
        bias = normal(rng, (E, N), dt)
        for T in Ts:
            idx = torch.from_numpy(rng.integers(-1, E + 1, (T, S)).astype(np.int32)).to(DEV)  # -1 and E: skipped slots
            xs = {0: normal(rng, (T, K), dt), 1: normal(rng, (T, S, K), dt)}
            for xpp in (0, 1):
                for b, bname in ((None, "nobias"), (bias, "bias")):
                    for mod, name, bits, _ in GROUPED[1:]:
                        m = ext(mod)
                        if not hasattr(m, "gemm"):
                            continue  # a weight-only layer: no quantised activations
                        xq = m.quantize_act(xs[xpp].reshape(-1, K))
                        tail = f"{dname} {bname} E={E} S={S} K={K} N={N} T={T} xpp={xpp} form=0"
                        print(f"{name} gemm {tail} {sha(m.gemm(*xq, idx, q[bits], s, b, e_col, dtype=dt, form=0))}")
                        if name in STRIP and T == Ts[-1]:
                            for strip in (1, 2, 4):
                                os.environ[STRIP[name]] = str(strip)
                                print(f"{name} strip={strip} forward {tail} {sha(m.forward(xs[xpp], idx, q[bits], s, b, e_col, form=0))}")
                                print(f"{name} strip={strip} gemm {tail} {sha(m.gemm(*xq, idx, q[bits], s, b, e_col, dtype=dt, form=0))}")
                            del os.environ[STRIP[name]]


def sha_any(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()  # gx in the dtype or in fp32


def grads(K, N):
    """The four input-gradient entries; every draw from streams seeded here alone."""
    E, S = 3, 4
    rng = np.random.default_rng(7000 + K + N)
    q = {4: codes(rng, E * N, K, 4), 6: codes(rng, E * N, K, 6)}
    s = torch.from_numpy(rng.integers(118, 131, (E * N, K // 32), dtype=np.uint8)).to(DEV)
    for dt, dname in DTS:
        for M in GRAD_M:
            gy = normal(rng, (M, N), dt)
            for fmt, bits in (("mxfp4", 4), ("mxfp6", 6)):
                gx = ext(fmt + "_linear_cuda").grad_input(gy, q[bits][:N], s[:N])
                print(f"grad_{fmt} {dname} K={K} N={N} M={M} {sha(gx)}")
        for T in GRAD_T:
            idx = torch.from_numpy(rng.integers(-1, E + 1, (T, S)).astype(np.int32)).to(DEV)  # -1 and E: skipped slots
            gy = normal(rng, (T, S, N), dt)
            for fmt, bits in (("mxfp4", 4), ("mxfp6", 6)):
                for odt, oname in ((None, "dtype"), (torch.float32, "fp32")):
                    gx = ext(fmt + "_experts_cuda").grad_input(gy, idx, q[bits].reshape(E, N, -1), s.reshape(E, N, -1), out_dtype=odt)
                    print(f"grad_experts_{fmt} {dname} gx={oname} E={E} S={S} K={K} N={N} T={T} {sha_any(gx)}")


def main():
    for K, N in DENSE:
        dense(K, N, DENSE_M)
    for E, S, K, N, Ts in EXPERTS:
        grouped(E, S, K, N, Ts)
    M, K, N = DENSE_TILE128
    dense(K, N, (M,))
    E, S, K, N, Ts = EXPERTS[0]
    for wn in (1, 2):
        grouped(E, S, K, N, Ts[-1:], knob_value=wn)
    routed(E, S, K, N, ROUTED_T)
    for K, N in GRAD:
        grads(K, N)


if __name__ == "__main__":
    main()
