#!/usr/bin/env python
"""One SHA-256 of y's bytes per case for the four MXFP4 layers (weight-only and W4A4, linear and experts), every form forced: two builds
of the library compute the same bits exactly when their listings are equal line for line.

  python tools/mxfp4_digest.py > new.txt;  BIE_HIP_LIB=/path/to/other/libbie_hip.so python tools/mxfp4_digest.py > old.txt;  diff old.txt new.txt

Every input comes from numpy.random.default_rng(seed) on the host, so both runs see the same bytes.  Cases: fp16 and bf16, bias on and
off; the linear layers at M in {1, 16, 17, 64, 65, 300} on 96 -> 130 and 2880 -> 2880; the expert layers with x per token and per pair
at E = 3, S = 4, 96 -> 33 (T in {1, 17, 300}) and E = 32, S = 4, 2880 -> 2880 (T in {16, 300})."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bitorch-engine_amd"))
DEV = "cuda"
DTS = ((torch.float16, "f16"), (torch.bfloat16, "bf16"))
DENSE = ((96, 130), (2880, 2880))
DENSE_M = (1, 16, 17, 64, 65, 300)
EXPERTS = ((3, 4, 96, 33, (1, 17, 300)), (32, 4, 2880, 2880, (16, 300)))


def sha(y):
    torch.cuda.synchronize()
    return hashlib.sha256(y.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def weights(rng, rows, K):
    q = torch.from_numpy(rng.integers(0, 256, (rows, K // 2), dtype=np.uint8)).to(DEV)
    s = torch.from_numpy(rng.integers(118, 131, (rows, K // 32), dtype=np.uint8)).to(DEV)
    return q, s


def normal(rng, shape, dt):
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dt).to(DEV)


def main():
    from bitorch_engine.extensions import mxfp4_a4_linear_cuda as a4, mxfp4_experts_a4_cuda as ma4, mxfp4_experts_cuda as moe, mxfp4_linear_cuda as mx
    for K, N in DENSE:
        rng = np.random.default_rng(1000 + K + N)
        q, s = weights(rng, N, K)
        e_col = mx.col_exp(s)
        for dt, dname in DTS:
            bias = normal(rng, (N,), dt)
            for M in DENSE_M:
                x = normal(rng, (M, K), dt)
                for b, bname in ((None, "nobias"), (bias, "bias")):
                    for layer, name in ((mx, "linear"), (a4, "linear_a4")):
                        for form in (0, 1):
                            if form == 0 and M > (16 if layer is mx else 64):
                                continue  # the decode form does not exist at this M
                            print(f"{name} {dname} {bname} K={K} N={N} M={M} form={form} {sha(layer.forward(x, q, s, b, e_col, form=form))}")
    for E, S, K, N, Ts in EXPERTS:
        rng = np.random.default_rng(2000 + E + K + N)
        q, s = weights(rng, E * N, K)
        q, s = q.reshape(E, N, K // 2), s.reshape(E, N, K // 32)
        e_col = moe.col_exp(s)
        for dt, dname in DTS:
            bias = normal(rng, (E, N), dt)
            for T in Ts:
                idx = torch.from_numpy(rng.integers(-1, E + 1, (T, S)).astype(np.int32)).to(DEV)  # -1 and E: skipped slots
                xs = {0: normal(rng, (T, K), dt), 1: normal(rng, (T, S, K), dt)}
                for xpp in (0, 1):
                    for b, bname in ((None, "nobias"), (bias, "bias")):
                        for layer, name in ((moe, "experts"), (ma4, "experts_a4")):
                            for form in (0, 1):
                                if form == 0 and T * S > 1024:
                                    continue  # the routed decode form does not exist at this P
                                y = layer.forward(xs[xpp], idx, q, s, b, e_col, form=form)
                                print(f"{name} {dname} {bname} E={E} S={S} K={K} N={N} T={T} xpp={xpp} form={form} {sha(y)}")


if __name__ == "__main__":
    main()
