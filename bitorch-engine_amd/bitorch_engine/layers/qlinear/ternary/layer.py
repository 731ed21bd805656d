"""Ternary (TWN) weight / binary activation linear: the base type and the ternarisation rule.  There is no reference implementation;
the semantics are this library's own ("Ternary linear layer")."""
import math

import torch
from torch import nn


def ternarize(weight: torch.Tensor, threshold_factor: float = 0.7):
    """TWN (Li & Liu 2016) per output row n, in fp32:  delta_n = threshold_factor * mean_k |W[n, k]|;  t = +1 where W > delta_n,
    -1 where W < -delta_n, else 0;  alpha_n = mean |W[n, k]| over the non-zero positions (0 for a row without any).
    -> (trits int8 [N, K], alpha fp32 [N], delta fp32 [N])."""
    w = weight.detach().float()
    a = w.abs()
    delta = threshold_factor * a.mean(dim=1)
    d = delta[:, None]
    t = (w > d).to(torch.int8) - (w < -d).to(torch.int8)
    nz = t != 0
    cnt = nz.sum(dim=1)
    alpha = torch.where(nz, a, torch.zeros_like(a)).sum(dim=1) / cnt.clamp(min=1).float()
    return t, alpha, delta


def ternarize_absmean(weight: torch.Tensor):
    """BitNet b1.58 absmean rule, per tensor, in fp32:  beta = max(mean |W|, 1e-5);  t = clamp(rint(W / beta), -1, 1);  alpha_n = beta for
    every row n.  -> (trits int8 [N, K], alpha fp32 [N])."""
    w = weight.detach().float()
    beta = w.abs().mean().clamp(min=1e-5)
    t = torch.round(w / beta).clamp(-1, 1).to(torch.int8)
    return t, beta.expand(w.shape[0]).clone()


class TernaryWeightState:
    """The weight-state contract shared by the ternary layers (TernaryLinearBase, qconv's TernaryConv2dBase): a float latent `weight`, the
    packed trits `qweight` and their per-output-channel scale `scale_w` (buffers), `bias_a` and `scale_a`.  A qweight-only checkpoint
    carries no `weight`; loading one drops the latent weight, and loading a latent weight re-derives qweight before the next packed
    forward.  Mixed in front of nn.Module; the layer sets `_packed` (qweight / scale_w hold the current weight)."""

    def generate_quantized_weight(self, qweight_only: bool = False) -> None:
        """Ternarise `weight` into qweight / scale_w; qweight_only: drop the float latent weight afterwards (a packed checkpoint)."""
        self.prepare_params()
        if qweight_only:
            self.weight = None

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # a qweight-only checkpoint carries no latent weight (and a latent weight may come into a layer that had dropped its own)
        if prefix + "weight" in state_dict:
            if self.weight is None:  # on the layer's device, whatever device the checkpoint tensor is on
                self.weight = nn.Parameter(torch.empty(state_dict[prefix + "weight"].shape, dtype=self.dtype, device=self._state_device()))
        elif self.weight is not None and prefix + "qweight" in state_dict:
            self.weight = None
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        # with a latent weight, qweight is re-derived from it before the next packed forward
        self._packed = self.weight is None

    def _state_device(self) -> torch.device:
        """The device the layer's tensors live on (a re-created latent weight goes there)."""
        return self.bias_a.device

    def _init_scale_a(self, x: torch.Tensor) -> None:
        # lazily initialised activation scale (2 * mean|x|, 4 * when not symmetric); the nonzero answer is remembered per version of the parameter
        from bitorch_engine.extensions.q_linear_cuda import _cached
        if not _cached(self.scale_a, "nonzero", lambda: bool(self.scale_a.is_nonzero())):
            self.scale_a.data = ((2 if self.symmetric else 4) * x.abs().mean()).to(self.dtype)


class TernaryLinearBase(TernaryWeightState, nn.Module):
    """Float latent `weight` [N, K] (kept while training; dropped by generate_quantized_weight(qweight_only=True) or set_ternary_weight),
    the packed trits `qweight` uint8 [2, N, K/8] and their per-row scale `scale_w` [N] (buffers), the learnable activation bias `bias_a` [K]
    and scale `scale_a` (initialised on the first forward to 2 * mean|x|, 4 * when not symmetric)."""

    def __init__(self, input_features: int, out_features: int, device: torch.device = None, dtype: torch.dtype = torch.float,
                 symmetric: bool = True, threshold_factor: float = 0.7) -> None:
        super().__init__()
        if input_features % 32 or input_features <= 0 or out_features <= 0:
            raise ValueError(f"ternary linear needs input_features % 32 == 0 and out_features >= 1 (got {input_features}, {out_features})")
        self.input_features, self.output_features = input_features, out_features
        self.device, self.dtype, self.symmetric, self.threshold_factor = device, dtype, symmetric, threshold_factor
        w = torch.empty((out_features, input_features), dtype=dtype, device=device)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.weight = nn.Parameter(w)
        self.bias_a = nn.Parameter(torch.zeros(input_features, dtype=dtype, device=device))
        self.scale_a = nn.Parameter(torch.tensor(0, dtype=dtype, device=device))
        self.register_buffer("qweight", torch.zeros((2, out_features, input_features // 8), dtype=torch.uint8, device=device))
        self.register_buffer("scale_w", torch.zeros(out_features, dtype=dtype, device=device))
        self._packed = False  # qweight / scale_w hold the current weight (or a loaded / set ternary weight)

    def prepare_params(self) -> None:
        raise NotImplementedError("Subclasses should implement this method.")

    def _check_forward(self, x: torch.Tensor) -> None:
        assert x.size(-1) == self.input_features, f"Weight and input tensor mismatch: {x.size(-1)} != {self.input_features}"
        assert x.dtype == self.dtype, f"dtype mismatch. Expected: '{self.dtype}', but '{x.dtype}' found"
