"""What the three weight-only MX linear layers (MXFP4LinearCuda, MXFP6LinearCuda, MXFP8LinearCuda) share about the gradient of their
float latent weight: the attribute grad_weight and the backward's grad_weight / grad_bias pair.

  grad_weight = "torch" (the default): gy^T . x and sum_m gy in fp32 torch, cast to the dtype, as before the attribute existed
  grad_weight = "kernel":              both from one call of extensions/mx_grad_weight_cuda.grad_weight (csrc/mx_wgrad.hip)

The attribute is a property of the object only: not a constructor argument, not saved, independent of grad_input."""
from bitorch_engine.utils.safe_import import import_extension

mx_grad_weight_cuda = import_extension("mx_grad_weight_cuda")


class GradWeightChoice:
    _grad_weight = "torch"

    @property
    def grad_weight(self) -> str:
        return self._grad_weight

    @grad_weight.setter
    def grad_weight(self, value: str) -> None:
        if value not in ("torch", "kernel"):
            raise ValueError(f'grad_weight must be "torch" or "kernel" (got {value!r})')
        self._grad_weight = value


def weight_grads(gy, x, need_w: bool, need_b: bool, kernel: bool):
    """(grad_weight, grad_bias) of a backward call, None where not needed.  With kernel=True gb is written only when need_b is set; a
    call that needs the bias gradient alone stays in torch (there is no product in it)."""
    grad_w = grad_b = None
    if kernel and need_w:
        if need_b:
            grad_w, grad_b = mx_grad_weight_cuda.grad_weight(gy, x, bias=True)
        else:
            grad_w = mx_grad_weight_cuda.grad_weight(gy, x)
        return grad_w, grad_b
    if need_w:
        grad_w = gy.float().t().mm(x.float()).to(gy.dtype)
    if need_b:
        grad_b = gy.float().sum(0).to(gy.dtype)
    return grad_w, grad_b
