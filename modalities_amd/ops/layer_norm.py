"""LayerNorm fwd/bwd (K5). HIP kernel: csrc/layer_norm.hip (register-resident
rows, bf16x8 loads, deterministic two-phase weight/bias-gradient reduce).
Replaces torch's nn.LayerNorm kernels for the layer_norm norm variant
(reference: src/modalities/models/components/layer_norms.py, used
gpt2_model.py:923-930) and for the ViT / CoCa norms."""

from typing import Optional

import torch
import torch.nn.functional as F

from modalities_amd.ops.backend import use_hip, hip_ext


def _aligned(t):
    """The kernels read rows with 16-byte loads. A contiguous view can start
    at an odd element offset (a flat slice, a parameter view in a flat
    buffer); such a tensor is copied to a fresh, aligned allocation."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _LayerNormHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        shape = x.shape
        x2d = _aligned(x.contiguous().view(-1, shape[-1]))
        weight = _aligned(weight.contiguous())
        bias = None if bias is None else _aligned(bias.contiguous())
        y, mean, rstd = hip_ext().layernorm_fwd(x2d, weight, bias, eps)
        ctx.save_for_backward(x2d, weight, mean, rstd)
        ctx.shape = shape
        ctx.has_bias = bias is not None
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, mean, rstd = ctx.saved_tensors
        dx, dw, db = hip_ext().layernorm_bwd(
            _aligned(dy.contiguous().view_as(x2d)), x2d, weight, mean, rstd,
            ctx.has_bias)
        return (dx.view(ctx.shape), dw.to(weight.dtype),
                db.to(weight.dtype) if ctx.has_bias else None, None)


def _hip_eligible(x, weight, bias) -> bool:
    """The kernels cover bf16 rows with H % 8 == 0, H up to the extension's
    layernorm_max_h(), outside autocast; every other dtype/shape keeps
    torch's layer_norm."""
    H = x.shape[-1] if x.dim() >= 1 else 0
    if x.numel() == 0 or H % 8 != 0 or H > hip_ext().layernorm_max_h():
        return False
    if weight is None or weight.dim() != 1 or weight.numel() != H:
        return False
    if bias is not None and (bias.dim() != 1 or bias.numel() != H):
        return False
    if any(t.dtype != torch.bfloat16
           for t in (x, weight, bias) if t is not None):
        return False
    return not torch.is_autocast_enabled(x.device.type)


def layer_norm(x: torch.Tensor, weight: torch.Tensor,
               bias: Optional[torch.Tensor] = None,
               eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm over the last dimension."""
    if use_hip(x, weight, bias) and _hip_eligible(x, weight, bias):
        return _LayerNormHip.apply(x, weight, bias, eps)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class LayerNorm(torch.nn.Module):
    """Drop-in for nn.LayerNorm(normalized_shape: int, eps, bias=...) backed
    by the HIP kernel for bf16 on device; same parameter names, so state
    dicts interchange."""

    def __init__(self, normalized_shape: int, eps: float = 1e-5,
                 bias: bool = True, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.normalized_shape = normalized_shape
        self.weight = torch.nn.Parameter(
            torch.empty(normalized_shape, device=device, dtype=dtype))
        if bias:
            self.bias = torch.nn.Parameter(
                torch.empty(normalized_shape, device=device, dtype=dtype))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return layer_norm(x, self.weight, self.bias, self.eps)

    def extra_repr(self):
        return (f"{self.normalized_shape}, eps={self.eps}, "
                f"bias={self.bias is not None}")
