"""Weight-only FP8 (or bf16) linears for single-token decoding.

A batch-1 decode step is a chain of GEMMs with one to eight activation rows:
their cost is the weight bytes. `skinny_linear` (csrc/decode_gemv.hip)
streams the weight once, straight to registers, for 1 <= M <= 8 rows of x;
`quantize_weight_fp8` halves the bytes it has to stream.

Weight format: OCP e4m3 (`torch.float8_e4m3fn`) codes with one fp32 scale per
output row, and the scale is a power of two:

    scale[n] = 2^ceil(log2(amax_n / 448)),   amax_n = max_k |w[n, k]|
    wq[n, k] = e4m3(clamp(w[n, k] / scale[n], -448, 448))     (nearest even)

so the row's largest value lands in (224, 448] (448 is the largest e4m3
value) and a zero row gets scale 1. A power-of-two scale costs at most one
binade of e4m3's dynamic range per row and leaves the relative precision of
normal values as it is; in exchange `scale[n] * wq[n, k]` is exactly
representable in bf16, so a model carrying the de-quantized weights on the
ordinary bf16 route is an exact reference for the quantized route, up to
accumulation order.

Arithmetic of `skinny_linear`: products and sums in fp32, then `* scale[n]`,
`+ bias[n]`, one rounding to bf16. The CPU route is the same expression in
torch fp32. bf16 weights (`scale=None`) go through the same kernel: the A/B
of the in-tree kernel against hipBLASLt at equal bytes.

`PreparedLinear` / `step_linear` are what the model uses: a prepared copy of
a Linear's weight, and the call that takes it for a single-token step.
"""

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from modalities_amd.ops.backend import hip_ext, use_hip

E4M3_MAX = 448.0
SKINNY_MAX_M = 8
SKINNY_K_MULTIPLE = 16
DECODE_WEIGHT_FORMATS = ("fp8_e4m3", "bf16")


def quantize_weight_fp8(w: torch.Tensor,
                        scale: Optional[torch.Tensor] = None
                        ) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (bf16 or fp32) -> (wq float8_e4m3fn [N, K] contiguous, scale
    fp32 [N]), per-row power-of-two scales (module docstring). An explicit
    `scale` (fp32 [N], positive) replaces the derived one; values beyond
    448 * scale then clamp to +-448. Non-finite weights raise ValueError;
    the NaN codes 0x7F / 0xFF are never produced."""
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError("quantize_weight_fp8: w must be a [N, K] tensor")
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"quantize_weight_fp8: w must be bf16 or fp32, got "
                        f"{w.dtype}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_fp8: w holds non-finite values")
    if scale is None:
        amax = wf.abs().amax(dim=1) if wf.shape[1] > 0 \
            else wf.new_zeros(wf.shape[0])
        # amax / 448 = m * 2^e with m in [0.5, 1): ceil(log2) is e, or e - 1
        # when the ratio is itself a power of two (m == 0.5). Exact, no log.
        m, e = torch.frexp(amax / E4M3_MAX)
        e = torch.where(m == 0.5, e - 1, e)
        scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e),
                            torch.ones_like(amax))
    else:
        if scale.dtype != torch.float32 or tuple(scale.shape) != (w.shape[0],):
            raise ValueError("quantize_weight_fp8: scale must be fp32 [N]")
        if not bool((torch.isfinite(scale) & (scale > 0)).all()):
            raise ValueError("quantize_weight_fp8: scale must be positive "
                             "and finite")
        scale = scale.to(wf.device)
    q = (wf / scale[:, None]).clamp(-E4M3_MAX, E4M3_MAX)
    wq = q.to(torch.float8_e4m3fn).contiguous()
    return wq, scale.contiguous()


def _check_skinny_args(x, w, scale, bias):
    for name, t in (("x", x), ("w", w)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"skinny_linear: {name} must be a tensor")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"skinny_linear: x must be bf16, got {x.dtype}")
    if w.dtype not in (torch.float8_e4m3fn, torch.bfloat16):
        raise TypeError("skinny_linear: w must be float8_e4m3fn or bf16, got "
                        f"{w.dtype}")
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError("skinny_linear: x must be [M, K] and w [N, K], got "
                         f"{tuple(x.shape)} and {tuple(w.shape)}")
    M, K = x.shape
    N = w.shape[0]
    if not 1 <= M <= SKINNY_MAX_M:
        raise ValueError(f"skinny_linear: M must be in [1, {SKINNY_MAX_M}], "
                         f"got {M}")
    if w.shape[1] != K:
        raise ValueError(f"skinny_linear: x has K = {K}, w has K = "
                         f"{w.shape[1]}")
    if K < SKINNY_K_MULTIPLE or K % SKINNY_K_MULTIPLE != 0:
        raise ValueError(f"skinny_linear: K must be a positive multiple of "
                         f"{SKINNY_K_MULTIPLE}, got {K}")
    if N < 1:
        raise ValueError("skinny_linear: w must have at least one row")
    if not w.is_contiguous():
        raise ValueError("skinny_linear: w must be contiguous")
    if x.stride(1) != 1:
        raise ValueError("skinny_linear: x must have unit stride in K")
    if w.device != x.device:
        raise ValueError(f"skinny_linear: w is on {w.device}, x on {x.device}")
    if w.dtype == torch.float8_e4m3fn:
        if not isinstance(scale, torch.Tensor):
            raise TypeError("skinny_linear: e4m3 weights need a scale tensor")
        if scale.dtype != torch.float32:
            raise TypeError(f"skinny_linear: scale must be fp32, got "
                            f"{scale.dtype}")
        if tuple(scale.shape) != (N,) or not scale.is_contiguous():
            raise ValueError(f"skinny_linear: scale must be contiguous [N] = "
                             f"{(N,)}, got {tuple(scale.shape)}")
        if scale.device != x.device:
            raise ValueError(f"skinny_linear: scale is on {scale.device}, x "
                             f"on {x.device}")
    elif scale is not None:
        raise ValueError("skinny_linear: bf16 weights take scale=None")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.bfloat16:
            raise TypeError("skinny_linear: bias must be a bf16 tensor or None")
        if tuple(bias.shape) != (N,) or not bias.is_contiguous():
            raise ValueError(f"skinny_linear: bias must be contiguous [N] = "
                             f"{(N,)}, got {tuple(bias.shape)}")
        if bias.device != x.device:
            raise ValueError(f"skinny_linear: bias is on {bias.device}, x on "
                             f"{x.device}")


def _skinny_linear_ref(x, w, scale, bias):
    acc = x.float() @ w.float().t()
    if scale is not None:
        acc = acc * scale
    if bias is not None:
        acc = acc + bias.float()
    return acc.to(torch.bfloat16)


def skinny_linear(x: torch.Tensor, w: torch.Tensor,
                  scale: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [M, N] bf16 = x [M, K] . w [N, K]^T (* scale[n]) (+ bias[n]).

    x: bf16, 1 <= M <= 8, unit stride in K; rows may be strided (a view into
    a wider buffer). w: contiguous [N, K], float8_e4m3fn with `scale` fp32
    [N], or bf16 with scale None. bias: bf16 [N] or None. K % 16 == 0.
    A row's result does not depend on M or on where the row sits in x.
    Inference only (no autograd)."""
    _check_skinny_args(x, w, scale, bias)
    if use_hip(x, w, scale, bias):
        if (x.shape[0] > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()   # the kernel reads x in 16-byte pieces
        return hip_ext().skinny_linear(x, w, scale, bias)
    return _skinny_linear_ref(x, w, scale, bias)


class PreparedLinear(NamedTuple):
    """Decode-time copy of one Linear: w [N, K] in `fmt`, its scale (e4m3
    only) and the bias in bf16."""
    w: torch.Tensor
    scale: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]


def skinny_eligible(in_features: int) -> bool:
    return in_features >= SKINNY_K_MULTIPLE \
        and in_features % SKINNY_K_MULTIPLE == 0


def prepare_linear(weight: torch.Tensor, bias: Optional[torch.Tensor],
                   fmt: str) -> PreparedLinear:
    if fmt not in DECODE_WEIGHT_FORMATS:
        raise ValueError(f"decode weight format must be one of "
                         f"{DECODE_WEIGHT_FORMATS}, got {fmt!r}")
    w = weight.detach()
    b = None if bias is None else bias.detach().to(torch.bfloat16).contiguous()
    if fmt == "bf16":
        # a bf16 contiguous weight is taken as it is (no second copy)
        return PreparedLinear(w.to(torch.bfloat16).contiguous(), None, b)
    if w.dtype not in (torch.bfloat16, torch.float32):
        w = w.float()
    wq, scale = quantize_weight_fp8(w)
    return PreparedLinear(wq, scale, b)


_ATTR = "_decode_prepared"


def set_prepared(lin: torch.nn.Module, prep: Optional[PreparedLinear]) -> None:
    """Attach (or, with None, drop) the prepared copy of `lin`. It is a plain
    attribute: no parameter, no buffer, not in the state dict."""
    if prep is None:
        lin.__dict__.pop(_ATTR, None)
    else:
        lin.__dict__[_ATTR] = prep


def get_prepared(lin: torch.nn.Module) -> Optional[PreparedLinear]:
    return lin.__dict__.get(_ATTR)


def step_linear(lin: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """`lin(x)` for a single-token step x [B, 1, K]: through `skinny_linear`
    on the prepared weight when `lin` has one, B <= 8 and x is bf16 on the
    weight's device; through the module itself (F.linear on the resident
    weight) otherwise."""
    prep = lin.__dict__.get(_ATTR)
    if prep is None:
        return lin(x)
    rows = x.numel() // x.shape[-1]
    if rows > SKINNY_MAX_M or rows < 1 or x.dtype != torch.bfloat16 \
            or x.device != prep.w.device:
        return F.linear(x, lin.weight, lin.bias)
    x2 = x.reshape(rows, x.shape[-1])
    y = skinny_linear(x2, prep.w, prep.scale, prep.bias)
    return y.view(*x.shape[:-1], prep.w.shape[0])
