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

`skinny_linear_mfma` (csrc/decode_gemv_mfma.hip) has the same contract for
1 <= M <= 32 rows. It feeds the weight to the matrix cores (MFMA), so its
arithmetic per weight does not grow with M; its sums are fp32 in another
fixed order, so it agrees with `skinny_linear` to the rounding bound, not
bit for bit.

`PreparedLinear` / `step_linear` are what the model uses: a prepared copy of
a Linear's weight, and the call that takes it for a single-token step: up to
8 rows through `skinny_linear`, 9 to 32 (on the GPU) through
`skinny_linear_mfma`.
`set_decode_mfma_min_rows` / MA_DECODE_MFMA_MIN_M move that border down for
A/B.

MXFP4 (`quantize_weight_mxfp4`, `skinny_linear_mxfp4`, decode weight format
"mxfp4"): OCP microscaling FP4, 0.53 bytes per weight. e2m1 codes (sign, two
exponent bits, one mantissa bit: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}), two per
byte with k = 2j in the low nibble of byte j and k = 2j + 1 in the high one,
and one e8m0 scale byte (2^(byte - 127)) per block of 32 consecutive k:

    e = ceil(log2(amax_block / 6)) clamped to [-125, 125],  byte = e + 127
    code = e2m1(w / 2^e)             (nearest, ties to the even mantissa bit)

The block's largest value lands in (3, 6] (6 is the largest e2m1 value), so
nothing saturates; that is the project's ceil rule, not the floor-and-
saturate rule of the OCP text. A zero block gets byte 127; the clamp keeps
0.5 * 2^e and 6 * 2^e normal bf16 values; the NaN byte 0xFF is never
produced. A code times a power of two is exact in bf16, so the de-quantized
model on the bf16 route is an exact reference here too.
`skinny_linear_mxfp4` (csrc/decode_gemv_fp4.hip) is one MFMA kernel for
1 <= M <= 32: gfx950 widens a byte to two scaled bf16 values in one
instruction, half a VALU op per weight whatever M is.
"""

import os
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from modalities_amd.ops.backend import hip_ext, use_hip
from modalities_amd.ops.rms_norm import RMSNorm
from modalities_amd.ops.swiglu import silu_mul_joint

E4M3_MAX = 448.0
SKINNY_MAX_M = 8
SKINNY_MFMA_MAX_M = 32
# skinny_linear_mfma: a workgroup owns 16 * RT weight rows. RT = 2 halves the
# x bytes a workgroup pulls from L2 per weight byte and wins wherever it still
# leaves this many workgroups (3/4 of the MI355X's 256 CUs; measured at N =
# 7680: 240 workgroups, against N = 2560: 80, nothing in between;
# profiles/decode_gemv.md).
SKINNY_MFMA_FILL_WGS = 192
SKINNY_K_MULTIPLE = 16
DECODE_WEIGHT_FORMATS = ("fp8_e4m3", "bf16", "mxfp4")
MXFP4_BLOCK = 32
MXFP4_MAX = 6.0
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # by code & 7
MXFP4_SCALE_BIAS = 127
MXFP4_MAX_EXP = 125
# skinny_linear_mxfp4: a workgroup owns 16 * RT weight rows, RT in (4, 2, 1):
# the largest that still leaves this many workgroups (measured: RT = 4 wins
# with 216 and loses with 120, RT = 2 wins with 240 and loses with 80;
# profiles/decode_gemv.md, "RT A/B"). The packed scale layout is the
# kernel's: [N, waves, k-groups, steps per wave].
SKINNY_FP4_FILL_WGS = 192
SKINNY_FP4_WAVES = 8
SKINNY_FP4_GROUPS = 4
SKINNY_FP4_QUAD = 4


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


def quantize_weight_mxfp4(w: torch.Tensor
                          ) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (bf16 or fp32), K % 32 == 0 -> (codes uint8 [N, K/2], scales
    uint8 [N, K/32]) in the MXFP4 layout of the module docstring. Pure torch,
    bit-identical on CPU and GPU. Non-finite weights raise ValueError."""
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        raise ValueError("quantize_weight_mxfp4: w must be a [N, K] tensor")
    if w.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"quantize_weight_mxfp4: w must be bf16 or fp32, got "
                        f"{w.dtype}")
    N, K = w.shape
    if K < MXFP4_BLOCK or K % MXFP4_BLOCK != 0:
        raise ValueError(f"quantize_weight_mxfp4: K must be a positive "
                         f"multiple of {MXFP4_BLOCK}, got {K}")
    wf = w.detach().float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_mxfp4: w holds non-finite values")
    amax = wf.abs().amax(dim=2)
    # amax / 6 = m * 2^e with m in [0.5, 1): ceil(log2) is e, or e - 1 when
    # the ratio is itself a power of two (m == 0.5). Exact, no log.
    m, e = torch.frexp(amax / MXFP4_MAX)
    e = torch.where(m == 0.5, e - 1, e)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    e = e.clamp(-MXFP4_MAX_EXP, MXFP4_MAX_EXP)
    # 2^-e built from its bits (127 - e is in [2, 252]): the product is exact
    inv = ((MXFP4_SCALE_BIAS - e).to(torch.int32) << 23).view(torch.float32)
    a = (wf.abs() * inv[:, :, None]).clamp(max=MXFP4_MAX)
    # nearest with ties to even on the grid of each binade: steps of 0.5
    # below 2, of 1 below 4, of 2 up to 6 (torch.round is half-to-even)
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
    q = torch.round(a / step) * step
    # value -> code: 0, .5, 1, 1.5 are 2q; 2, 3 are q + 2; 4, 6 are q/2 + 4
    code = torch.where(q < 2, 2 * q, torch.where(q < 4, q + 2, q / 2 + 4))
    code = code.to(torch.uint8) | torch.signbit(wf).to(torch.uint8) * 8
    code = code.reshape(N, K // 2, 2)
    codes = (code[:, :, 0] | (code[:, :, 1] << 4)).contiguous()
    scales = (e + MXFP4_SCALE_BIAS).to(torch.uint8).contiguous()
    return codes, scales


def mxfp4_scale_steps(K: int) -> int:
    """Steps per wave the packed scale layout holds: a wave's share of the
    ceil(K / 128) wave steps, rounded up to whole dwords."""
    steps = -(-K // (MXFP4_BLOCK * SKINNY_FP4_GROUPS))
    per_wave = -(-steps // SKINNY_FP4_WAVES)
    return -(-per_wave // SKINNY_FP4_QUAD) * SKINNY_FP4_QUAD


def pack_mxfp4_scales(scales: torch.Tensor) -> torch.Tensor:
    """scales uint8 [N, K/32] -> uint8 [N, 8, 4, T] in the order the kernel
    consumes them: [n, w, g, t] is the scale of block 4 * (w + 8 t) + g, so a
    lane's next four steps are one dword; blocks past K/32 hold 127 (2^0)."""
    N, C = scales.shape
    T = mxfp4_scale_steps(C * MXFP4_BLOCK)
    per_t = SKINNY_FP4_WAVES * SKINNY_FP4_GROUPS
    padded = scales.new_full((N, T * per_t), MXFP4_SCALE_BIAS)
    padded[:, :C] = scales
    return padded.view(N, T, SKINNY_FP4_WAVES, SKINNY_FP4_GROUPS) \
        .permute(0, 2, 3, 1).contiguous()


def _unpacked_mxfp4_scales(scales: torch.Tensor, C: int) -> torch.Tensor:
    if scales.dim() == 2:
        return scales
    return scales.permute(0, 3, 1, 2).reshape(scales.shape[0], -1)[:, :C]


def dequantize_weight_mxfp4(codes: torch.Tensor,
                            scales: torch.Tensor) -> torch.Tensor:
    """(codes uint8 [N, K/2], scales uint8 [N, K/32] or their packed form)
    -> bf16 [N, K], exactly code * 2^(scale - 127)."""
    N, half = codes.shape
    C = half * 2 // MXFP4_BLOCK
    sc = _unpacked_mxfp4_scales(scales, C)
    if tuple(sc.shape) != (N, C):
        raise ValueError(f"dequantize_weight_mxfp4: scales must be [N, K/32] "
                         f"= {(N, C)}, got {tuple(sc.shape)}")
    nib = torch.stack((codes & 0xF, codes >> 4), dim=2).reshape(N, 2 * half)
    mag = torch.tensor(MXFP4_VALUES, device=codes.device)[(nib & 7).long()]
    val = torch.where((nib & 8) != 0, -mag, mag)
    two_e = (sc.to(torch.int32) << 23).view(torch.float32)   # as the kernel
    val = val.view(N, C, MXFP4_BLOCK) * two_e[:, :, None]
    return val.reshape(N, 2 * half).to(torch.bfloat16)


def _fp4_row_tiles(N: int) -> int:
    for rt in (4, 2):
        if -(-N // (16 * rt)) >= SKINNY_FP4_FILL_WGS:
            return rt
    return 1


def skinny_linear_mxfp4(x: torch.Tensor, codes: torch.Tensor,
                        scales: torch.Tensor,
                        bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [M, N] bf16 = x [M, K] . dequantize_weight_mxfp4(codes, scales)^T
    (+ bias[n]) for 1 <= M <= 32, K % 32 == 0: fp32 products and sums, one
    rounding. x: bf16, unit stride in K, rows may be strided. codes: uint8
    [N, K/2]; scales: uint8 [N, K/32], or `pack_mxfp4_scales` of it (what
    `prepare_linear` keeps; the plain layout is packed on every call). A
    row's result does not depend on M or on where the row sits in x.
    Measured once on the 2.7B shapes (profiles/decode_gemv.md, "MXFP4
    kernel"): against the e4m3 kernels it ties at M = 1 (lm_head 1.12x) and
    wins 1.1-2.5x at M = 8..32; against hipBLASLt on bf16 it wins 1.4-2.5x
    up to M = 16 and 1.08-1.25x at M = 32, where W_2 only ties (1.01x).
    Inference only (no autograd)."""
    for name, t in (("x", x), ("codes", codes), ("scales", scales)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"skinny_linear_mxfp4: {name} must be a tensor")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"skinny_linear_mxfp4: x must be bf16, got {x.dtype}")
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise TypeError("skinny_linear_mxfp4: codes and scales must be uint8")
    if x.dim() != 2 or codes.dim() != 2:
        raise ValueError("skinny_linear_mxfp4: x must be [M, K] and codes "
                         f"[N, K/2], got {tuple(x.shape)} and "
                         f"{tuple(codes.shape)}")
    M, K = x.shape
    N = codes.shape[0]
    if not 1 <= M <= SKINNY_MFMA_MAX_M:
        raise ValueError(f"skinny_linear_mxfp4: M must be in [1, "
                         f"{SKINNY_MFMA_MAX_M}], got {M}")
    if K < MXFP4_BLOCK or K % MXFP4_BLOCK != 0 or codes.shape[1] * 2 != K:
        raise ValueError(f"skinny_linear_mxfp4: K must be a positive multiple "
                         f"of {MXFP4_BLOCK} shared by x and codes, got {K} "
                         f"and {codes.shape[1] * 2}")
    if N < 1 or not codes.is_contiguous():
        raise ValueError("skinny_linear_mxfp4: codes must be contiguous with "
                         "at least one row")
    want = ((N, K // MXFP4_BLOCK), (N, SKINNY_FP4_WAVES, SKINNY_FP4_GROUPS,
                                    mxfp4_scale_steps(K)))
    if tuple(scales.shape) not in want:
        raise ValueError(f"skinny_linear_mxfp4: scales must be [N, K/32] = "
                         f"{want[0]} or packed {want[1]}, got "
                         f"{tuple(scales.shape)}")
    if x.stride(1) != 1:
        raise ValueError("skinny_linear_mxfp4: x must have unit stride in K")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.bfloat16:
            raise TypeError("skinny_linear_mxfp4: bias must be a bf16 tensor "
                            "or None")
        if tuple(bias.shape) != (N,) or not bias.is_contiguous():
            raise ValueError(f"skinny_linear_mxfp4: bias must be contiguous "
                             f"[N] = {(N,)}, got {tuple(bias.shape)}")
    for name, t in (("codes", codes), ("scales", scales), ("bias", bias)):
        if t is not None and t.device != x.device:
            raise ValueError(f"skinny_linear_mxfp4: {name} is on {t.device}, "
                             f"x on {x.device}")
    if use_hip(x, codes, scales, bias):
        if (M > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()   # the kernel reads x in 16-byte pieces
        if scales.dim() == 2:
            scales = pack_mxfp4_scales(scales)
        return hip_ext().skinny_linear_mxfp4(x, codes, scales.contiguous(),
                                             bias, _fp4_row_tiles(N))
    return _skinny_linear_ref(x, dequantize_weight_mxfp4(codes, scales), None,
                              bias)


def _check_skinny_args(x, w, scale, bias, max_m=SKINNY_MAX_M):
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
    if not 1 <= M <= max_m:
        raise ValueError(f"skinny_linear: M must be in [1, {max_m}], "
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


def _check_fused_args(x, w, norm_weight, norm_eps, residual, glu):
    M, K = x.shape
    N = w.shape[0]
    if norm_weight is not None:
        if not isinstance(norm_weight, torch.Tensor) \
                or norm_weight.dtype != torch.bfloat16:
            raise TypeError("skinny_linear: norm_weight must be a bf16 tensor "
                            "or None")
        if tuple(norm_weight.shape) != (K,) or not norm_weight.is_contiguous():
            raise ValueError(f"skinny_linear: norm_weight must be contiguous "
                             f"[K] = {(K,)}, got {tuple(norm_weight.shape)}")
        if norm_weight.device != x.device:
            raise ValueError(f"skinny_linear: norm_weight is on "
                             f"{norm_weight.device}, x on {x.device}")
        if not norm_eps >= 0:
            raise ValueError(f"skinny_linear: norm_eps must be >= 0, got "
                             f"{norm_eps}")
    if glu and N % 2 != 0:
        raise ValueError(f"skinny_linear: glu needs an even N (gate | up "
                         f"rows), got {N}")
    if residual is not None:
        n_out = N // 2 if glu else N
        if not isinstance(residual, torch.Tensor) \
                or residual.dtype != torch.bfloat16:
            raise TypeError("skinny_linear: residual must be a bf16 tensor or "
                            "None")
        if tuple(residual.shape) != (M, n_out):
            raise ValueError(f"skinny_linear: residual must be [M, N_out] = "
                             f"{(M, n_out)}, got {tuple(residual.shape)}")
        if residual.stride(1) != 1:
            raise ValueError("skinny_linear: residual must have unit stride "
                             "in N")
        if residual.device != x.device:
            raise ValueError(f"skinny_linear: residual is on "
                             f"{residual.device}, x on {x.device}")


def _skinny_linear_fused_ref(x, w, scale, bias, norm_weight, norm_eps,
                             residual, glu):
    xf = x.float()
    if norm_weight is not None:
        inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + norm_eps)
        xf = xf * norm_weight.float()
    acc = xf @ w.float().t()
    if norm_weight is not None:
        acc = acc * inv
    if scale is not None:
        acc = acc * scale
    if bias is not None:
        acc = acc + bias.float()
    if glu:
        h = acc.shape[1] // 2
        acc = F.silu(acc[:, :h]) * acc[:, h:]
    if residual is not None:
        acc = acc + residual.float()
    return acc.to(torch.bfloat16)


def skinny_linear(x: torch.Tensor, w: torch.Tensor,
                  scale: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, *,
                  norm_weight: Optional[torch.Tensor] = None,
                  norm_eps: float = 1e-6,
                  residual: Optional[torch.Tensor] = None,
                  glu: bool = False) -> torch.Tensor:
    """y [M, N] bf16 = x [M, K] . w [N, K]^T (* scale[n]) (+ bias[n]).

    x: bf16, 1 <= M <= 8, unit stride in K; rows may be strided (a view into
    a wider buffer). w: contiguous [N, K], float8_e4m3fn with `scale` fp32
    [N], or bf16 with scale None. bias: bf16 [N] or None. K % 16 == 0.
    A row's result does not depend on M or on where the row sits in x.
    Inference only (no autograd).

    Three independent options fold the elementwise neighbours of a decode
    GEMM into it (csrc/decode_gemv_fused.hip); with none set the call is the
    plain kernel's, bit for bit:

    * norm_weight bf16 [K], norm_eps: x is the raw input of an RMSNorm with
      this weight; y is the linear of the normalised x, which is never
      written: inv[m] * sum_k (x[m, k] g[k]) w[n, k] with inv[m] =
      rsqrt(mean_k x[m, k]^2 + eps) applied once per output.
    * glu: w is a packed [2H, K] gate | up weight (gate rows first, as
      `SwiGLU.Wv` stores it) and y [M, H] = silu(gate) * up, each half after
      its own scale and bias.
    * residual bf16 [M, N_out] (unit stride in N): added last.

    Order: * inv[m], * scale[n], + bias[n], gate, + residual, all in fp32,
    then the one rounding to bf16. y is a fresh tensor."""
    _check_skinny_args(x, w, scale, bias)
    if norm_weight is None and residual is None and not glu:
        if use_hip(x, w, scale, bias):
            if (x.shape[0] > 1 and x.stride(0) % 8 != 0) \
                    or x.data_ptr() % 16 != 0:
                x = x.contiguous()   # the kernel reads x in 16-byte pieces
            return hip_ext().skinny_linear(x, w, scale, bias)
        return _skinny_linear_ref(x, w, scale, bias)
    _check_fused_args(x, w, norm_weight, norm_eps, residual, glu)
    if use_hip(x, w, scale, bias, norm_weight, residual):
        if (x.shape[0] > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()   # the kernel reads x in 16-byte pieces
        if norm_weight is not None and norm_weight.data_ptr() % 16 != 0:
            norm_weight = norm_weight.clone()   # and g likewise
        return hip_ext().skinny_linear_fused(x, w, scale, bias, norm_weight,
                                             float(norm_eps), residual,
                                             bool(glu))
    return _skinny_linear_fused_ref(x, w, scale, bias, norm_weight, norm_eps,
                                    residual, glu)


def skinny_linear_mfma(x: torch.Tensor, w: torch.Tensor,
                       scale: Optional[torch.Tensor] = None,
                       bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`skinny_linear`'s contract for 1 <= M <= 32, on the matrix cores:
    y [M, N] bf16 = x [M, K] . w [N, K]^T (* scale[n]) (+ bias[n]), fp32
    products and sums, one rounding. A row's result does not depend on M or
    on where the row sits in x. Against hipBLASLt on the bf16 weight
    (2.7B shapes, profiles/decode_gemv.md): with e4m3 weights it wins at
    M = 8 (1.11-1.73x) and M = 16 (1.10-1.53x; lm_head ties) and loses at
    M = 32 (0.73-0.96x), where the x every workgroup reads from L2 outweighs
    the halved weight bytes; with bf16 weights it loses at most shapes."""
    _check_skinny_args(x, w, scale, bias, SKINNY_MFMA_MAX_M)
    if use_hip(x, w, scale, bias):
        if (x.shape[0] > 1 and x.stride(0) % 8 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()   # the kernel reads x in 16-byte pieces
        rt = 2 if -(-w.shape[0] // 32) >= SKINNY_MFMA_FILL_WGS else 1
        return hip_ext().skinny_linear_mfma(x, w, scale, bias, rt)
    return _skinny_linear_ref(x, w, scale, bias)


def _env_min_rows() -> int:
    n = int(os.environ.get("MA_DECODE_MFMA_MIN_M", SKINNY_MAX_M + 1))
    if not 1 <= n <= SKINNY_MAX_M + 1:
        raise ValueError(f"MA_DECODE_MFMA_MIN_M must be in [1, "
                         f"{SKINNY_MAX_M + 1}], got {n}")
    return n


_MFMA_MIN_ROWS = _env_min_rows()


def set_decode_mfma_min_rows(n: int) -> None:
    """Smallest batch `step_linear` sends to `skinny_linear_mfma`: 9 (the
    default) keeps batches of up to 8 on `skinny_linear`; 1..8 move them to
    the MFMA kernel (A/B). MA_DECODE_MFMA_MIN_M sets the initial value."""
    global _MFMA_MIN_ROWS
    if not 1 <= int(n) <= SKINNY_MAX_M + 1:
        raise ValueError(f"set_decode_mfma_min_rows: n must be in [1, "
                         f"{SKINNY_MAX_M + 1}], got {n}")
    _MFMA_MIN_ROWS = int(n)


def decode_mfma_min_rows() -> int:
    return _MFMA_MIN_ROWS


_FUSED_STEP = os.environ.get("MA_DECODE_FUSED_STEP", "0")
if _FUSED_STEP not in ("0", "1"):
    raise ValueError(f"MA_DECODE_FUSED_STEP must be 0 or 1, got "
                     f"{_FUSED_STEP!r}")
_FUSED_STEP = _FUSED_STEP == "1"


def set_decode_fused_step(on: bool) -> None:
    """Whether a single-token step on prepared bf16 / e4m3 decode weights
    folds its RMSNorms, its SwiGLU gate and its residual adds into the skinny
    GEMMs next to them (`skinny_linear`'s norm_weight / glu / residual):
    5 of about 13 launches per layer. Off by default; MA_DECODE_FUSED_STEP
    sets the initial value. The fused step agrees with the unfused one to
    rounding, not bit for bit: it skips the bf16 roundings in between."""
    global _FUSED_STEP
    if not isinstance(on, bool):
        raise ValueError(f"set_decode_fused_step: on must be a bool, got "
                         f"{on!r}")
    _FUSED_STEP = on


def decode_fused_step() -> bool:
    return _FUSED_STEP


class PreparedLinear(NamedTuple):
    """Decode-time copy of one Linear: w [N, K] in `fmt`, its scale (e4m3:
    fp32 [N]; mxfp4: w holds the uint8 codes [N, K/2] and scale the packed
    e8m0 bytes of `pack_mxfp4_scales`; bf16: None) and the bias in bf16."""
    w: torch.Tensor
    scale: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]


def skinny_eligible(in_features: int, fmt: Optional[str] = None) -> bool:
    mult = MXFP4_BLOCK if fmt == "mxfp4" else SKINNY_K_MULTIPLE
    return in_features >= mult and in_features % mult == 0


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
    if fmt == "mxfp4":
        codes, scales = quantize_weight_mxfp4(w)
        return PreparedLinear(codes, pack_mxfp4_scales(scales), b)
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


def _fused_step_ok(prep, x, rows, norm, residual) -> bool:
    if not _FUSED_STEP or prep is None or prep.w.dtype == torch.uint8:
        return False
    if not 1 <= rows <= SKINNY_MAX_M or (x.is_cuda and rows >= _MFMA_MIN_ROWS):
        return False
    if x.dtype != torch.bfloat16 or x.device != prep.w.device:
        return False
    if norm is not None and not (
            isinstance(norm, RMSNorm) and norm.weight.dtype == torch.bfloat16
            and tuple(norm.weight.shape) == (x.shape[-1],)
            and norm.weight.device == x.device):
        return False
    return residual is None or (residual.dtype == torch.bfloat16
                                and residual.device == x.device)


def step_linear(lin: torch.nn.Module, x: torch.Tensor,
                norm: Optional[torch.nn.Module] = None,
                residual: Optional[torch.Tensor] = None,
                glu: bool = False) -> torch.Tensor:
    """`lin(x)` for a single-token step, optionally with its neighbours:
    residual + gate(lin(norm(x))), where `norm` is the norm module in front
    of `lin`, glu=True gates a packed gate | up projection (`silu_mul_joint`)
    and `residual` is added last. With `set_decode_fused_step(True)`, a
    prepared bf16 / e4m3 copy, at most 8 rows on the VALU route and `norm`
    (if given) an `ops.rms_norm.RMSNorm` over K, the whole expression is one
    `skinny_linear` launch with the fused options. In every other case (the
    switch off, an MXFP4 copy, a batch on the MFMA route, a LayerNorm, a
    layer without a prepared copy) it is the composition of the pieces as
    they run unfused, bit for bit: `norm(x)`, the linear below,
    `silu_mul_joint`, the add."""
    if norm is None and residual is None and not glu:
        return _step_linear(lin, x)
    prep = lin.__dict__.get(_ATTR)
    rows = x.numel() // x.shape[-1]
    if _fused_step_ok(prep, x, rows, norm, residual):
        n_out = prep.w.shape[0] // 2 if glu else prep.w.shape[0]
        y = skinny_linear(
            x.reshape(rows, x.shape[-1]), prep.w, prep.scale, prep.bias,
            norm_weight=None if norm is None else norm.weight.detach(),
            norm_eps=1e-6 if norm is None else norm.eps,
            residual=None if residual is None
            else residual.reshape(rows, n_out), glu=glu)
        return y.view(*x.shape[:-1], n_out)
    y = _step_linear(lin, x if norm is None else norm(x))
    if glu:
        y = silu_mul_joint(y)
    return y if residual is None else residual + y


def _step_linear(lin: torch.nn.Module, x: torch.Tensor) -> torch.Tensor:
    """`lin(x)` for a single-token step x [B, 1, K]: on the prepared weight
    when `lin` has one, B <= 32 and x is bf16 on the weight's device --
    through `skinny_linear` for B <= 8, through `skinny_linear_mfma` for
    9 <= B <= 32 (`set_decode_mfma_min_rows` moves the border down);
    through the module itself (F.linear on the resident weight) otherwise.
    The MFMA route is the device's: on the CPU, where there is no kernel to
    reach, a step of more than 8 rows stays on F.linear as it always has.
    An MXFP4 copy (uint8 codes) sends 1 <= B <= 32 to `skinny_linear_mxfp4`,
    on the CPU too (there the torch expression on the de-quantized weight)."""
    prep = lin.__dict__.get(_ATTR)
    if prep is None:
        return lin(x)
    rows = x.numel() // x.shape[-1]
    if prep.w.dtype == torch.uint8:
        if not 1 <= rows <= SKINNY_MFMA_MAX_M or x.dtype != torch.bfloat16 \
                or x.device != prep.w.device:
            return F.linear(x, lin.weight, lin.bias)
        y = skinny_linear_mxfp4(x.reshape(rows, x.shape[-1]), prep.w,
                                prep.scale, prep.bias)
        return y.view(*x.shape[:-1], prep.w.shape[0])
    mfma = x.is_cuda and rows >= _MFMA_MIN_ROWS
    max_rows = SKINNY_MFMA_MAX_M if mfma else SKINNY_MAX_M
    if rows > max_rows or rows < 1 or x.dtype != torch.bfloat16 \
            or x.device != prep.w.device:
        return F.linear(x, lin.weight, lin.bias)
    x2 = x.reshape(rows, x.shape[-1])
    if mfma:
        y = skinny_linear_mfma(x2, prep.w, prep.scale, prep.bias)
    else:
        y = skinny_linear(x2, prep.w, prep.scale, prep.bias)
    return y.view(*x.shape[:-1], prep.w.shape[0])
