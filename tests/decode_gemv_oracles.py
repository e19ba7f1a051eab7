"""fp64 oracle and checker for `skinny_linear` (no GPU needed), in the style
of tests/kernel_oracles.py.

The reference is computed in fp64 from the very `wq`, `scale`, `x` and `bias`
the kernel receives:  ref[m, n] = scale[n] * sum_k x[m, k] * wq[n, k] + bias[n]
(scale = 1 for bf16 weights).  The bound is the project's single-rounding
rule, not a fitted number:

    |y - ref| <= 2^-8 |ref| + 2^-18 S + floor,
    S = scale[n] * sum_k |x[m, k] * wq[n, k]| + |bias[n]|.

One bf16 ulp for the single rounding of the output, 64 fp32 ulps of the sum
of |terms| for the fp32 accumulation in whatever order.

`check_skinny_linear(fn, ...)` takes a callable with the op's signature, so
it serves the HIP kernel on the GPU and the torch implementation and its
deliberate mutants on the CPU.  It returns {name: ratio}; a correct
implementation has every ratio <= 1 (`kernel_oracles.require` asserts it).
"""

import torch

from tests.kernel_oracles import F32_TINY, single_rounding_ratio

E4M3 = torch.float8_e4m3fn


def e4m3_codes(codes):
    """uint8 codes -> float8_e4m3fn tensor of the same shape (bit cast)."""
    return torch.as_tensor(codes, dtype=torch.uint8).view(E4M3)


def all_valid_codes():
    """The 254 e4m3 codes that are not NaN (0x7F and 0xFF are)."""
    c = torch.arange(256, dtype=torch.int32)
    return c[(c & 0x7F) != 0x7F].to(torch.uint8)


def skinny_reference(x, w, scale, bias):
    """(ref, S) in fp64, from the kernel's own inputs."""
    xd = x.double()
    wd = w.to(torch.float32).double()
    ref = xd @ wd.t()
    S = xd.abs() @ wd.abs().t()
    if scale is not None:
        ref = ref * scale.double()
        S = S * scale.double().abs()
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs()
    return ref, S


def check_skinny_linear(fn, x, w, scale, bias):
    y = fn(x, w, scale, bias)
    assert y.dtype == torch.bfloat16, y.dtype
    assert tuple(y.shape) == (x.shape[0], w.shape[0]), tuple(y.shape)
    ref, S = skinny_reference(x.cpu(), w.cpu(),
                              None if scale is None else scale.cpu(),
                              None if bias is None else bias.cpu())
    return {"y": single_rounding_ratio(y.cpu(), ref, S, floor=F32_TINY)}


def make_case(M, N, K, fmt, bias, seed, x_pad=0, device="cpu"):
    """Random inputs: x ~ N(0, 1) bf16 (rows strided by K + x_pad when x_pad
    is set, a view into a wider buffer), w ~ N(0, 0.05) with a per-row
    spread of magnitudes, quantized for "fp8_e4m3"."""
    from modalities_amd.ops import quantize_weight_fp8
    g = torch.Generator().manual_seed(seed)
    xbuf = torch.randn(M, K + x_pad, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * 0.05
    w = w * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g).float())
    b = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16) if bias else None
    if fmt == "fp8_e4m3":
        wq, scale = quantize_weight_fp8(w)
    else:
        wq, scale = w.to(torch.bfloat16), None
    xbuf = xbuf.to(device)
    x = xbuf[:, x_pad // 2:x_pad // 2 + K] if x_pad else xbuf
    return (x, wq.to(device), None if scale is None else scale.to(device),
            None if b is None else b.to(device))
