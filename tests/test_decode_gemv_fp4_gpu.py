"""`skinny_linear_mxfp4` (csrc/decode_gemv_fp4.hip) and the "mxfp4" decode
route on the GPU. A wave step is 128 k and a quad (one scale dword) 4 steps of
each of 8 waves: K = 32, 96 (a partial step) and 5216 = 4096 + 8 * 128 + 96
(every wave runs a full and a predicated quad, wave 0 a partial last step).
N: 1, 17, 33 (RT = 1) and the first N of RT = 2 and of RT = 4. The bound is
the single-rounding rule unchanged: widening code * scale to bf16 is exact."""

import functools

import pytest
import torch

from modalities_amd.ops import decode_linear as dl
from tests.kernel_oracles import F32_TINY, require, single_rounding_ratio
from tests.test_decode_gemv_fp4_cpu import _dequantized_copy
from tests.test_decode_gemv_gpu import _chunk, _decode_8, _model, _prompt

pytestmark = pytest.mark.gpu

DEV, K_TAIL = "cuda:0", 5216
MS = [1, 2, 15, 16, 17, 32]


@functools.lru_cache(maxsize=2)
def _weight(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * 0.05
    w = w * torch.exp2(torch.randint(-6, 7, (N, 1), generator=g).float())
    w = w * torch.exp2(torch.randint(-4, 5, (N, K // 32), generator=g)
                       .float()).repeat_interleave(32, 1)
    codes, scales = dl.quantize_weight_mxfp4(w.to(DEV))
    deq = dl.dequantize_weight_mxfp4(codes, scales).double()
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    return codes, scales, deq, bias


def _x(M, K, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(M, K + pad, generator=g).to(torch.bfloat16).to(DEV)
    return buf[:, pad // 2:pad // 2 + K] if pad else buf


def _ratio(x, N, K, bias):
    codes, scales, deq, b = _weight(N, K)
    b = b if bias else None
    y = dl.skinny_linear_mxfp4(x, codes, scales, b)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (x.shape[0], N)
    ref = x.double() @ deq.t()
    S = x.double().abs() @ deq.abs().t()
    if bias:
        ref, S = ref + b.double(), S + b.double().abs()
    return single_rounding_ratio(y, ref, S, floor=F32_TINY)


@pytest.mark.parametrize("K", [32, 96, K_TAIL])
@pytest.mark.parametrize("N", [1, 17, 33, "rt2", "rt4"])
def test_random_against_fp64(N, K):
    """Every M, with and without bias; at N = 33, K = 5216 also x as a view
    into a wider buffer (pad 32 is read in place, pad 6 copied)."""
    if isinstance(N, str):
        rt = int(N[2])
        N = 16 * rt * (dl.SKINNY_FP4_FILL_WGS - 1) + 1
        assert dl._fp4_row_tiles(N) == rt == 2 * dl._fp4_row_tiles(N - 1)
    r = {f"M{M}b{int(bias)}": _ratio(_x(M, K, seed=M + K), N, K, bias)
         for M in MS for bias in (False, True)}
    if (N, K) == (33, K_TAIL):
        r.update({f"pad{p}": _ratio(_x(17, K, 31, p), N, K, True)
                  for p in (32, 6)})
    require(f"skinny_linear_mxfp4 N{N} K{K}", r)


@pytest.mark.parametrize("k0", [0, 32, 64, 96, 1184, 4160, K_TAIL - 32])
def test_exact_decode_by_one_hot_rows(k0):
    """One-hot x rows select k0 .. k0 + 31: y[m, n] is scale * code bit for
    bit. Along n every k meets all 16 codes; scale bytes include 2 and 252.
    Offsets: the first wave step, another wave, the second quad, the tail."""
    K = K_TAIL
    n, k = torch.arange(32)[:, None], torch.arange(K)[None, :]
    nib = ((n + 5 * k) % 16).to(torch.uint8)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    sbytes = torch.tensor([2, 252, 127, 119, 140], dtype=torch.uint8)
    scales = sbytes[(n + 3 * torch.arange(K // 32)[None, :]) % 5].contiguous()
    x = torch.zeros(32, K, dtype=torch.bfloat16)
    x[torch.arange(32), k0 + torch.arange(32)] = 1.0
    y = dl.skinny_linear_mxfp4(x.to(DEV), codes.to(DEV), scales.to(DEV))
    deq = dl.dequantize_weight_mxfp4(codes, scales)
    # + 0.0: code 8 is -0.0; summed with the other k's +0.0 it is +0.0
    want = (deq[:, k0:k0 + 32].float().t() + 0.0).to(torch.bfloat16)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


def test_row_is_bit_identical_for_every_m_place_and_tiling():
    from modalities_amd.ops.backend import hip_ext
    codes, scales, _, b = _weight(65, K_TAIL)
    x = _x(32, K_TAIL, seed=21)
    y32 = dl.skinny_linear_mxfp4(x, codes, scales, b)
    y1 = dl.skinny_linear_mxfp4(x[20:21], codes, scales, b)
    assert torch.equal(y1[0], y32[20])
    packed = dl.pack_mxfp4_scales(scales)
    for rt in (1, 2, 4):
        assert torch.equal(
            hip_ext().skinny_linear_mxfp4(x, codes, packed, b, rt), y32), rt


def test_generate_tokens_with_mxfp4_weights():
    """The captured step launches the MXFP4 GEMM and replays to the eager
    text; the steps match the de-quantized copy on the bf16 route."""
    from modalities_amd.inference import text_generation as tg
    from modalities_amd.tokenization.tokenizer_wrapper import CharTokenizer
    model = _model(vocab_size=260)
    kw = dict(prompt_template="{text}", sequence_length=24, temperature=0.0,
              device=torch.device(DEV), decode_weight_format="mxfp4")
    text = tg.TextInferenceComponent(model, CharTokenizer(), **kw) \
        .generate_tokens("hello world")
    assert model.decode_weight_format == "mxfp4"
    eager = tg.TextInferenceComponent(model, CharTokenizer(),
                                      use_decode_graph=False, **kw)
    assert text == eager.generate_tokens("hello world")

    ref = _dequantized_copy(model)
    prompt = _prompt(2, _chunk() - 3)
    want, fed = _decode_8(ref, prompt, prefill=model)
    got, _ = _decode_8(model, prompt, feed=fed)
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-2,
                               atol=2e-2)
    replay, _ = _decode_8(model, prompt, graph=True, feed=fed)
    assert torch.equal(got, replay)
