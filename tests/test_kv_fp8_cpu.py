"""The e4m3 KV-cache format on its torch route (no GPU): format properties,
the model's FP8-cache path against a round-tripped bf16 cache, and the
argument checks."""

import pytest
import torch

from modalities_amd import ops
from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig, KVCache

E4M3 = torch.float8_e4m3fn


def _rows(D, seed=0):
    """bf16 [64, 3, D] whose rows span 40 binades."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-20, 20, (64, 3, 1), generator=g).float()
    return (torch.randn(64, 3, D, generator=g) * torch.exp2(e)).bfloat16()


def _rt(x):
    return ops.dequantize_kv_fp8(*ops.quantize_kv_fp8(x))


@pytest.mark.parametrize("D", [16, 64, 80, 128])
def test_format_properties(D):
    x = _rows(D, seed=D)
    codes, scale = ops.quantize_kv_fp8(x)
    assert codes.dtype == E4M3 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    # power-of-two scales; the largest element lands in (224, 448] (its
    # code may round down to 224)
    assert (torch.frexp(scale)[0] == 0.5).all()
    cmax = codes.float().abs().amax(-1)
    assert ((cmax >= 224) & (cmax <= 448)).all()
    # scale * code is exact in bf16
    exact = codes.float() * scale.unsqueeze(-1)
    deq = ops.dequantize_kv_fp8(codes, scale)
    assert torch.equal(deq.float(), exact)
    # |x - scale code| <= amax / 16. e4m3 has 3 mantissa bits: in units of
    # the scale its step is 32 on [256, 448] and 16 on [128, 256], so the
    # error is at most half of that, 16 or 8. The row's largest element is
    # above 224: if it is above 256, 16 < amax / 16; if not, every element
    # is at most 256 and 8 < 224 / 16 < amax / 16.
    err = (x.float() - exact).abs().amax(-1)
    amax = x.float().abs().amax(-1)
    assert (err <= amax / 16).all()
    # idempotent in value
    assert torch.equal(_rt(deq), deq)


def test_zero_row():
    x = _rows(64)
    x[5, 1] = 0
    codes, scale = ops.quantize_kv_fp8(x)
    assert scale[5, 1] == 1 and torch.count_nonzero(codes[5, 1].float()) == 0


def _tiny(**kw):
    torch.manual_seed(3)
    cfg = dict(vocab_size=64, n_layer=2, n_embd=64, n_head_q=4, n_head_kv=2,
               ffn_hidden=128, sequence_length=32, seed=7, dropout=0.0)
    cfg.update(kw)
    return GPT2LLM(GPT2LLMConfig(**cfg)).to(torch.bfloat16).eval()


@pytest.mark.parametrize("kw", [dict(fused_qkv=True), dict(
    fused_qkv=False, poe_type="ABSOLUTE", qkv_transform="IdentityTransform")],
    ids=["rope", "absolute"])
def test_forward_cached_equals_round_tripped_bf16_cache(kw):
    """Prefill and a chunk attend on fresh bf16 K/V plus the de-quantised
    prefix: bit-equal to the bf16 cache whose rows are round-tripped after
    each call. A single token attends to its own quantised row, the bf16
    run to its bf16 row: the project's route tolerance."""
    model = _tiny(**kw)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 64, (2, 10), generator=g)
    fp8 = model.new_kv_cache(2, 16, kv_format="fp8_e4m3")
    ref = model.new_kv_cache(2, 16)
    assert fp8.k[0].dtype == E4M3 and fp8.k_scale[0].shape == (2, 16, 2)
    lo = 0
    for hi in (6, 9, 10):
        a = model.forward_cached({"input_ids": ids[:, lo:hi]}, fp8)["logits"]
        b = model.forward_cached({"input_ids": ids[:, lo:hi]}, ref)["logits"]
        if hi - lo > 1:
            assert torch.equal(a, b)
        else:
            torch.testing.assert_close(a.float(), b.float(), rtol=2e-2,
                                       atol=2e-2)
        for i in range(2):
            for c, q, s in ((ref.k[i], fp8.k[i], fp8.k_scale[i]),
                            (ref.v[i], fp8.v[i], fp8.v_scale[i])):
                c[:, lo:hi] = _rt(c[:, lo:hi])
                # (after the single token the inputs of layer 1 differ)
                assert hi - lo == 1 or torch.equal(
                    ops.dequantize_kv_fp8(q[:, :hi], s[:, :hi]), c[:, :hi])
        lo = hi
    assert fp8.pos == ref.pos == 10


def test_argument_errors():
    q = torch.zeros(2, 1, 4, 64, dtype=torch.bfloat16)
    kv = torch.zeros(2, 1, 2, 64, dtype=torch.bfloat16)
    bf = torch.zeros(2, 8, 2, 64, dtype=torch.bfloat16)
    codes, sc = bf.to(E4M3), torch.ones(2, 8, 2)
    n = torch.tensor([3, 4], dtype=torch.int32)
    for call in (
            lambda c, **s: ops.decode_attention(q, c, c, n, **s),
            lambda c, **s: ops.decode_rope_append(q, kv, kv, None, None, n,
                                                  c, c, **s)):
        with pytest.raises(TypeError, match="float8_e4m3fn caches"):
            call(bf, k_scale=sc, v_scale=sc)            # bf16 with scales
        with pytest.raises(ValueError, match="needs k_scale"):
            call(codes)                                 # FP8 without
        with pytest.raises(ValueError, match="both"):
            call(codes, k_scale=sc)
        with pytest.raises(ValueError, match="v_scale must be"):
            call(codes, k_scale=sc, v_scale=sc[:, :4])
        with pytest.raises(TypeError, match="k_scale must be an fp32"):
            call(codes, k_scale=sc.double(), v_scale=sc)
        call(codes, k_scale=sc, v_scale=sc)
    with pytest.raises(TypeError):
        ops.quantize_kv_fp8(q.float())
    with pytest.raises(ValueError, match="kv_format"):
        KVCache(1, 1, 8, 2, 64, "cpu", torch.bfloat16, kv_format="fp8_e5m2")


def test_unknown_kv_cache_format_and_sharded_model():
    from modalities_amd.inference.text_generation import (
        TextInferenceComponent)
    model = _tiny()
    with pytest.raises(ValueError, match="kv_cache_format"):
        TextInferenceComponent(model, None, "{text}", 8,
                               kv_cache_format="int4")
    TextInferenceComponent(model, None, "{text}", 8,
                           kv_cache_format="fp8_e4m3")
    # what tensor / context parallelism does to a block: a bound forward
    model.blocks[0].attn.forward = model.blocks[0].attn.forward
    with pytest.raises(NotImplementedError, match="sharded"):
        model.new_kv_cache(1, 8, kv_format="fp8_e4m3")
    model.new_kv_cache(1, 8)
