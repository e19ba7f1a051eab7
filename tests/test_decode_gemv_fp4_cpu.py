"""MXFP4 weight quantizer and the "mxfp4" decode-weight wiring of GPT2LLM, on
the CPU (where `skinny_linear_mxfp4` is torch on the de-quantized weight)."""

import copy

import pytest
import torch

from modalities_amd.ops import decode_linear as dl
from tests.test_decode_gemv_cpu import MODEL_VARIANTS, _tiny

MAGS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]      # by code & 7


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_midpoints_round_to_the_even_code(sign):
    mids = [(a + b) / 2 for a, b in zip(MAGS, MAGS[1:])]
    assert mids == [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    even = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    w = torch.zeros(1, 32)
    w[0, :7] = torch.tensor(mids) * sign
    w[0, 31] = 6.0                                   # pins the scale to 2^0
    codes, scales = dl.quantize_weight_mxfp4(w)
    assert scales.tolist() == [[127]]
    got = dl.dequantize_weight_mxfp4(codes, scales).float()[0, :7]
    assert got.tolist() == [sign * v for v in even]


@pytest.mark.parametrize("e", [-125, -7, 0, 3, 125])
def test_block_scale_follows_the_ceil_rule(e):
    up, down = 1 + 2.0 ** -23, 1 - 2.0 ** -24
    w = torch.zeros(3, 32)
    w[:, 5] = torch.tensor([6.0, 6.0 * up, 6.0 * down]) * 2.0 ** e
    _, scales = dl.quantize_weight_mxfp4(w)
    want_above = min(e + 1, 125)                     # the clamp
    assert scales[:, 0].tolist() == [127 + e, 127 + want_above, 127 + e]


def test_zero_block_clamps_and_non_finite():
    w = torch.zeros(1, 96)
    w[0, 40] = 2.0 ** -140                           # e clamps at -125
    w[0, 70] = 3e38                                  # e clamps at +125
    codes, scales = dl.quantize_weight_mxfp4(w)
    assert codes.dtype == scales.dtype == torch.uint8
    assert tuple(codes.shape) == (1, 48) and scales.tolist() == [[127, 2, 252]]
    assert not bool(codes[0, :16].any())
    assert codes[0, 35].item() == 7                  # saturates at 6 * 2^125
    for bad in (float("inf"), float("nan")):
        w[0, 3] = bad
        with pytest.raises(ValueError, match="non-finite"):
            dl.quantize_weight_mxfp4(w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_round_trip_returns_the_same_codes_and_scales(dtype):
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 256, (8, 48), generator=g, dtype=torch.uint8)
    codes[:, ::16] = 0xF7                 # every block holds +-6: scale fixed
    scales = torch.randint(2, 253, (8, 3), generator=g, dtype=torch.uint8)
    w = dl.dequantize_weight_mxfp4(codes, scales)
    c2, s2 = dl.quantize_weight_mxfp4(w.to(dtype))
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


def test_nibble_and_byte_layout():
    """Row 0: k = 0..15 walk the codes 0..15, scale 2^1. Row 1: 6 at k = 31,
    -0.5 at k = 2, scale 2^-2."""
    w = torch.zeros(2, 32)
    w[0, :8] = torch.tensor(MAGS) * 2
    w[0, 8:16] = -torch.tensor(MAGS) * 2
    w[1, 31], w[1, 2] = 6.0 * 0.25, -0.5 * 0.25
    codes, scales = dl.quantize_weight_mxfp4(w)
    assert scales.tolist() == [[128], [125]]
    assert codes[0, :8].tolist() == [0x10, 0x32, 0x54, 0x76,
                                     0x98, 0xBA, 0xDC, 0xFE]
    assert codes[1].tolist() == [0, 0x09] + [0] * 13 + [0x70]
    assert torch.equal(dl.dequantize_weight_mxfp4(codes, scales).float(),
                       w)


def _dequantized_copy(model):
    ref = copy.deepcopy(model)
    ref.clear_decode_weights()
    with torch.no_grad():
        for a, b in zip(model._decode_linears(), ref._decode_linears()):
            p = dl.get_prepared(a)
            deq = dl.dequantize_weight_mxfp4(p.w, p.scale)
            if b.weight is ref.wte.weight:   # tied head: keep the bf16 table
                b.weight = torch.nn.Parameter(deq)
            else:
                b.weight.copy_(deq)
    return ref


@pytest.mark.parametrize("name", sorted(MODEL_VARIANTS))
def test_prepared_model_matches_dequantized_copy(name):
    model = _tiny(**MODEL_VARIANTS[name])
    with torch.no_grad():
        for lin in model._decode_linears():
            if lin.bias is not None:
                lin.bias.normal_(0, 0.1)
    plain = copy.deepcopy(model)
    model.prepare_decode_weights("mxfp4")
    if name == "split_gelu_tied":
        codes, _ = dl.quantize_weight_mxfp4(model.wte.weight)
        assert torch.equal(dl.get_prepared(model.lm_head).w, codes)
    ref = _dequantized_copy(model)
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, 97, (2, 5), generator=g)
    ca, cb = model.new_kv_cache(2, max_len=16), ref.new_kv_cache(2, max_len=16)
    out = model.forward_cached({"input_ids": prompt}, ca)["logits"]
    want = model.forward_cached({"input_ids": prompt}, cb)["logits"]
    unprepared = plain.forward_cached(
        {"input_ids": prompt}, plain.new_kv_cache(2, max_len=16))["logits"]
    assert torch.equal(out, unprepared), "the prefill stays on bf16 weights"
    for _ in range(8):
        nxt = want[:, -1, :].argmax(-1, keepdim=True)
        out = model.forward_cached({"input_ids": nxt}, ca)["logits"]
        want = ref.forward_cached({"input_ids": nxt}, cb)["logits"]
        torch.testing.assert_close(out.float(), want.float(),
                                   rtol=2e-2, atol=2e-2)


def test_in_features_48_keeps_f_linear():
    model = _tiny(n_embd=48, n_head_q=2, n_head_kv=2, ffn_hidden=128,
                  activation_type="gelu")
    model.prepare_decode_weights("mxfp4")
    by_k = {l.in_features: dl.get_prepared(l) for l in model._decode_linears()}
    assert by_k[48] is None and by_k[128].w.dtype == torch.uint8


def test_config_key_reaches_the_model(tmp_path):
    model = ("{sample_key: input_ids, prediction_key: logits, vocab_size: 260,"
             " n_layer: 2, n_head_q: 4, n_head_kv: 4, n_embd: 64,"
             " ffn_hidden: 128, sequence_length: 24, seed: 3}")
    cfg = tmp_path / "gen.yaml"
    cfg.write_text(f"""\
settings: {{referencing_keys: {{sample_key: input_ids, prediction_key: logits}},
           device: cpu, sequence_length: 24}}
model: {{component_key: model, variant_key: gpt2, config: {model}}}
tokenizer: {{component_key: tokenizer, variant_key: char, config: {{}}}}
text_inference: {{prompt_template: "{{text}}", temperature: 0.0,
                 decode_weight_format: mxfp4}}
""")
    from modalities_amd.api import _build_text_inference_component
    comp = _build_text_inference_component(cfg)
    assert comp.decode_weight_format == "mxfp4"
    comp.model.to(torch.bfloat16)
    assert isinstance(comp.generate_tokens("hey"), str)
    assert all(dl.get_prepared(l).w.dtype == torch.uint8
               for l in comp.model._decode_linears())
