"""FP8 weight quantizer, the skinny_linear checker against mutants, and the
prepared-decode-weight wiring of GPT2LLM -- all on the CPU."""

import copy

import pytest
import torch

from tests import decode_gemv_oracles as go
from tests import kernel_oracles as ko

E4M3 = torch.float8_e4m3fn


def _ops():
    from modalities_amd import ops
    return ops


def _bits(wq):
    return wq.view(torch.uint8)


# ------------------------------------------------------------------ quantizer
@pytest.mark.parametrize("e", [-20, -3, 0, 1, 9])
def test_every_code_survives_a_round_trip(e):
    """quantize(dequantize(code) * 2^e) returns the code, bit for bit: the
    row holds +-448, so its scale is exactly 2^e."""
    codes = go.all_valid_codes()
    assert codes.numel() == 254
    w = (go.e4m3_codes(codes).float() * 2.0 ** e)[None, :]
    wq, scale = _ops().quantize_weight_fp8(w)
    assert wq.dtype == E4M3 and wq.is_contiguous() and wq.shape == w.shape
    assert scale.dtype == torch.float32 and scale.tolist() == [2.0 ** e]
    got, want = _bits(wq)[0], codes.clone()
    # -0.0 (0x80) and +0.0 are one value; the sign of zero is kept or not
    zero = (want & 0x7F) == 0
    assert torch.equal(got[~zero], want[~zero])
    assert bool(((got[zero] & 0x7F) == 0).all())
    # the bf16 input gives the same codes (every e4m3 * 2^e is a bf16 value)
    wq_b, scale_b = _ops().quantize_weight_fp8(w.to(torch.bfloat16))
    assert torch.equal(_bits(wq_b), _bits(wq)) and torch.equal(scale_b, scale)


def test_ties_round_to_even():
    # e4m3 has 3 mantissa bits: between 16 and 32 the values step by 2, so
    # odd integers are ties. 448 pins the scale to 1.
    w = torch.tensor([[448.0, 17.0, 19.0, 21.0, 23.0, -17.0, -19.0,
                       1.0625, 1.1875]])
    wq, scale = _ops().quantize_weight_fp8(w)
    assert scale.tolist() == [1.0]
    assert wq.float().tolist() == [[448.0, 16.0, 20.0, 20.0, 24.0, -16.0,
                                    -20.0, 1.0, 1.25]]


def test_amax_maps_into_the_top_binade():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 48, generator=g) * torch.exp2(
        torch.randint(-30, 30, (64, 1), generator=g).float())
    w[1:4] = 0.0
    w[0, 0], w[1, 0], w[2, 0] = 1e30, -448.0, 224.0    # edges: huge, exact
    w[3, 5] = 2.0 ** -100                               # tiny row
    wq, scale = _ops().quantize_weight_fp8(w)
    m, e = torch.frexp(scale)
    assert bool((m == 0.5).all()), "scales must be powers of two"
    top = wq.float().abs().amax(dim=1)
    # amax / scale lies in (224, 448]; rounding to e4m3 can reach 224
    assert bool((top >= 224.0).all()) and bool((top <= 448.0).all()), top
    # amax = 448 * 2^k or 224 * 2^k: the ceil puts both at 448
    assert scale[1].item() == 1.0 and top[1].item() == 448.0
    assert scale[2].item() == 0.5 and top[2].item() == 448.0
    # values beyond amax cannot occur: nothing was clamped
    assert bool(((w / scale[:, None]).abs() <= 448.0).all())


def test_explicit_scale_exercises_the_clamp():
    w = torch.tensor([[1000.0, -1000.0, 449.0, 3.0]])
    wq, scale = _ops().quantize_weight_fp8(w, scale=torch.ones(1))
    assert wq.float().tolist() == [[448.0, -448.0, 448.0, 3.0]]
    assert scale.tolist() == [1.0]
    with pytest.raises(ValueError):
        _ops().quantize_weight_fp8(w, scale=torch.zeros(1))


def test_zero_rows_get_scale_one_and_zero_codes():
    w = torch.zeros(3, 32)
    w[1, 4] = 0.25
    wq, scale = _ops().quantize_weight_fp8(w)
    assert scale[0].item() == 1.0 and scale[2].item() == 1.0
    assert bool((_bits(wq)[0] == 0).all()) and bool((_bits(wq)[2] == 0).all())
    assert wq[1, 4].float().item() * scale[1].item() == 0.25


def test_no_nan_code_is_ever_produced():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(256, 256, generator=g) * torch.exp2(
        torch.randint(-120, 120, (256, 1), generator=g).float())
    w[:, ::7] *= 1e-6
    for t in (w, w.to(torch.bfloat16)):
        wq, _ = _ops().quantize_weight_fp8(t)
        assert bool(((_bits(wq) & 0x7F) != 0x7F).all())
    # the clamp is what keeps saturated values off the NaN code
    wq, _ = _ops().quantize_weight_fp8(torch.full((1, 16), 3e38),
                                       scale=torch.full((1,), 2.0 ** -100))
    assert bool((_bits(wq) == 0x7E).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_input_raises(bad):
    w = torch.ones(2, 16)
    w[1, 3] = bad
    with pytest.raises(ValueError, match="non-finite"):
        _ops().quantize_weight_fp8(w)
    with pytest.raises(TypeError):
        _ops().quantize_weight_fp8(torch.ones(2, 16, dtype=torch.float16))


def test_dequantized_weight_is_exact_in_bf16():
    g = torch.Generator().manual_seed(2)
    w = torch.randn(96, 80, generator=g) * torch.exp2(
        torch.randint(-20, 20, (96, 1), generator=g).float())
    wq, scale = _ops().quantize_weight_fp8(w)
    deq = wq.float() * scale[:, None]
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)


# -------------------------------------------------------------------- checker
CASES = [(1, 3, 16, False), (2, 65, 1040, True), (8, 17, 2560, True),
         (5, 64, 48, False)]


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "bf16"])
@pytest.mark.parametrize("M,N,K,bias", CASES)
def test_checker_passes_the_torch_implementation(fmt, M, N, K, bias):
    args = go.make_case(M, N, K, fmt, bias, seed=M * 1000 + N, x_pad=32)
    r = go.check_skinny_linear(_ops().skinny_linear, *args)
    ko.require(f"skinny_linear cpu {fmt} M{M} N{N} K{K}", r)


def _mutants():
    ref = _ops().skinny_linear

    def scale_of_previous_row(x, w, scale, bias):
        return ref(x, w, scale.roll(1), bias)

    def last_chunk_dropped(x, w, scale, bias):
        w2 = w.float().clone()
        w2[:, -16:] = 0
        return ref(x, w2.to(w.dtype), scale, bias)

    def bytes_swapped_in_a_group(x, w, scale, bias):
        b = w.view(torch.uint8).clone()
        b[:, 1::4], b[:, 2::4] = w.view(torch.uint8)[:, 2::4], \
            w.view(torch.uint8)[:, 1::4]
        return ref(x, b.view(w.dtype), scale, bias)

    def bias_after_rounding(x, w, scale, bias):
        y = ref(x, w, scale, None)
        return (y.float() + bias.float()).to(torch.bfloat16)

    return {f.__name__: f for f in (scale_of_previous_row, last_chunk_dropped,
                                    bytes_swapped_in_a_group,
                                    bias_after_rounding)}


@pytest.mark.parametrize("name", ["scale_of_previous_row",
                                  "last_chunk_dropped",
                                  "bytes_swapped_in_a_group",
                                  "bias_after_rounding"])
def test_checker_rejects_mutants(name):
    args = go.make_case(4, 65, 1040, "fp8_e4m3", True, seed=11)
    good = go.check_skinny_linear(_ops().skinny_linear, *args)
    assert max(good.values()) <= 1.0
    r = go.check_skinny_linear(_mutants()[name], *args)
    print(name, r)
    assert max(r.values()) > 1.0, f"mutant {name} passed the checker: {r}"


def test_skinny_linear_argument_errors():
    sl = _ops().skinny_linear
    x, w, scale, bias = go.make_case(2, 8, 32, "fp8_e4m3", True, seed=5)
    with pytest.raises(ValueError, match="M must be"):
        sl(x.repeat(5, 1)[:9], w, scale, bias)
    with pytest.raises(ValueError, match="multiple of 16"):
        sl(x[:, :24], w.view(torch.uint8)[:, :24].contiguous().view(E4M3),
           scale, bias)
    with pytest.raises(TypeError):
        sl(x.float(), w, scale, bias)
    with pytest.raises(TypeError):
        sl(x, w.float(), scale, bias)
    with pytest.raises(TypeError):
        sl(x, w, scale.double(), bias)
    with pytest.raises(TypeError):
        sl(x, w, None, bias)
    with pytest.raises(TypeError):
        sl(x, w, scale, bias.float())
    with pytest.raises(ValueError, match="contiguous"):
        sl(x, w.t().contiguous().t(), scale, bias)
    with pytest.raises(ValueError, match="scale=None"):
        sl(x, w.to(torch.bfloat16), scale, bias)
    with pytest.raises(ValueError):
        sl(x, w, scale[:-1].contiguous(), bias)


# --------------------------------------------------------------- model wiring
def _tiny(**kw):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    cfg = dict(vocab_size=97, n_layer=2, n_head_q=4, n_head_kv=2, n_embd=64,
               ffn_hidden=128, sequence_length=32, seed=1, dropout=0.0)
    cfg.update(kw)
    return GPT2LLM(GPT2LLMConfig(**cfg)).to(torch.bfloat16).eval()


def _dequantized_copy(model):
    """A deep copy whose linears carry scale * wq as their bf16 weights and
    no prepared weights: the reference on the existing route."""
    from modalities_amd.ops.decode_linear import get_prepared
    ref = copy.deepcopy(model)
    ref.clear_decode_weights()
    with torch.no_grad():
        for a, b in zip(model._decode_linears(), ref._decode_linears()):
            p = get_prepared(a)
            if p is not None and p.scale is not None:
                deq = (p.w.float() * p.scale[:, None]).to(b.weight.dtype)
                if b.weight is ref.wte.weight:
                    # tied head: the embedding lookup keeps the bf16 table
                    b.weight = torch.nn.Parameter(deq)
                else:
                    b.weight.copy_(deq)
    return ref


MODEL_VARIANTS = {
    "fused_swiglu": dict(fused_qkv=True),
    "split_swiglu_unpacked": dict(fused_qkv=False, packed_swiglu=False),
    "fused_gelu_bias": dict(fused_qkv=True, activation_type="gelu", bias=True),
    "split_gelu_tied": dict(fused_qkv=False, activation_type="gelu",
                            use_weight_tying=True),
}


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "bf16"])
@pytest.mark.parametrize("name", sorted(MODEL_VARIANTS))
def test_prepared_model_matches_dequantized_copy(name, fmt, monkeypatch):
    from modalities_amd.ops import decode_linear as dl
    model = _tiny(**MODEL_VARIANTS[name])
    if MODEL_VARIANTS[name].get("bias"):
        with torch.no_grad():
            for lin in model._decode_linears():
                if lin.bias is not None:
                    lin.bias.normal_(0, 0.1)
    model.prepare_decode_weights(fmt)
    assert model.decode_weight_format == fmt
    n_lin = len(model._decode_linears())
    assert all(dl.get_prepared(l) is not None
               for l in model._decode_linears())
    if name == "split_gelu_tied" and fmt == "fp8_e4m3":
        p = dl.get_prepared(model.lm_head)
        wq, _ = dl.quantize_weight_fp8(model.wte.weight)
        assert torch.equal(p.w.view(torch.uint8), wq.view(torch.uint8))
    ref = _dequantized_copy(model)
    assert ref.decode_weight_format is None

    calls = []
    real = dl.skinny_linear
    monkeypatch.setattr(dl, "skinny_linear",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, 97, (2, 5), generator=g)
    ca, cb = model.new_kv_cache(2, max_len=16), ref.new_kv_cache(2, max_len=16)
    # the prefill stays on the resident bf16 weights, so both caches are
    # filled by `model`; only the single-token steps differ between the two
    out = model.forward_cached({"input_ids": prompt}, ca)["logits"]
    want = model.forward_cached({"input_ids": prompt}, cb)["logits"]
    assert not calls, "the prefill must stay on the bf16 weights"
    assert torch.equal(out, want)
    for _ in range(8):
        nxt = want[:, -1, :].argmax(-1, keepdim=True)
        out = model.forward_cached({"input_ids": nxt}, ca)["logits"]
        want = ref.forward_cached({"input_ids": nxt}, cb)["logits"]
        torch.testing.assert_close(out.float(), want.float(),
                                   rtol=2e-2, atol=2e-2)
    assert len(calls) == 8 * n_lin, (len(calls), n_lin)


def test_batch_above_eight_and_odd_k_keep_f_linear(monkeypatch):
    from modalities_amd.ops import decode_linear as dl
    model = _tiny(fused_qkv=True)
    model.prepare_decode_weights("fp8_e4m3")
    calls = []
    real = dl.skinny_linear
    monkeypatch.setattr(dl, "skinny_linear",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    plain = _tiny(fused_qkv=True)
    ids = torch.randint(0, 97, (9, 1))
    a = model.forward_cached({"input_ids": ids},
                             model.new_kv_cache(9, max_len=8))["logits"]
    b = plain.forward_cached({"input_ids": ids},
                             plain.new_kv_cache(9, max_len=8))["logits"]
    assert not calls and torch.equal(a, b)
    assert not dl.skinny_eligible(24) and dl.skinny_eligible(48)


def test_train_load_state_dict_and_clear_drop_the_weights():
    from modalities_amd.ops.decode_linear import get_prepared
    model = _tiny()
    keys = set(model.state_dict())

    def prepared():
        return [get_prepared(l) is not None for l in model._decode_linears()]

    model.prepare_decode_weights("fp8_e4m3")
    assert all(prepared()) and all(b.decode_weights for b in model.blocks)
    assert set(model.state_dict()) == keys, "state dict must be untouched"
    model.eval()
    assert all(prepared()), "eval() keeps them"
    model.clear_decode_weights()
    assert not any(prepared()) and model.decode_weight_format is None
    assert not any(b.decode_weights for b in model.blocks)

    model.prepare_decode_weights("bf16")
    model.train()
    assert not any(prepared()) and model.decode_weight_format is None
    model.eval()

    model.prepare_decode_weights("fp8_e4m3")
    model.load_state_dict(copy.deepcopy(model.state_dict()))
    assert not any(prepared()) and model.decode_weight_format is None

    with pytest.raises(ValueError, match="fp8_e4m3"):
        model.prepare_decode_weights("int4")


def test_cleared_model_is_bit_identical_to_a_fresh_one():
    model, fresh = _tiny(), _tiny()
    model.prepare_decode_weights("fp8_e4m3")
    model.clear_decode_weights()
    ids = torch.randint(0, 97, (2, 4))
    ca, cb = model.new_kv_cache(2, max_len=8), fresh.new_kv_cache(2, max_len=8)
    for t in (ids, ids[:, :1], ids[:, 1:2]):
        a = model.forward_cached({"input_ids": t}, ca)["logits"]
        b = fresh.forward_cached({"input_ids": t}, cb)["logits"]
        assert torch.equal(a, b)


def test_sharded_models_are_refused():
    model = _tiny()
    model.blocks[0].mlp.forward = lambda x: x      # what TP/CP install
    with pytest.raises(NotImplementedError, match="sharded"):
        model.prepare_decode_weights("fp8_e4m3")
    model = _tiny()
    lin = model.blocks[1].attn.c_proj
    lin.weight.data = torch.empty(0, dtype=torch.bfloat16)   # engine-held
    with pytest.raises(NotImplementedError, match="engine"):
        model.prepare_decode_weights("fp8_e4m3")


def test_decode_weight_format_reaches_the_model_through_the_config(tmp_path):
    cfg_text = """\
settings:
  referencing_keys: {sample_key: input_ids, prediction_key: logits}
  device: cpu
  sequence_length: 24

model:
  component_key: model
  variant_key: gpt2
  config:
    sample_key: input_ids
    prediction_key: logits
    vocab_size: 260
    n_layer: 2
    n_head_q: 4
    n_head_kv: 4
    n_embd: 64
    ffn_hidden: 128
    sequence_length: 24
    seed: 3

tokenizer:
  component_key: tokenizer
  variant_key: char
  config: {}

text_inference:
  prompt_template: "{text}"
  temperature: 0.0
  decode_weight_format: fp8_e4m3
"""
    cfg = tmp_path / "gen.yaml"
    cfg.write_text(cfg_text)
    from modalities_amd.api import _build_text_inference_component
    from modalities_amd.ops.decode_linear import get_prepared
    comp = _build_text_inference_component(cfg)
    assert comp.decode_weight_format == "fp8_e4m3"
    assert comp.model.decode_weight_format is None, "prepared before use"
    comp.model.to(torch.bfloat16)
    text = comp.generate_tokens("hey")
    assert isinstance(text, str)
    assert comp.model.decode_weight_format == "fp8_e4m3"
    assert all(get_prepared(l) is not None
               for l in comp.model._decode_linears())

    cfg.write_text(cfg_text.replace("  decode_weight_format: fp8_e4m3\n", ""))
    comp = _build_text_inference_component(cfg)
    assert comp.decode_weight_format is None
    comp.generate_tokens("hey")
    assert comp.model.decode_weight_format is None
