"""The decode route of GPT2LLM.forward_cached on the GPU: single-token steps
through decode_rope_append + decode_attention, the A/B switch, and the
hipGraph replay of a captured step."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

VARIANTS = {
    "fused_gqa": dict(fused_qkv=True, n_head_q=4, n_head_kv=2),
    "split_gqa": dict(fused_qkv=False, n_head_q=4, n_head_kv=2),
    "fused_mha": dict(fused_qkv=True, n_head_q=8, n_head_kv=8),
    "split_mqa": dict(fused_qkv=False, n_head_q=8, n_head_kv=1),
    "fused_mqa_qknorm": dict(fused_qkv=True, n_head_q=8, n_head_kv=1,
                             use_qk_norm=True),
    "split_gqa_qknorm": dict(fused_qkv=False, n_head_q=4, n_head_kv=2,
                             use_qk_norm=True),
    "absolute": dict(fused_qkv=True, n_head_q=4, n_head_kv=2,
                     poe_type="ABSOLUTE", qkv_transform="IdentityTransform"),
}


def _chunk():
    from modalities_amd.ops.backend import hip_ext
    return hip_ext().decode_attn_kv_chunk()


def _model(vocab=128, **kw):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    torch.manual_seed(3)
    cfg = dict(vocab_size=vocab, n_layer=2, n_embd=512, ffn_hidden=1024,
               sequence_length=_chunk() + 32, seed=7, dropout=0.0)
    cfg.update(kw)
    return GPT2LLM(GPT2LLMConfig(**cfg)).to(DEV).to(torch.bfloat16).eval()


def _prompt(B, T, vocab=128):
    g = torch.Generator().manual_seed(9)
    return torch.randint(0, vocab, (B, T), generator=g).to(DEV)


@pytest.fixture
def decode_switch():
    from modalities_amd import ops
    was = ops.decode_attention_enabled()
    yield ops.set_decode_attention
    ops.set_decode_attention(was)


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_decode_route_matches_full_reforward(name, decode_switch):
    """Prefill c - 3 tokens, then 8 greedy tokens: decoding crosses a chunk
    edge of the decode kernel.  Tolerance of the existing KV-cache test."""
    decode_switch(True)
    model = _model(**VARIANTS[name])
    c = _chunk()
    prompt = _prompt(2, c - 3)
    with torch.no_grad():
        cache = model.new_kv_cache(2, max_len=c + 16)
        model.forward_cached({"input_ids": prompt}, cache)
        ref = model({"input_ids": prompt})["logits"]
        ids = prompt
        for step in range(8):
            nxt = ref[:, -1, :].argmax(-1, keepdim=True)
            ids = torch.cat([ids, nxt], dim=1)
            ref = model({"input_ids": ids})["logits"]
            out = model.forward_cached({"input_ids": nxt}, cache)["logits"]
            assert tuple(out.shape) == (2, 1, 128)
            torch.testing.assert_close(out[:, -1].float(), ref[:, -1].float(),
                                       rtol=2e-2, atol=2e-2)
        assert cache.pos == c + 5
        assert cache.pos_dev.tolist() == [c + 5] * 2
        assert cache.lens_dev.tolist() == [c + 5] * 2


def _decode_8(model, prompt, switch_on, decode_switch, graph=False):
    from modalities_amd.inference.text_generation import DecodeGraph
    decode_switch(switch_on)
    logits = []
    with torch.no_grad():
        cache = model.new_kv_cache(prompt.shape[0], max_len=_chunk() + 16)
        out = model.forward_cached({"input_ids": prompt}, cache)["logits"]
        g = DecodeGraph(model, cache, "input_ids", "logits") if graph else None
        for _ in range(8):
            nxt = out[:, -1, :].argmax(-1, keepdim=True)
            if g is not None:
                out = g.step(nxt)
            else:
                out = model.forward_cached({"input_ids": nxt}, cache)["logits"]
            logits.append(out.clone())
    return torch.cat(logits, 1), cache


@pytest.mark.parametrize("name", ["fused_gqa", "absolute"])
def test_switch_off_is_the_prefill_kernel_route(name, decode_switch,
                                                monkeypatch):
    """With the switch off no decode kernel runs and the logits are those
    of the flash_attention route, bit for bit, whatever ran before."""
    from modalities_amd.models import gpt2
    model = _model(**VARIANTS[name])
    prompt = _prompt(2, _chunk() - 3)
    off1, cache = _decode_8(model, prompt, False, decode_switch)
    assert cache.pos_dev.tolist() == [cache.pos] * 2
    on, _ = _decode_8(model, prompt, True, decode_switch)
    # same prompt, same first token: the two routes agree on its logits
    torch.testing.assert_close(on[:, 0].float(), off1[:, 0].float(),
                               rtol=2e-2, atol=2e-2)

    def boom(*a, **k):
        raise AssertionError("decode kernel reached with the switch off")
    monkeypatch.setattr(gpt2, "decode_attention", boom)
    monkeypatch.setattr(gpt2, "decode_rope_append", boom)
    off2, _ = _decode_8(model, prompt, False, decode_switch)
    assert torch.equal(off1, off2)
    with pytest.raises(AssertionError, match="switch off"):
        _decode_8(model, prompt, True, decode_switch)


@pytest.mark.parametrize("name", ["fused_gqa", "split_mqa", "absolute"])
def test_graph_replay_equals_eager_decode(name, decode_switch):
    model = _model(**VARIANTS[name])
    prompt = _prompt(2, _chunk() - 3)
    eager, cache_e = _decode_8(model, prompt, True, decode_switch)
    replay, cache_g = _decode_8(model, prompt, True, decode_switch, graph=True)
    assert torch.equal(eager, replay)
    assert cache_g.pos == cache_e.pos
    assert torch.equal(cache_g.pos_dev, cache_e.pos_dev)
    n = cache_e.pos
    for a, b in zip(cache_e.k + cache_e.v, cache_g.k + cache_g.v):
        assert torch.equal(a[:, :n], b[:, :n])


def test_generate_tokens_same_text_with_and_without_graph(decode_switch,
                                                          monkeypatch):
    from modalities_amd.inference import text_generation as tg
    from modalities_amd.tokenization.tokenizer_wrapper import CharTokenizer
    decode_switch(True)
    model = _model(vocab=260, fused_qkv=True, n_head_q=4, n_head_kv=2)
    made = []
    real = tg.DecodeGraph

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.steps = 0
            made.append(self)

        def step(self, next_ids):
            self.steps += 1
            return super().step(next_ids)
    monkeypatch.setattr(tg, "DecodeGraph", Spy)
    kw = dict(prompt_template="{text}", sequence_length=24, temperature=0.0,
              device=torch.device(DEV))
    with_graph = tg.TextInferenceComponent(model, CharTokenizer(), **kw)
    without = tg.TextInferenceComponent(model, CharTokenizer(),
                                        use_decode_graph=False, **kw)
    a = with_graph.generate_tokens("hello world")
    assert len(made) == 1, "the decode step was not captured"
    b = without.generate_tokens("hello world")
    assert len(made) == 1
    assert made[0].steps >= 1, "no token came from a graph replay"
    assert a == b
