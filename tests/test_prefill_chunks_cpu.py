"""TextInferenceComponent(prefill_chunk_tokens=n): a prompt fed to the KV
cache in chunks generates what the prompt in one piece generates."""

import pytest
import torch

from modalities_amd import ops
from modalities_amd.inference.text_generation import TextInferenceComponent
from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
from modalities_amd.tokenization.tokenizer_wrapper import CharTokenizer


def _tiny():
    torch.manual_seed(3)
    return GPT2LLM(GPT2LLMConfig(
        vocab_size=260, n_layer=2, n_embd=64, n_head_q=4, n_head_kv=2,
        ffn_hidden=128, sequence_length=32, seed=7, dropout=0.0)).eval()


def test_chunked_prefill_generates_the_same_text():
    kw = dict(prompt_template="{text}", sequence_length=32, temperature=0.0)
    model, seen = _tiny(), []
    real = model.forward_cached
    model.forward_cached = lambda inputs, cache: (
        seen.append(inputs["input_ids"].shape[1]) or real(inputs, cache))
    whole = TextInferenceComponent(model, CharTokenizer(), **kw)
    chunked = TextInferenceComponent(model, CharTokenizer(),
                                     prefill_chunk_tokens=5, **kw)
    was = ops.decode_chunk_tokens()
    a = whole.generate_tokens("hello, world")          # 12 tokens
    assert seen[0] == 12
    del seen[:]
    b = chunked.generate_tokens("hello, world")
    assert seen[:4] == [5, 5, 2, 1]
    assert a == b and len(a) > 0
    assert ops.decode_chunk_tokens() == was


@pytest.mark.parametrize("bad", [1, -3, 2.5, True])
def test_bad_prefill_chunk_tokens(bad):
    with pytest.raises(ValueError, match="prefill_chunk_tokens"):
        TextInferenceComponent(_tiny(), CharTokenizer(), "{text}", 32,
                               prefill_chunk_tokens=bad)
