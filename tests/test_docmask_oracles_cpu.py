"""CPU tests for document-masked attention: the `document_starts` helper,
the power of the checkers in tests/docmask_oracles.py (they accept the
correct emulation and reject each deliberate mutant), and the model-level
contract of `attention_document_masking` on every attention path.

The model-level leakage tests fail without the feature: plain causal
attention lets document B read document A."""

import pytest
import torch

from tests import docmask_oracles as do_
from tests import kernel_oracles as ko

from modalities_amd.exceptions import ConfigError
from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
from modalities_amd.ops.attention import (_attention_ref, document_ends,
                                          document_starts, flash_attention)

EOD = 7


# ------------------------------------------------------------ document_starts
def _ids(rows):
    return torch.tensor(rows, dtype=torch.int64)


DOC_START_CASES = {
    "no_eod": _ids([[1, 2, 3, 4, 5, 6]]),
    "eod_at_0": _ids([[EOD, 2, 3, 4, 5, 6]]),
    "eod_at_last": _ids([[1, 2, 3, 4, 5, EOD]]),
    "consecutive_eods": _ids([[1, EOD, EOD, EOD, 5, 6, EOD, 1]]),
    "every_token_eod": _ids([[EOD] * 9]),
    "single_token": _ids([[EOD]]),
    "batch_2_layouts": _ids([[1, 2, EOD, 4, 5, 6, EOD, 8, 9, 1],
                             [EOD, 2, 3, 4, 5, EOD, EOD, 8, 9, EOD]]),
}


@pytest.mark.parametrize("name", list(DOC_START_CASES))
def test_document_starts_matches_the_definition(name):
    ids = DOC_START_CASES[name]
    got = document_starts(ids, EOD)
    want = do_.python_document_starts(ids, EOD)
    assert got.dtype == torch.int32 and got.shape == ids.shape
    assert got.is_contiguous()
    assert torch.equal(got, want), (got, want)
    T = ids.shape[1]
    pos = torch.arange(T, dtype=torch.int32)[None]
    assert (got <= pos).all() and (got >= 0).all()
    assert (got[:, 1:] >= got[:, :-1]).all()
    # the key-side mirror the backward kernels take
    assert torch.equal(document_ends(got), do_.start_to_end(got))


def test_document_ends_of_layouts():
    start = do_.layouts_to_start([[0, 3, 4], [0]], 8)
    assert document_ends(start).tolist() == [[2, 2, 2, 3, 7, 7, 7, 7],
                                             [7] * 8]
    assert document_ends(start).dtype == torch.int32


# --------------------------------------------------- checkers vs. the mutants
# B = 2 with different layouts; document starts off the 64-key tile edge
T_CPU, D_CPU = 200, 16
LAYOUTS_CPU = [[0, 70, 71, 150], [0, 33, 130]]


def _cpu_case(dlse=False):
    inp = ko.attn_random_inputs(2, T_CPU, T_CPU, 4, 2, D_CPU, "cpu", seed=11)
    start = do_.layouts_to_start(LAYOUTS_CPU, T_CPU)
    g = None
    if dlse:
        g = torch.randn(2, 4, T_CPU, generator=ko._gen(5))
    return do_.DocCase(inp, start, dlse=g)


@pytest.fixture(scope="module")
def cpu_case():
    return _cpu_case()


def test_checkers_accept_the_emulation(cpu_case):
    r, o, lse = do_.check_doc_fwd(do_.torch_doc_fwd, cpu_case)
    ko.require("doc/cpu/fwd", r)
    ko.require("doc/cpu/bwd", do_.check_doc_bwd(do_.torch_doc_bwd, cpu_case))


def test_checkers_accept_the_emulation_with_dlse():
    case = _cpu_case(dlse=True)
    bwd = lambda *a: do_.torch_doc_bwd(*a[:8], dlse=a[8])
    ko.require("doc/cpu/bwd_dlse", do_.check_doc_bwd(bwd, case))
    # ... and the dlse term is not decorative
    drop = lambda *a: do_.torch_doc_bwd(*a[:8])
    assert ko.rejected(do_.check_doc_bwd(drop, case))


def test_reference_agrees_with_the_wrapper_cpu_path(cpu_case):
    c = cpu_case
    o = _attention_ref(c.q, c.k, c.v, True, doc_start=c.start)
    assert ko.ratio((o.double() - c.ref["o"]).abs(),
                    3 * ko.BF16_ULP * c.ref["absPV"] + ko.F32_TINY) <= 1
    assert torch.equal(o, flash_attention(c.q, c.k, c.v, doc_start=c.start))


@pytest.mark.parametrize("mut", do_.FWD_MUTANTS)
def test_forward_checker_rejects(cpu_case, mut):
    f = lambda q, k, v, s: do_.torch_doc_fwd(q, k, v, s, mut=mut)
    r, _, _ = do_.check_doc_fwd(f, cpu_case)
    print(mut, r)
    assert ko.rejected(r)


@pytest.mark.parametrize("mut", do_.BWD_MUTANTS)
def test_backward_checker_rejects(cpu_case, mut):
    f = lambda *a: do_.torch_doc_bwd(*a, mut=mut)
    r = do_.check_doc_bwd(f, cpu_case)
    print(mut, r)
    assert ko.rejected(r)


def test_counting_checker():
    start = do_.layouts_to_start(LAYOUTS_CPU, T_CPU)
    ok = do_.check_doc_counting(do_.torch_doc_fwd, D_CPU, start, "cpu")
    ko.require("doc/cpu/count", ok)
    for mut in do_.FWD_MUTANTS:
        f = lambda q, k, v, s: do_.torch_doc_fwd(q, k, v, s, mut=mut)
        assert ko.rejected(do_.check_doc_counting(f, D_CPU, start, "cpu")), mut


# ------------------------------------------------------------- wrapper errors
def test_wrapper_validates_doc_start_on_cpu():
    q = torch.randn(2, 8, 2, 16)
    ds = torch.zeros(2, 8, dtype=torch.int32)
    flash_attention(q, q, q, doc_start=ds)
    with pytest.raises(TypeError, match="int32"):
        flash_attention(q, q, q, doc_start=ds.long())
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        flash_attention(q, q, q, doc_start=ds[:, :7].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        flash_attention(q, q, q, doc_start=torch.zeros(
            8, 2, dtype=torch.int32).t())
    with pytest.raises(ValueError, match="causal"):
        flash_attention(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(ValueError, match="q_offset"):
        flash_attention(q, q, q, q_offset=1, doc_start=ds)
    with pytest.raises(ValueError, match="Tq == Tkv"):
        flash_attention(q[:, :4], q, q, doc_start=ds[:, :4].contiguous())


# ---------------------------------------------------------------- model level
VOCAB = 64


def _tiny(impl, fused, masking, **kw):
    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=VOCAB, n_layer=2, n_head_q=4, n_head_kv=2,
                        n_embd=32, ffn_hidden=64, sequence_length=32,
                        attention_implementation=impl, fused_qkv=fused,
                        attention_document_masking=masking,
                        eod_token_id=EOD if masking else None, **kw)
    return GPT2LLM(cfg).float()


def _abc():
    """[A, eod, B] twice: same B, A's tokens replaced by other tokens."""
    a1 = [10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    a2 = [30, 31, 32, 33, 34, 35, 36, 37, 38, 39]
    b = [20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 20, 21]
    ids1 = torch.tensor([a1 + [EOD] + b])
    ids2 = torch.tensor([a2 + [EOD] + b])
    return ids1, ids2, len(a1) + 1


IMPL_FUSED = [(i, f) for i in ("hip_flash", "pytorch_flash", "manual")
              for f in (False, True)]


@pytest.mark.parametrize("impl,fused", IMPL_FUSED)
def test_model_documents_do_not_leak(impl, fused):
    ids1, ids2, nb = _abc()
    model = _tiny(impl, fused, True)
    with torch.no_grad():
        l1 = model({"input_ids": ids1})["logits"]
        l2 = model({"input_ids": ids2})["logits"]
    # masked scores are exactly -inf, so masked weights are exactly 0
    assert torch.equal(l1[:, nb:], l2[:, nb:])
    assert not torch.equal(l1[:, :nb], l2[:, :nb])

    model.zero_grad()
    out = model({"input_ids": ids1})["logits"]
    out[:, nb:].float().square().sum().backward()
    g = model.wte.weight.grad
    only_in_a = list(range(10, 20))
    assert g[20:30].abs().max() > 0
    assert torch.equal(g[only_in_a], torch.zeros_like(g[only_in_a]))


@pytest.mark.parametrize("impl,fused", IMPL_FUSED)
def test_model_flag_off_documents_leak(impl, fused):
    ids1, ids2, nb = _abc()
    model = _tiny(impl, fused, False)
    with torch.no_grad():
        l1 = model({"input_ids": ids1})["logits"]
        l2 = model({"input_ids": ids2})["logits"]
    assert not torch.equal(l1[:, nb:], l2[:, nb:])


def test_model_absolute_positions_keep_window_positions():
    ids1, ids2, nb = _abc()
    model = _tiny("manual", False, True, poe_type="ABSOLUTE",
                  qkv_transform="IdentityTransform")
    with torch.no_grad():
        l1 = model({"input_ids": ids1})["logits"]
        l2 = model({"input_ids": ids2})["logits"]
        alone = model({"input_ids": ids1[:, nb:]})["logits"]
    assert torch.equal(l1[:, nb:], l2[:, nb:])
    # positions are NOT reset: B alone (positions 0..) differs from B in
    # the window (positions nb..)
    assert not torch.allclose(l1[:, nb:], alone)


def test_forward_cached_ignores_the_flag():
    ids1, _, _ = _abc()
    on, off = _tiny("manual", False, True), _tiny("manual", False, False)
    off.load_state_dict(on.state_dict())
    with torch.no_grad():
        a = on.forward_cached({"input_ids": ids1}, on.new_kv_cache(1))
        b = off.forward_cached({"input_ids": ids1}, off.new_kv_cache(1))
    assert torch.equal(a["logits"], b["logits"])


def test_config_validator():
    base = dict(vocab_size=VOCAB, n_layer=1, n_head_q=2, n_head_kv=2,
                n_embd=16, ffn_hidden=32, sequence_length=8)
    assert GPT2LLMConfig(**base).attention_document_masking is False
    assert GPT2LLMConfig(**base).eod_token_id is None
    GPT2LLMConfig(**base, eod_token_id=3)            # harmless without flag
    GPT2LLMConfig(**base, attention_document_masking=True,
                  eod_token_id=VOCAB - 1)
    with pytest.raises(ValueError, match="eod_token_id"):
        GPT2LLMConfig(**base, attention_document_masking=True)
    with pytest.raises(ValueError, match="vocab_size"):
        GPT2LLMConfig(**base, attention_document_masking=True,
                      eod_token_id=VOCAB)
    with pytest.raises(ValueError, match="vocab_size"):
        GPT2LLMConfig(**base, attention_document_masking=True,
                      eod_token_id=-1)


def test_parallel_wrappers_refuse_the_flag():
    from modalities_amd.parallel.cp import get_gpt2_context_parallel_model
    from modalities_amd.parallel.pp import split_model_into_stages
    from modalities_amd.parallel.pp_split import split_model_into_stages_by_fqn
    from modalities_amd.parallel.tp import get_gpt2_tensor_parallelized_model
    model = _tiny("manual", False, True)
    with pytest.raises(ConfigError, match="attention_document_masking"):
        get_gpt2_tensor_parallelized_model(model, tp_rank=0, tp_size=2)
    with pytest.raises(ConfigError, match="attention_document_masking"):
        get_gpt2_context_parallel_model(model, cp_rank=0, cp_size=2)
    with pytest.raises(ConfigError, match="attention_document_masking"):
        split_model_into_stages(model, 2)
    with pytest.raises(ConfigError, match="attention_document_masking"):
        split_model_into_stages_by_fqn(model, 2)
    # without the flag the same calls go through
    split_model_into_stages(_tiny("manual", False, False), 2)


def test_positional_three_argument_block_call():
    model = _tiny("manual", False, True)
    x = torch.randn(1, 8, 32)
    cos, sin = model._rope(8, x.device)
    block = model.blocks[0]
    y = block(x, cos, sin)
    assert torch.equal(y, block(x, cos, sin, doc_start=None))
    assert torch.equal(block.attn(x, cos, sin), block.attn(x, cos, sin, None))
    ds = torch.zeros(1, 8, dtype=torch.int32)
    # one document == plain causal
    assert torch.allclose(y, block(x, cos, sin, doc_start=ds), atol=1e-6)
