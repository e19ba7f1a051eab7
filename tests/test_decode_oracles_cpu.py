"""The decode oracles judge themselves on the CPU: the plain-torch emulation
of the split-KV scheme passes every check, each deliberate mutant is
rejected at every shape family that tests/test_decode_attention_gpu.py
runs, and the CPU paths of the new ops agree with the existing
references."""

import functools

import pytest
import torch

from tests import decode_oracles as do
from tests import kernel_oracles as ko

CPU = "cpu"
CHUNK = 256     # what the emulation is chunked by here (the kernel's default)
CHUNK_MIN = 16

MUTANTS = ["len_plus1", "len_minus1", "drop_last_chunk",
           "combine_no_rescale", "gqa_mod", "len_of_row0"]


def _dec(mut):
    return lambda q, kc, vc, lens, chunk: do.torch_decode_attn(
        q, kc, vc, lens, chunk, mut=mut)


def _family(name):
    """(lens, Lmax, chunk, head configs, D) of a GPU shape family."""
    kind, D = name.split("/")
    D = int(D)
    c = CHUNK
    if kind == "oracle":
        return do.oracle_lengths(D, c), 2 * c + 64, c, do.HEADS, D
    if kind == "many_chunks":
        c0 = CHUNK_MIN
        return [c0 - 1, c0, c0 + 1, 5 * c0 + 3], 8 * c0, c0, [(4, 2)], D
    assert kind == "mixed"
    return [1, c + 1, 2 * c + 17], 3 * c, c, [(4, 2)], D


FAMILIES = [f"{k}/{D}" for k in ("oracle", "many_chunks", "mixed")
            for D in do.HEAD_DIMS]


@functools.lru_cache(maxsize=None)
def _inputs(name, heads):
    lens, Lmax, chunk, _, D = _family(name)
    inp = do.decode_inputs(lens, Lmax, heads[0], heads[1], D, CPU,
                           seed=len(name) + heads[0], stale="ones")
    return inp, tuple(do.row_cases(inp))


def _run(name, mut):
    lens, Lmax, chunk, heads, D = _family(name)
    res = {}
    for hs in heads:
        inp, cases = _inputs(name, hs)
        r, _, _ = do.check_decode_rows(_dec(mut), inp, chunk, list(cases))
        res.update({f"{hs}/{k}": v for k, v in r.items()})
    res.update(do.check_decode_counting(_dec(mut), D, lens, Lmax, chunk, CPU,
                                        stale="ones"))
    return res


@pytest.mark.parametrize("name", FAMILIES)
def test_emulation_accepted(name):
    for label, r in _run(name, None).items():
        ko.require(f"cpu/decode/{name}/{label}", r)


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_rejected(name, mut):
    res = _run(name, mut)
    hits = [k for k, r in res.items() if ko.rejected(r)]
    print(mut, name, "rejected by", hits)
    assert hits, f"mutant {mut} passed every checker at {name}"
    if mut in ("len_plus1", "len_minus1"):
        # an off-by-one length moves a count at EVERY length
        assert all(ko.rejected(r) for k, r in res.items()
                   if k.startswith("count/")), res


def test_stale_nan_rows_do_not_reach_the_emulation():
    inp = do.decode_inputs([1, 17, 300], 320, 4, 2, 64, CPU, stale="nan")
    res, o, lse = do.check_decode_rows(_dec(None), inp, CHUNK)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    for label, r in res.items():
        ko.require("cpu/decode/nan/" + label, r)


# ------------------------------------------------------- RoPE + cache append
@pytest.mark.parametrize("rope", [True, False])
def test_rope_append_emulation_and_mutant(rope):
    from modalities_amd.ops.rope import rope_apply
    Lmax = 24
    inp = do.rope_append_inputs([0, Lmax - 1, 7, Lmax, Lmax + 9, -1], Lmax,
                                4, 2, 64, CPU, rope=rope)
    ok = do.check_rope_append(do.torch_rope_append, inp, rope_apply)
    assert all(ok.values()), ok
    bad = do.check_rope_append(
        functools.partial(do.torch_rope_append, mut="append_pos_plus1"),
        inp, rope_apply)
    assert bad["q"] and not bad["k_cache"] and not bad["v_cache"], bad


@pytest.mark.parametrize("rope", [True, False])
def test_decode_rope_append_cpu_path(rope):
    from modalities_amd.ops import decode_rope_append
    from modalities_amd.ops.rope import rope_apply
    Lmax = 24
    inp = do.rope_append_inputs([0, Lmax - 1, 7, Lmax, Lmax + 9, -1], Lmax,
                                4, 2, 80, CPU, rope=rope)
    ok = do.check_rope_append(decode_rope_append, inp, rope_apply)
    assert all(ok.values()), ok


# ------------------------------------------------------------ ops on the CPU
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 80), (2, 2, 128)])
def test_decode_attention_cpu_equals_attention_ref(Hq, Hkv, D):
    from modalities_amd.ops import decode_attention
    from modalities_amd.ops.attention import _attention_ref
    lens = [1, 0, 37, 40, 45]
    inp = do.decode_inputs(lens, 40, Hq, Hkv, D, CPU, stale="nan")
    o = decode_attention(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    assert o.shape == inp["q"].shape and o.dtype == torch.bfloat16
    for b, n in enumerate(lens):
        n = min(n, 40)
        if n == 0:
            assert torch.count_nonzero(o[b]) == 0
            continue
        want = _attention_ref(inp["q"][b:b + 1], inp["kc"][b:b + 1, :n],
                              inp["vc"][b:b + 1, :n], causal=True)
        assert torch.equal(o[b:b + 1], want), (b, n)


def test_decode_attention_bad_arguments_cpu():
    from modalities_amd.ops import decode_attention
    inp = do.decode_inputs([3, 4], 8, 4, 2, 64, CPU)
    q, kc, vc, lens = inp["q"], inp["kc"], inp["vc"], inp["lens"]
    with pytest.raises(TypeError):
        decode_attention(q, kc, vc, lens.long())
    with pytest.raises(ValueError):
        decode_attention(q, kc, vc, lens[:1])
    with pytest.raises(ValueError):
        decode_attention(q, kc, vc[:, :4], lens)
    with pytest.raises(ValueError):
        decode_attention(q[:, :, :3], kc, vc, lens)
    bad = do.decode_inputs([3, 4], 8, 4, 2, 96, CPU)
    with pytest.raises(ValueError, match="head_dim"):
        decode_attention(bad["q"], bad["kc"], bad["vc"], bad["lens"])


def test_decode_switch_round_trip():
    from modalities_amd import ops
    was = ops.decode_attention_enabled()
    try:
        ops.set_decode_attention(False)
        assert not ops.decode_attention_enabled()
        ops.set_decode_attention(True)
        assert ops.decode_attention_enabled()
    finally:
        ops.set_decode_attention(was)


# ------------------------------------------------------------------ KV cache
def _tiny(**kw):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    cfg = dict(vocab_size=97, n_layer=2, n_head_q=4, n_head_kv=2, n_embd=64,
               ffn_hidden=128, sequence_length=32, seed=1, dropout=0.0)
    cfg.update(kw)
    return GPT2LLM(GPT2LLMConfig(**cfg)).eval()


def test_kv_cache_reset_clears_the_device_counters():
    model = _tiny()
    cache = model.new_kv_cache(3, max_len=16)
    for t in (cache.pos_dev, cache.lens_dev):
        assert t.dtype == torch.int32 and tuple(t.shape) == (3,)
    ids = torch.randint(0, 97, (3, 5))
    model.forward_cached({"input_ids": ids}, cache)
    model.forward_cached({"input_ids": ids[:, :1]}, cache)
    assert cache.pos == 6 and cache.pos_dev.tolist() == [6, 6, 6]
    cache.lens_dev.fill_(7)
    cache.reset()
    assert cache.pos == 0
    assert cache.pos_dev.tolist() == [0, 0, 0]
    assert cache.lens_dev.tolist() == [0, 0, 0]
