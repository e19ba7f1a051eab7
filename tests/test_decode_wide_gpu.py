"""Attention of long token chunks over the KV cache
(attention_decode_wide.hip), bf16 and e4m3 caches: against the fp64 oracle of
tests/kernel_oracles.py (bounds unchanged; FP8 over the de-quantised caches),
the queries without keys, the bit-level invariances, the border inside
ops.decode_attention and the model route."""

import functools

import pytest
import torch

from modalities_amd import ops
from modalities_amd.ops import attention as oa
from tests import decode_oracles as do
from tests.test_decode_chunk_gpu import (DEV, FORMATS, NAN, _caches, _check,
                                         _inputs, chunk_switch)  # noqa: F401
from tests.test_decode_model_gpu import VARIANTS, _model, _prompt
from tests.test_kv_fp8_gpu import _ext

pytestmark = pytest.mark.gpu


def _run(fmt, q, caches, lens, chunk=0, kernel="wide"):
    return getattr(_ext(), f"decode_attn_{kernel}_fp8_fwd" if fmt == "fp8"
                   else f"decode_attn_{kernel}_fwd")(q, *caches, lens, chunk)


@pytest.mark.parametrize("Hq,Hkv,T", [(2, 2, 33), (8, 1, 9), (4, 2, 64)])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_fp64_oracle(D, fmt, Hq, Hkv, T):
    """66, 72 and 128 query rows per kv head: a second block of 2 rows, tiles
    that mix tokens and heads of a group, exactly two blocks."""
    assert _ext().decode_attn_wide_rows() == 64
    c = _ext().decode_attn_wide_kv_chunk_min()
    s = _ext().decode_attn_wide_key_step()
    lens = [T, T + 1, s - 1, s, s + 1, c - 1, c, c + 1, c + T - 1, 2 * c + 17]
    inp = _inputs(lens, 3 * c, T, Hq, Hkv, D, fmt, seed=D + Hq + T)
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"], c)
    _check(f"wide/{fmt}/D{D}/h{Hq}:{Hkv}/T{T}", inp, o, lse)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_many_steps(D, fmt):
    """Chunks of 4 key steps: both staging buffers, loads two steps ahead,
    walks that end inside a step and chunks cut short by the bound."""
    s = _ext().decode_attn_wide_key_step()
    lens = [2 * s - 1, 3 * s + 5, 4 * s, 4 * s + 1, 9 * s + 3]
    inp = _inputs(lens, 10 * s, 20, 4, 2, D, fmt, seed=D)    # 40 rows
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"], 4 * s)
    _check(f"wide/{fmt}/steps/D{D}", inp, o, lse)


@pytest.mark.parametrize("fmt", FORMATS)
def test_queries_without_keys(fmt):
    T = 40
    inp = _inputs([0, 1, T - 1], 64, T, 4, 2, 80, fmt, seed=5)
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"])
    _check(f"wide/{fmt}/nokeys", inp, o, lse)


@functools.lru_cache(maxsize=None)
def _shared(fmt):
    c = _ext().decode_attn_wide_kv_chunk_min()
    lens = [c - 1, 2 * c + 17, 45]
    inp = _inputs(lens, 3 * c, 21, 4, 2, 80, fmt, seed=11)   # 42 rows
    caches = _caches(fmt, inp)
    return c, lens, inp, caches, _run(fmt, inp["q"], caches, inp["lens"], c)


@pytest.mark.parametrize("fmt", FORMATS)
def test_stale_rows_and_invariance(fmt):
    c, lens, inp, caches, (o, lse) = _shared(fmt)
    zeroed = [t.clone() for t in caches]
    for b, n in enumerate(lens):
        for t in zeroed:
            t[b, n:] = 0
    oz, lz = _run(fmt, inp["q"], zeroed, inp["lens"], c)
    assert torch.equal(o, oz) and torch.equal(lse, lz)
    for b, n in enumerate(lens):
        # alone in its batch, in a cache twice as long, NaN beyond the length
        two = []
        for t in caches:
            big = torch.full((1, 2 * t.shape[1]) + tuple(t.shape[2:]), NAN,
                             device=DEV).to(t.dtype)
            big[:, :n] = t[b:b + 1, :n]
            two.append(big)
        o1, l1 = _run(fmt, inp["q"][b:b + 1].contiguous(), two,
                      inp["lens"][b:b + 1].contiguous(), c)
        assert torch.equal(o1, o[b:b + 1]) and torch.equal(l1, lse[b:b + 1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_strided_q(fmt):
    c, lens, inp, caches, (o, lse) = _shared(fmt)
    B, T, Hq, D = inp["q"].shape
    qkv = torch.randn(B, T, (Hq + 2 * 2) * D, device=DEV).bfloat16()
    q = qkv[..., :Hq * D].view(B, T, Hq, D)
    q.copy_(inp["q"])
    assert not q.is_contiguous()
    os_, ls = _run(fmt, q, caches, inp["lens"], c)
    assert torch.equal(os_, o) and torch.equal(ls, lse)


@pytest.mark.parametrize("fmt", FORMATS)
def test_public_route_border(fmt):
    """ops.decode_attention: the wide entry from the border up, the chunk
    entry one row below it, bit for bit (Hq == Hkv: rows == T)."""
    border = oa._DECODE_WIDE_MIN_ROWS
    for T, kernel in ((border, "wide"), (border - 1, "chunk")):
        inp = _inputs([T + 70, T, 3], T + 80, T, 2, 2, 64, fmt, seed=T)
        caches = _caches(fmt, inp)
        if fmt == "fp8":
            kq, ks, vq, vs = caches
            got = ops.decode_attention(inp["q"], kq, vq, inp["lens"],
                                       k_scale=ks, v_scale=vs)
        else:
            got = ops.decode_attention(inp["q"], *caches, inp["lens"])
        want, _ = _run(fmt, inp["q"], caches, inp["lens"], kernel=kernel)
        assert torch.equal(got, want), kernel


@pytest.mark.parametrize("fmt", FORMATS)
def test_model_wide_route(fmt, chunk_switch, monkeypatch):  # noqa: F811
    """A chunk of 40 tokens (80 query rows per kv head) after a prefill.
    bf16: against a full re-forward. FP8: against the chunk kernel serving
    the same step (both read quantised rows). Tolerance of
    test_model_chunk_route."""
    from modalities_amd.models import gpt2
    model = _model(**VARIANTS["fused_gqa"])
    n0, T = 70, 40
    ids = _prompt(2, n0 + T)
    chunk_switch(64)
    monkeypatch.setattr(oa, "_DECODE_WIDE_MIN_ROWS", 33)   # 80 rows: wide
    real, seen = gpt2.decode_attention, []

    def spy(q, *a, **k):
        seen.append(q.shape[1])
        return real(q, *a, **k)
    monkeypatch.setattr(gpt2, "decode_attention", spy)

    def feed():
        with torch.no_grad():
            cache = model.new_kv_cache(
                2, max_len=n0 + T + 8,
                kv_format=None if fmt == "bf16" else "fp8_e4m3")
            model.forward_cached({"input_ids": ids[:, :n0]}, cache)
            return model.forward_cached({"input_ids": ids[:, n0:]},
                                        cache)["logits"]
    got = feed()
    assert seen == [T, T]                              # two layers
    if fmt == "bf16":
        with torch.no_grad():
            ref = model({"input_ids": ids})["logits"][:, n0:]
    else:
        monkeypatch.setattr(oa, "_DECODE_WIDE_MIN_ROWS", 1 << 30)
        ref = feed()
    torch.testing.assert_close(got.float(), ref.float(), rtol=2e-2, atol=2e-2)
