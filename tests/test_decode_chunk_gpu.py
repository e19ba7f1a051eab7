"""Multi-token attention over the KV cache (attention_decode_chunk.hip), bf16
and e4m3 caches: against the fp64 oracle of tests/kernel_oracles.py (bounds
unchanged; FP8 over the de-quantised caches), the queries without keys, the
bit-level invariances, and the model route behind set_decode_chunk_tokens."""

import functools

import pytest
import torch

from modalities_amd import ops
from tests import decode_oracles as do
from tests import kernel_oracles as ko
from tests.test_decode_model_gpu import VARIANTS, _model, _prompt
from tests.test_kv_fp8_gpu import _ext, _fp8_caches, _rt

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
FORMATS = ["bf16", "fp8"]


def _inputs(lens, Lmax, T, Hq, Hkv, D, fmt, seed):
    """decode_inputs with T query tokens per row; rows at or beyond a length
    hold NaN. FP8: the caches went through quantise -> de-quantise, so the
    fp64 reference sees the values the kernel sees."""
    inp = do.decode_inputs(lens, Lmax, Hq, Hkv, D, DEV, seed=seed)
    g = ko._gen(seed + 1)
    inp["q"] = ko.bf(torch.randn(len(lens), T, Hq, D, generator=g)).to(DEV)
    if fmt == "fp8":
        inp["kc"], inp["vc"] = _rt(inp["kc"]), _rt(inp["vc"])
    return inp


def _caches(fmt, inp):
    """What the kernel gets: for FP8 (k_codes, k_scale, v_codes, v_scale),
    with NaN codes and NaN scales at or beyond a length."""
    if fmt == "fp8":
        return _fp8_caches(inp["kc"], inp["vc"], inp["lens"])
    return inp["kc"], inp["vc"]


def _run(fmt, q, caches, lens, chunk=0):
    fwd = _ext().decode_attn_chunk_fp8_fwd if fmt == "fp8" \
        else _ext().decode_attn_chunk_fwd
    return fwd(q, *caches, lens, chunk)


def _check(label, inp, o, lse):
    """Row b against attn_ref64 over its n visible cache rows; the queries
    t < T - n see no key: zeros and -inf."""
    T = inp["q"].shape[1]
    for b, n in enumerate(inp["lens"].tolist()):
        t0 = max(T - n, 0)
        assert not o[b, :t0].any() and (lse[b, :, :t0] == -ko.INF).all()
        if n == 0:
            continue
        assert torch.isfinite(o[b, t0:].float()).all()
        assert torch.isfinite(lse[b, :, t0:]).all()
        case = ko.AttnCase(dict(q=inp["q"][b:b + 1, t0:],
                                k=inp["kc"][b:b + 1, :n],
                                v=inp["vc"][b:b + 1, :n], do=None),
                           off=n - (T - t0), backward=False)
        got = lambda *a: (o[b:b + 1, t0:], lse[b:b + 1, :, t0:])
        ko.require(f"{label}/row{b}/len{n}", ko.check_attn_fwd(got, case)[0])


@pytest.mark.parametrize("T", [2, 5, 16, 17])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (4, 2), (8, 1)])
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_fp64_oracle(D, Hq, Hkv, fmt, T):
    c = _ext().decode_attn_chunk_kv_chunk()
    w = _ext().decode_attn_chunk_wave_keys()
    lens = [T, T + 1, w - 1, w, w + 1, c - 1, c, c + 1, c + T - 1, 2 * c + 17]
    inp = _inputs(lens, 3 * c, T, Hq, Hkv, D, fmt, seed=D + Hq + T)
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"])
    _check(f"chunk/{fmt}/D{D}/h{Hq}:{Hkv}/T{T}", inp, o, lse)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_many_chunks(D, fmt):
    c0 = _ext().decode_attn_chunk_kv_chunk_min()
    inp = _inputs([c0 - 1, c0, c0 + 1, 5 * c0 + 3], 8 * c0, 5, 4, 2, D, fmt,
                  seed=3)
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"], c0)
    _check(f"chunk/{fmt}/chunks/D{D}", inp, o, lse)


@pytest.mark.parametrize("fmt", FORMATS)
def test_queries_without_keys(fmt):
    T = 5
    inp = _inputs([0, 1, T - 1], 64, T, 4, 2, 80, fmt, seed=5)
    o, lse = _run(fmt, inp["q"], _caches(fmt, inp), inp["lens"])
    _check(f"chunk/{fmt}/nokeys", inp, o, lse)


@functools.lru_cache(maxsize=None)
def _shared(fmt):
    c = _ext().decode_attn_chunk_kv_chunk()
    lens = [c - 1, 2 * c + 17, 5]
    inp = _inputs(lens, 3 * c, 5, 4, 2, 80, fmt, seed=11)
    caches = _caches(fmt, inp)
    return lens, inp, caches, _run(fmt, inp["q"], caches, inp["lens"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_stale_rows_and_invariance(fmt):
    lens, inp, caches, (o, lse) = _shared(fmt)
    zeroed = [t.clone() for t in caches]
    for b, n in enumerate(lens):
        for t in zeroed:
            t[b, n:] = 0
    oz, lz = _run(fmt, inp["q"], zeroed, inp["lens"])
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
                      inp["lens"][b:b + 1].contiguous())
        assert torch.equal(o1, o[b:b + 1]) and torch.equal(l1, lse[b:b + 1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_strided_q(fmt):
    lens, inp, caches, (o, lse) = _shared(fmt)
    B, T, Hq, D = inp["q"].shape
    qkv = torch.randn(B, T, (Hq + 2 * 2) * D, device=DEV).bfloat16()
    q = qkv[..., :Hq * D].view(B, T, Hq, D)
    q.copy_(inp["q"])
    assert not q.is_contiguous()
    os_, ls = _run(fmt, q, caches, inp["lens"])
    assert torch.equal(os_, o) and torch.equal(ls, lse)


@pytest.fixture
def chunk_switch():
    was = ops.decode_chunk_tokens()
    yield ops.set_decode_chunk_tokens
    ops.set_decode_chunk_tokens(was)


def _feed_chunks(model, ids, n0, kv_format, round_trip=False):
    """Prefill ids[:, :n0], then feed chunks of 2 and 7 tokens; their
    logits."""
    c = _ext().decode_attn_chunk_kv_chunk()
    out = []
    with torch.no_grad():
        cache = model.new_kv_cache(2, max_len=c + 16, kv_format=kv_format)
        model.forward_cached({"input_ids": ids[:, :n0]}, cache)
        if round_trip:
            for t in cache.k + cache.v:
                t[:, :n0] = _rt(t[:, :n0])
        for T in (2, 7):
            out.append(model.forward_cached(
                {"input_ids": ids[:, cache.pos:cache.pos + T]},
                cache)["logits"])
    return torch.cat(out, 1)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["fused_gqa", "split_mqa", "absolute"])
def test_model_chunk_route(name, fmt, chunk_switch, monkeypatch):
    """bf16: against a full re-forward. FP8: against the bf16 cache holding
    round-tripped rows, so the two runs differ in summation order only."""
    from modalities_amd.models import gpt2
    assert ops.decode_chunk_tokens() == 0, "the switch's default is off"
    model = _model(**VARIANTS[name])
    n0 = _ext().decode_attn_chunk_kv_chunk() - 3
    ids = _prompt(2, n0 + 9)
    real, seen = gpt2.decode_attention, []
    chunk_switch(16)
    if fmt == "bf16":
        with torch.no_grad():
            ref = model({"input_ids": ids})["logits"][:, n0:]
    else:
        def attend_round_tripped(q, kc, vc, lens):
            n, T = int(lens[0]), q.shape[1]
            kc[:, n - T:n], vc[:, n - T:n] = (_rt(kc[:, n - T:n]),
                                              _rt(vc[:, n - T:n]))
            return real(q, kc, vc, lens)
        monkeypatch.setattr(gpt2, "decode_attention", attend_round_tripped)
        ref = _feed_chunks(model, ids, n0, None, round_trip=True)

    def spy(q, *a, **k):
        seen.append(q.shape[1])
        return real(q, *a, **k)
    monkeypatch.setattr(gpt2, "decode_attention", spy)
    got = _feed_chunks(model, ids, n0, None if fmt == "bf16" else "fp8_e4m3")
    assert seen == [2, 2, 7, 7]          # two layers per chunk
    torch.testing.assert_close(got.float(), ref.float(), rtol=2e-2, atol=2e-2)
