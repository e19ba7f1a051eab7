"""The e4m3 KV cache on the GPU: the quantiser bit for bit against the torch
CPU expression, the quantising append and prefill store against the bf16
ones, the FP8 decode attention against the fp64 oracle of
tests/kernel_oracles.py (bounds unchanged), and the model's decode route."""

import functools

import pytest
import torch

from modalities_amd import ops
from tests import decode_oracles as do
from tests import kernel_oracles as ko
from tests.test_decode_model_gpu import (VARIANTS, _chunk, _model, _prompt,
                                         decode_switch)  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")

# Where the FP8 partial kernel changes path inside a chunk: SLOTS row slots
# (64 at D = 64, 32 at D = 80 / 128), keys taken 4 at a time, then singly.
EDGES = {64: (63, 64, 65, 255, 256, 257),
         80: (31, 32, 33, 127, 128, 129),
         128: (31, 32, 33, 127, 128, 129)}


def _ext():
    from modalities_amd.ops.backend import hip_ext
    return hip_ext()


def _bits(codes):
    return codes.view(torch.uint8).cpu()


def _same(got, want):
    """(codes, scale) pairs, bit for bit."""
    return (torch.equal(_bits(got[0]), _bits(want[0]))
            and torch.equal(got[1].cpu(), want[1].cpu()))


def _rt(x):
    return ops.dequantize_kv_fp8(*ops.quantize_kv_fp8(x))


# -- 1. quantiser ----------------------------------------------------------
def _quantiser_rows(D):
    g = ko._gen(D)
    e = torch.randint(-30, 30, (200, 2, 1), generator=g).float()
    x = (torch.randn(200, 2, D, generator=g) * torch.exp2(e)).bfloat16()
    hand = torch.randn(6, 2, D, generator=g).bfloat16()
    hand[0] *= 0.25
    hand[0, :, 3] = 9600.0          # scale 32: the rest lands in subnormals
    hand[1] = hand[1].clamp(-1, 1) * 8
    hand[1, :, 5] = 448.0 * 8       # amax = 448 * 2^n, n > 0
    hand[2] = hand[2].clamp(-1, 1) / 32
    hand[2, :, D - 1] = -448.0 / 16  # and n < 0
    hand[3, :, 0] = -0.0
    hand[4] = torch.where(hand[4] > 0, 5.0, -5.0).bfloat16()   # +-amax
    return torch.cat([x, hand])


@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_quantiser_bit_for_bit(D):
    x = _quantiser_rows(D)
    want = ops.quantize_kv_fp8(x)            # the torch expression, CPU
    assert _same(ops.quantize_kv_fp8(x.to(DEV)), want)
    # strided: k as a view into a fused-QKV activation [B, T, (Hq + 2 Hkv) D]
    qkv = torch.randn(2, 103, 5 * D, device=DEV).bfloat16()
    k = qkv[..., 2 * D:4 * D].view(2, 103, 2, D)
    assert not k.is_contiguous()
    assert _same(ops.quantize_kv_fp8(k), ops.quantize_kv_fp8(k.cpu()))


def test_quantiser_zero_row():
    x = _quantiser_rows(64).to(DEV)
    x[17, 1] = 0
    codes, scale = ops.quantize_kv_fp8(x)
    assert scale[17, 1] == 1 and torch.count_nonzero(_bits(codes[17, 1])) == 0


# -- 2. append and prefill store -------------------------------------------
def _fp8_sentinels(inp):
    """FP8 caches holding the quantised sentinel pattern of the bf16 ones."""
    (kq, ks), (vq, vs) = (ops.quantize_kv_fp8(inp[n]) for n in ("kc", "vc"))
    return kq, vq, ks, vs


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 80), (3, 3, 128)])
def test_append_equals_quantised_bf16_append(Hq, Hkv, D, rope):
    """Same q; the whole FP8 cache equals the quantised bf16 cache, so the
    appended row is quantize(bf16 row) and every other row is untouched."""
    Lmax = 48
    inp = do.rope_append_inputs([0, Lmax - 1, 7, Lmax, Lmax + 9, -1, 31],
                                Lmax, Hq, Hkv, D, DEV, seed=D, rope=rope)
    kq, vq, ks, vs = _fp8_sentinels(inp)
    args = [inp[n] for n in ("q", "k", "v", "cos", "sin", "pos")]
    q_bf = ops.decode_rope_append(*args, inp["kc"], inp["vc"])
    q_f8 = ops.decode_rope_append(*args, kq, vq, k_scale=ks, v_scale=vs)
    assert torch.equal(q_f8, q_bf)
    assert _same((kq, ks), ops.quantize_kv_fp8(inp["kc"].cpu()))
    assert _same((vq, vs), ops.quantize_kv_fp8(inp["vc"].cpu()))


@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_prefill_store_equals_quantised_bf16_store(D, T):
    """37 rows x 2 heads x 2 batch rows fill no whole workgroup."""
    Lmax, pos, Hkv = 48, 5, 2
    inp = do.rope_append_inputs([0, 0], Lmax, 2, Hkv, D, DEV, seed=T)
    kq, vq, ks, vs = _fp8_sentinels(inp)
    qkv = torch.randn(2, T, 4 * D, device=DEV).bfloat16()
    k = qkv[..., D:3 * D].view(2, T, Hkv, D)
    v = qkv[..., :2 * D].view(2, T, Hkv, D)
    ops.kv_quantize_store(k, v, kq, vq, ks, vs, pos)
    inp["kc"][:, pos:pos + T], inp["vc"][:, pos:pos + T] = k, v
    assert _same((kq, ks), ops.quantize_kv_fp8(inp["kc"].cpu()))
    assert _same((vq, vs), ops.quantize_kv_fp8(inp["vc"].cpu()))


# -- 3. attention against fp64 ---------------------------------------------
def _fp8_caches(kc, vc, lens):
    """Codes and scales of bf16 caches; at or beyond a length both are NaN."""
    (kq, ks), (vq, vs) = ops.quantize_kv_fp8(kc), ops.quantize_kv_fp8(vc)
    for b, n in enumerate(lens.tolist()):
        ks[b, max(n, 0):] = NAN
        vs[b, max(n, 0):] = NAN
    return kq, ks, vq, vs


def _dec(q, kc, vc, lens, chunk=0):
    return _ext().decode_attn_fp8_fwd(q, *_fp8_caches(kc, vc, lens), lens,
                                      chunk)


def _inputs(lens, Lmax, Hq, Hkv, D, seed):
    """decode_inputs whose caches went through quantise -> de-quantise: the
    fp64 reference sees the values the kernel sees (stale rows stay NaN)."""
    inp = do.decode_inputs(lens, Lmax, Hq, Hkv, D, DEV, seed=seed)
    inp["kc"], inp["vc"] = _rt(inp["kc"]), _rt(inp["vc"])
    return inp


def _require_all(label, res):
    for k, r in res.items():
        ko.require(f"{label}/{k}", r)


@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_fp64_oracle(D, Hq, Hkv):
    c = _chunk()
    lens = sorted({1, 2, c - 1, c, c + 1, 2 * c + 1} | set(EDGES[D]))
    Lmax = 2 * c + 64
    inp = _inputs(lens, Lmax, Hq, Hkv, D, seed=D + Hq)
    res, o, lse = do.check_decode_rows(_dec, inp, 0)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    _require_all(f"fp8/D{D}/h{Hq}:{Hkv}", res)
    _require_all(f"fp8/D{D}/h{Hq}:{Hkv}", do.check_decode_counting(
        _dec, D, lens, Lmax, 0, DEV, Hq=Hq, Hkv=Hkv))


@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_many_chunks(D):
    c0 = _ext().decode_attn_kv_chunk_min()
    lens = [c0 - 1, c0, c0 + 1, 5 * c0 + 3]
    inp = _inputs(lens, 8 * c0, 4, 2, D, seed=3)
    res, _, _ = do.check_decode_rows(_dec, inp, c0)
    _require_all(f"fp8/chunks/D{D}", res)
    _require_all(f"fp8/chunks/D{D}", do.check_decode_counting(
        _dec, D, lens, 8 * c0, c0, DEV, Hq=4, Hkv=2))


@pytest.mark.parametrize("rep", [3, 6])
def test_group_sizes_off_the_register_tile(rep):
    """rep = 3 leaves a row of the 4-head tile empty; rep = 6 needs a second
    group of 4 with half of it empty."""
    c = _chunk()
    inp = _inputs([c + 5, 7], 2 * c, rep * 2, 2, 80, seed=rep)
    res, _, _ = do.check_decode_rows(_dec, inp, 0)
    _require_all(f"fp8/rep{rep}", res)


# -- 4. invariance ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shared(D=80):
    c = _chunk()
    lens = [c - 1, 2 * c + 17, 5]
    inp = do.decode_inputs(lens, 3 * c, 4, 2, D, DEV, seed=11)
    return lens, inp, _fp8_caches(inp["kc"], inp["vc"], inp["lens"])


def test_batch_and_cache_invariance():
    lens, inp, caches = _shared()
    dec = _ext().decode_attn_fp8_fwd
    o, lse = dec(inp["q"], *caches, inp["lens"])
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    for b, n in enumerate(lens):
        q1 = inp["q"][b:b + 1].contiguous()
        n1 = inp["lens"][b:b + 1].contiguous()
        one = [t[b:b + 1].contiguous() for t in caches]
        o1, l1 = dec(q1, *one, n1)
        assert torch.equal(o1, o[b:b + 1]) and torch.equal(l1, lse[b:b + 1])
        # the same row in a cache twice as long, NaN beyond the length
        two = []
        for t in one:
            big = torch.full((1, 2 * t.shape[1]) + tuple(t.shape[2:]), NAN,
                             device=DEV).to(t.dtype)
            big[:, :n] = t[:, :n]
            two.append(big)
        o2, l2 = dec(q1, *two, n1)
        assert torch.equal(o2, o[b:b + 1]) and torch.equal(l2, lse[b:b + 1])


def test_stale_rows_are_never_read():
    lens, inp, caches = _shared()
    dec = _ext().decode_attn_fp8_fwd
    o, lse = dec(inp["q"], *caches, inp["lens"])
    zeroed = [t.clone() for t in caches]
    for b, n in enumerate(lens):
        for t in zeroed:
            t[b, n:] = 0
    oz, lz = dec(inp["q"], *zeroed, inp["lens"])
    assert torch.equal(o, oz) and torch.equal(lse, lz)


# -- 5. model --------------------------------------------------------------
def _decode_8(model, prompt, kv_format, graph=False, tokens=None,
              round_trip=False):
    """Prefill, then 8 steps: greedy, or fed `tokens`. Returns the logits,
    the tokens fed and the cache."""
    from modalities_amd.inference.text_generation import DecodeGraph
    logits, fed = [], []
    with torch.no_grad():
        cache = model.new_kv_cache(2, max_len=_chunk() + 16,
                                   kv_format=kv_format)
        out = model.forward_cached({"input_ids": prompt}, cache)["logits"]
        if round_trip:
            for t in cache.k + cache.v:
                t[:, :cache.pos] = _rt(t[:, :cache.pos])
        g = DecodeGraph(model, cache, "input_ids", "logits") if graph else None
        for i in range(8):
            nxt = out[:, -1, :].argmax(-1, keepdim=True) if tokens is None \
                else tokens[i]
            fed.append(nxt)
            out = g.step(nxt) if g is not None else \
                model.forward_cached({"input_ids": nxt}, cache)["logits"]
            logits.append(out.clone())
    return torch.cat(logits, 1), fed, cache


@pytest.mark.parametrize("name,weights", [
    ("fused_gqa", None), ("split_mqa", None), ("absolute", None),
    ("fused_gqa", "fp8_e4m3")])
def test_model_fp8_cache(name, weights, decode_switch, monkeypatch):  # noqa
    """Reference: the bf16 cache holding round-tripped rows, so the two
    runs differ in summation order only. Graph replay equals eager."""
    from modalities_amd.models import gpt2
    decode_switch(True)
    model = _model(**VARIANTS[name])
    if weights is not None:
        model.prepare_decode_weights(weights)
    prompt = _prompt(2, _chunk() - 3)
    eager, fed, cache_e = _decode_8(model, prompt, "fp8_e4m3")
    replay, _, cache_g = _decode_8(model, prompt, "fp8_e4m3", graph=True)
    assert torch.equal(eager, replay)
    n = cache_e.pos
    assert n == cache_g.pos == _chunk() + 5
    for name_ in ("k", "v", "k_scale", "v_scale"):
        for a, b in zip(getattr(cache_e, name_), getattr(cache_g, name_)):
            assert torch.equal(a[:, :n].view(torch.uint8),
                               b[:, :n].view(torch.uint8))

    real = gpt2.decode_rope_append

    def append_round_tripped(q, k, v, cos, sin, pos, kc, vc):
        out = real(q, k, v, cos, sin, pos, kc, vc)
        rows, p = torch.arange(q.shape[0], device=DEV), pos.long()
        kc[rows, p], vc[rows, p] = _rt(kc[rows, p]), _rt(vc[rows, p])
        return out
    monkeypatch.setattr(gpt2, "decode_rope_append", append_round_tripped)
    ref, _, _ = _decode_8(model, prompt, None, tokens=fed, round_trip=True)
    torch.testing.assert_close(eager.float(), ref.float(), rtol=2e-2,
                               atol=2e-2)
