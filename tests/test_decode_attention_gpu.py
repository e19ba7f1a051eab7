"""Split-KV decode attention and the fused RoPE + cache append on the GPU.

Every case uses a cache much longer than the lengths, and every cache row
at or beyond a row's length holds bf16 NaN: one read past the length
poisons the output.  The fp64 reference and the bounds are those of
tests/kernel_oracles.py (see tests/decode_oracles.py)."""

import functools

import pytest
import torch

from tests import decode_oracles as do
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from modalities_amd.ops.backend import hip_ext
    return hip_ext()


def _dec(q, kc, vc, lens, chunk=0):
    return _ext().decode_attn_fwd(q, kc, vc, lens, chunk)


def _c():
    return _ext().decode_attn_kv_chunk()


def _c0():
    return _ext().decode_attn_kv_chunk_min()


def _require_all(label, res):
    for k, r in res.items():
        ko.require(f"{label}/{k}", r)


@pytest.mark.parametrize("Hq,Hkv", do.HEADS)
@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_fp64_oracle(D, Hq, Hkv):
    """Every length of the list as one batch row (the op takes per-row
    lengths), random data against fp64; then counting V per length."""
    c = _c()
    lens = do.oracle_lengths(D, c)
    Lmax = 2 * c + 64
    inp = do.decode_inputs(lens, Lmax, Hq, Hkv, D, DEV, seed=D + Hq)
    res, o, lse = do.check_decode_rows(_dec, inp, 0)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    _require_all(f"decode/D{D}/h{Hq}:{Hkv}", res)
    _require_all(f"decode/D{D}/h{Hq}:{Hkv}", do.check_decode_counting(
        _dec, D, lens, Lmax, 0, DEV, Hq=Hq, Hkv=Hkv))


@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_many_chunks(D):
    c0 = _c0()
    lens = [c0 - 1, c0, c0 + 1, 5 * c0 + 3]
    inp = do.decode_inputs(lens, 8 * c0, 4, 2, D, DEV, seed=3)
    res, o, lse = do.check_decode_rows(_dec, inp, c0)
    _require_all(f"decode/chunks/D{D}", res)
    _require_all(f"decode/chunks/D{D}", do.check_decode_counting(
        _dec, D, lens, 8 * c0, c0, DEV, Hq=4, Hkv=2))


@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_mixed_lengths(D):
    c = _c()
    inp = do.decode_inputs([1, c + 1, 2 * c + 17], 3 * c, 4, 2, D, DEV, seed=5)
    res, o, lse = do.check_decode_rows(_dec, inp, 0)
    assert tuple(o.shape) == (3, 1, 4, D) and tuple(lse.shape) == (3, 4, 1)
    _require_all(f"decode/mixed/D{D}", res)


@pytest.mark.parametrize("rep", [3, 12])
def test_group_sizes_off_the_register_tile(rep):
    """rep = 3 leaves a row of the 4-row tile empty; rep = 12 needs a second
    group of 8 with half of it empty."""
    c = _c()
    inp = do.decode_inputs([c + 5, 7], 2 * c, rep * 2, 2, 64, DEV, seed=rep)
    res, _, _ = do.check_decode_rows(_dec, inp, 0)
    _require_all(f"decode/rep{rep}", res)


@functools.lru_cache(maxsize=None)
def _shared(D=80):
    c = _c()
    lens = [c - 1, 2 * c + 17, 5]
    return lens, 3 * c, do.decode_inputs(lens, 3 * c, 4, 2, D, DEV, seed=11)


def test_stale_rows_are_never_read():
    lens, Lmax, inp = _shared()
    o, lse = _dec(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    kz, vz = inp["kc"].clone(), inp["vc"].clone()
    for b, n in enumerate(lens):
        kz[b, n:] = 0
        vz[b, n:] = 0
    oz, lz = _dec(inp["q"], kz, vz, inp["lens"])
    assert torch.equal(o, oz) and torch.equal(lse, lz)


def test_batch_and_cache_invariance():
    lens, Lmax, inp = _shared()
    o, lse = _dec(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    for b in range(3):
        q1, k1, v1 = (inp[n][b:b + 1].contiguous() for n in ("q", "kc", "vc"))
        n1 = inp["lens"][b:b + 1].contiguous()
        o1, l1 = _dec(q1, k1, v1, n1)
        assert torch.equal(o1, o[b:b + 1]) and torch.equal(l1, lse[b:b + 1])
        # the same row in a cache twice as long
        k2 = torch.full((1, 2 * Lmax) + tuple(k1.shape[2:]), float("nan"),
                        dtype=k1.dtype, device=DEV)
        v2 = k2.clone()
        k2[:, :lens[b]], v2[:, :lens[b]] = k1[:, :lens[b]], v1[:, :lens[b]]
        o2, l2 = _dec(q1, k2, v2, n1)
        assert torch.equal(o2, o[b:b + 1]) and torch.equal(l2, lse[b:b + 1])


def test_determinism():
    lens, Lmax, inp = _shared()
    a = _dec(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    b = _dec(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("D", do.HEAD_DIMS)
def test_counting_v_across_chunk_edges(D):
    c = _c()
    lens = [c - 1, c, c + 1, 2 * c, 2 * c + 1]
    _require_all(f"decode/count/D{D}", do.check_decode_counting(
        _dec, D, lens, 3 * c, 0, DEV, Hq=8, Hkv=1))


def test_length_zero_and_length_beyond_the_cache():
    """The cache is a view inside a larger NaN buffer: a read before its
    first or past its last row would poison the result."""
    D, Hq, Hkv, Lmax, pad = 64, 4, 2, 40, 8
    lens = [0, Lmax, Lmax + 5, -3, 17]
    inp = do.decode_inputs([0, Lmax, Lmax, 0, 17], Lmax, Hq, Hkv, D, DEV,
                           seed=2)
    big_k = torch.full((5, Lmax + 2 * pad, Hkv, D), float("nan"),
                       dtype=torch.bfloat16, device=DEV)
    big_v = big_k.clone()
    kc, vc = big_k[:, pad:pad + Lmax], big_v[:, pad:pad + Lmax]
    kc.copy_(inp["kc"])
    vc.copy_(inp["vc"])
    n = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = _dec(inp["q"], kc, vc, n)
    assert torch.isfinite(o.float()).all()
    for b in (0, 3):
        assert torch.count_nonzero(o[b]) == 0
        assert (lse[b] == -float("inf")).all()
    assert torch.isfinite(lse[[1, 2, 4]]).all()
    got = lambda b: (lambda q, k, v, off: (o[b:b + 1], lse[b:b + 1]))
    for b, S in ((1, Lmax), (2, Lmax), (4, 17)):
        ko.require(f"decode/clamp/row{b}",
                   ko.check_attn_fwd(got(b), do.row_case(inp, b, S))[0])


def test_strided_q_and_caches():
    """q as a view into a fused-QKV row, caches as head-sliced views of a
    wider buffer: the same bits as contiguous copies."""
    D, Hq, Hkv, Lmax = 128, 4, 2, 300
    lens = [300, 129]
    inp = do.decode_inputs(lens, Lmax, Hq, Hkv, D, DEV, seed=4)
    qkv = torch.randn(2, 1, (Hq + 2 * Hkv) * D, device=DEV).bfloat16()
    qkv[..., :Hq * D] = inp["q"].reshape(2, 1, Hq * D)
    q_view = qkv[..., :Hq * D].view(2, 1, Hq, D)
    wide_k = torch.full((2, Lmax, Hkv + 1, D), float("nan"),
                        dtype=torch.bfloat16, device=DEV)
    wide_v = wide_k.clone()
    wide_k[:, :, :Hkv], wide_v[:, :, :Hkv] = inp["kc"], inp["vc"]
    assert not q_view.is_contiguous()
    a = _dec(q_view, wide_k[:, :, :Hkv], wide_v[:, :, :Hkv], inp["lens"])
    b = _dec(inp["q"], inp["kc"], inp["vc"], inp["lens"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    res, _, _ = do.check_decode_rows(lambda *x: a, inp, 0)
    _require_all("decode/strided", res)


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("Hq,Hkv,D", [(4, 2, 64), (8, 1, 80), (3, 3, 128)])
def test_decode_rope_append(Hq, Hkv, D, rope):
    """q, k, v are views into a fused-QKV row.  Bit-identical to rope_apply
    on the sliced tables plus an indexed copy; rows with pos outside
    [0, Lmax) leave the sentinel-filled cache untouched."""
    from modalities_amd.ops import decode_rope_append
    from modalities_amd.ops.rope import rope_apply
    Lmax = 48
    inp = do.rope_append_inputs([0, Lmax - 1, 7, Lmax, Lmax + 9, -1, 31],
                                Lmax, Hq, Hkv, D, DEV, seed=D, rope=rope)
    assert not inp["k"].is_contiguous()
    ok = do.check_rope_append(decode_rope_append, inp, rope_apply)
    assert all(ok.values()), ok


def test_decode_rope_append_into_strided_cache():
    from modalities_amd.ops import decode_rope_append
    from modalities_amd.ops.rope import rope_apply
    Lmax, pad = 16, 4
    inp = do.rope_append_inputs([3, Lmax - 1, 0], Lmax, 4, 2, 64, DEV)
    big = [torch.zeros(3, Lmax + 2 * pad, 2, 64, dtype=torch.bfloat16,
                       device=DEV) for _ in range(2)]
    views = [t[:, pad:pad + Lmax] for t in big]
    views[0].copy_(inp["kc"])
    views[1].copy_(inp["vc"])
    inp["kc"], inp["vc"] = views

    def step(q, k, v, cos, sin, pos, kc, vc):
        # check_rope_append hands over clones; write through the views
        out = decode_rope_append(q, k, v, cos, sin, pos, views[0], views[1])
        kc.copy_(views[0])
        vc.copy_(views[1])
        return out

    want = do.rope_append_expected(inp, rope_apply)
    got_q = step(inp["q"], inp["k"], inp["v"], inp["cos"], inp["sin"],
                 inp["pos"], views[0].clone(), views[1].clone())
    assert torch.equal(got_q, want[0])
    assert torch.equal(views[0], want[1]) and torch.equal(views[1], want[2])
    for t in big:   # nothing outside the view was written
        assert torch.count_nonzero(t[:, :pad]) == 0
        assert torch.count_nonzero(t[:, pad + Lmax:]) == 0


def test_bad_arguments():
    from modalities_amd.ops import decode_attention
    inp = do.decode_inputs([3, 4], 8, 4, 2, 64, DEV)
    q, kc, vc, lens = inp["q"], inp["kc"], inp["vc"], inp["lens"]
    with pytest.raises(TypeError):
        decode_attention(q, kc, vc, lens.long())
    with pytest.raises(ValueError):
        decode_attention(q, kc, vc, lens.cpu())
    with pytest.raises(ValueError):
        decode_attention(q, kc, vc, lens[:1])
    with pytest.raises(ValueError):
        decode_attention(q, kc, vc, lens.view(2, 1))
    bad = do.decode_inputs([3, 4], 8, 4, 2, 96, DEV)
    with pytest.raises(ValueError, match="head_dim"):
        decode_attention(bad["q"], bad["kc"], bad["vc"], bad["lens"])
    # the binding checks for itself
    with pytest.raises(RuntimeError, match="head_dim"):
        _dec(bad["q"], bad["kc"], bad["vc"], bad["lens"])
    with pytest.raises(RuntimeError, match="kv_lens"):
        _dec(q, kc, vc, lens.long())
    with pytest.raises(RuntimeError, match=f"smallest legal value is {_c0()}"):
        _dec(q, kc, vc, lens, _c0() // 2)
    assert decode_attention(q, kc, vc, lens).shape == q.shape
