"""ops.decode_attention with T > 1 query tokens per row on the CPU route,
its argument errors, and the set_decode_chunk_tokens switch."""

import pytest
import torch

from modalities_amd import ops
from tests import decode_oracles as do
from tests import kernel_oracles as ko


def _inputs(lens, Lmax, T, Hq, Hkv, D, seed=0):
    inp = do.decode_inputs(lens, Lmax, Hq, Hkv, D, "cpu", seed=seed)
    g = ko._gen(seed + 1)
    inp["q"] = ko.bf(torch.randn(len(lens), T, Hq, D, generator=g))
    return inp


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
@pytest.mark.parametrize("T,Hq,Hkv,D", [(2, 2, 2, 64), (5, 4, 2, 80)])
def test_cpu_route_against_fp64(T, Hq, Hkv, D, fmt):
    lens = [T - 1, T, 40, 0]            # the first row has a query without keys
    inp = _inputs(lens, 48, T, Hq, Hkv, D, seed=T)
    kc, vc, scales = inp["kc"], inp["vc"], {}
    if fmt == "fp8":
        (kq, ks), (vq, vs) = ops.quantize_kv_fp8(kc), ops.quantize_kv_fp8(vc)
        kc, vc = ops.dequantize_kv_fp8(kq, ks), ops.dequantize_kv_fp8(vq, vs)
        o = ops.decode_attention(inp["q"], kq, vq, inp["lens"], k_scale=ks,
                                 v_scale=vs)
    else:
        o = ops.decode_attention(inp["q"], kc, vc, inp["lens"])
    assert tuple(o.shape) == (4, T, Hq, D) and o.dtype == torch.bfloat16
    for b, n in enumerate(lens):
        t0 = max(T - n, 0)
        assert not o[b, :t0].any()
        if n == 0:
            continue
        r = ko.attn_ref64(inp["q"][b:b + 1, t0:], kc[b:b + 1, :n],
                          vc[b:b + 1, :n], off=n - (T - t0))
        ko.require(f"cpu/{fmt}/T{T}/len{n}", {"o": ko.ratio(
            (o[b:b + 1, t0:].double() - r["o"]).abs(),
            3 * ko.BF16_ULP * r["absPV"] + ko.F32_TINY)})


def test_argument_errors():
    inp = _inputs([8, 8], 16, 3, 4, 2, 64)
    q, kc, vc, lens = inp["q"], inp["kc"], inp["vc"], inp["lens"]
    with pytest.raises(ValueError, match=r"\[B, T, Hq, D\] with T >= 1"):
        ops.decode_attention(q[:, :0], kc, vc, lens)
    with pytest.raises(ValueError, match="do not match q"):
        ops.decode_attention(q, kc[:1], vc[:1], lens)
    codes = kc.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="needs k_scale and v_scale"):
        ops.decode_attention(q, codes, codes, lens)


def test_switch_rejects_negatives():
    was = ops.decode_chunk_tokens()
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="set_decode_chunk_tokens"):
            ops.set_decode_chunk_tokens(bad)
    # decode_attention with T > 1 is what the switch routes to
    inp = _inputs([6], 8, 2, 2, 1, 64)
    assert ops.decode_attention(inp["q"], inp["kc"], inp["vc"],
                                inp["lens"]).shape[1] == 2
    assert ops.decode_chunk_tokens() == was
