"""The fused options of `skinny_linear` (csrc/decode_gemv_fused.hip) and the
fused decode step of GPT2LLM on the GPU. K values are the pass, trip and tail
edges listed in test_decode_gemv_gpu.py; N_out = 17 is a partial workgroup at
both row tilings (34 weight rows under glu)."""

import pytest
import torch

from tests import decode_gemv_oracles as go
from tests import kernel_oracles as ko
from tests import test_decode_gemv_gpu as base

pytestmark = pytest.mark.gpu

DEV, _sl, FMTS = base.DEV, base._sl, base.FMTS
OPTIONS = {"norm": (True, False, False), "residual": (False, True, False),
           "norm_glu": (True, False, True), "all": (True, True, True)}


def fused_reference(x, w, scale, bias, g, eps, res, glu):
    """(ref, S) in fp64: ref = inv * scale * sum (x g) w + bias, S the same
    over absolute values; glu: h = silu(a) u, S_h = 1.1 |u| S_a + |silu(a)|
    S_u (|silu'| <= 1.1); a residual adds to ref and |residual| to S."""
    x, w, scale, bias, g, res = (None if t is None else t.cpu()
                                 for t in (x, w, scale, bias, g, res))
    xd, wd = x.double(), w.float().double()
    inv = 1.0
    if g is not None:
        inv = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
        xd = xd * g.double()
    sc = 1.0 if scale is None else scale.double()
    ref = inv * sc * (xd @ wd.t())
    S = inv * sc * (xd.abs() @ wd.abs().t())
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    if glu:
        H = ref.shape[1] // 2
        a, u = ref[:, :H], ref[:, H:]
        silu = a * torch.sigmoid(a)
        ref, S = silu * u, 1.1 * u.abs() * S[:, :H] + silu.abs() * S[:, H:]
    if res is not None:
        ref, S = ref + res.double(), S + res.double().abs()
    return ref, S


def fused_case(M, n_out, K, fmt, opts, seed, device, x_pad=0):
    """make_case plus g and residual; rows scaled by 2^-4..2^4."""
    norm, res, glu = opts
    x, w, sc, b = go.make_case(M, n_out * (1 + glu), K, fmt, True, seed,
                               x_pad=x_pad, device=device)
    gen = torch.Generator().manual_seed(seed + 1000)
    x.mul_(torch.exp2(torch.linspace(-4, 4, M))[:, None].to(x))
    g = (1 + 0.5 * torch.randn(K, generator=gen)).to(torch.bfloat16) \
        .to(device) if norm else None
    r = torch.randn(M, n_out, generator=gen).to(torch.bfloat16).to(device) \
        if res else None
    return x, w, sc, b, g, r, glu


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("K", [16, 528, 1040, 2064, 2560, 4112])
def test_fused_against_fp64(fmt, opt, K):
    worst = {}
    for M in base.MS:
        x, w, sc, b, g, r, glu = fused_case(M, 17, K, fmt, OPTIONS[opt],
                                            K + M, DEV)
        x[M - 1] *= 1e-3     # a row on which eps = 1e-2 matters
        for eps in (1e-6, 1e-2):
            y = _sl()(x, w, sc, b, norm_weight=g, norm_eps=eps, residual=r,
                      glu=glu)
            ref, S = fused_reference(x, w, sc, b, g, eps, r, glu)
            assert y.dtype == torch.bfloat16 and y.shape == ref.shape
            worst[f"M{M}eps{eps:g}"] = ko.single_rounding_ratio(y.cpu(), ref,
                                                                S)
    ko.require(f"skinny_linear fused {opt} {fmt} K{K}", worst)


def test_zero_row_gives_bias_plus_residual():
    x, w, sc, b, g, r, _ = fused_case(3, 17, 1040, "fp8_e4m3",
                                      (True, True, False), 7, DEV)
    x[1] = 0
    y = _sl()(x, w, sc, b, norm_weight=g, residual=r)
    want = (b.float() + r[1].float()).to(torch.bfloat16)
    assert torch.equal(y[1].view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("fmt", FMTS)
def test_fused_row_is_bit_identical_for_every_m_and_place(fmt):
    x, w, sc, b, g, r, _ = fused_case(8, 65, 2560, fmt, (True, True, True),
                                      21, DEV)
    kw = dict(norm_weight=g, glu=True)
    y8 = _sl()(x, w, sc, b, residual=r, **kw)
    yr = _sl()(x.flip(0).contiguous(), w, sc, b,
               residual=r.flip(0).contiguous(), **kw)
    assert torch.equal(yr.flip(0), y8)
    for M in (1, 2, 3, 5):
        ym = _sl()(x[8 - M:].contiguous(), w, sc, b, residual=r[8 - M:], **kw)
        assert torch.equal(ym, y8[8 - M:]), (fmt, M)


def test_residual_is_added_before_the_single_rounding():
    x, w, sc, b, _, r, _ = fused_case(3, 17, 528, "fp8_e4m3",
                                      (False, True, False), 41, DEV)
    fused = _sl()(x, w, sc, b, residual=r)
    late = (_sl()(x, w, sc, b).float() + r.float()).to(torch.bfloat16)
    ref, _ = fused_reference(x, w, sc, b, None, 0.0, r, False)
    assert not torch.equal(fused, late), "the case cannot tell the two apart"
    assert (fused.cpu().double() - ref).abs().sum() \
        < (late.cpu().double() - ref).abs().sum()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("pad", [32, 6])
def test_strided_x_and_residual(fmt, pad):
    x, w, sc, b, g, r, glu = fused_case(5, 33, 1040, fmt, (True, True, True),
                                        31, DEV, x_pad=pad)
    rv = torch.randn(5, 33 + pad, device=DEV).to(torch.bfloat16)[:, 3:36]
    rv.copy_(r)
    assert not x.is_contiguous() and not rv.is_contiguous()
    kw = dict(norm_weight=g, glu=glu)
    y = _sl()(x, w, sc, b, residual=rv, **kw)
    ref, S = fused_reference(x, w, sc, b, g, 1e-6, rv, glu)
    ko.require(f"fused strided {fmt} pad{pad}",
               {"y": ko.single_rounding_ratio(y.cpu(), ref, S)})
    assert torch.equal(y, _sl()(x.contiguous(), w, sc, b, residual=r, **kw))


@pytest.fixture
def fused_step():
    from modalities_amd import ops
    ops.set_decode_fused_step(True)
    yield ops
    ops.set_decode_fused_step(False)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("variant", [
    dict(), dict(fused_qkv=False, activation_type="gelu", bias=True)])
def test_fused_model_matches_dequantized_copy(fmt, variant, monkeypatch,
                                              fused_step):
    from modalities_amd.ops import decode_linear as dl
    model = base._model(**variant)
    model.prepare_decode_weights(fmt)
    ref = base._dequantized_copy(model)
    prompt = base._prompt(2, base._chunk() - 3)
    want, fed = base._decode_8(ref, prompt, prefill=model)
    calls = []
    real = dl.skinny_linear
    monkeypatch.setattr(dl, "skinny_linear", lambda *a, **k: calls.append(
        any(k.get(o) is not None and k.get(o) is not False
            for o in ("norm_weight", "residual", "glu"))) or real(*a, **k))
    got, _ = base._decode_8(model, prompt, feed=fed)
    assert len(calls) == 8 * len(model._decode_linears())
    assert all(calls), "a linear of the step ran unfused"
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-2,
                               atol=2e-2)


@pytest.mark.parametrize("fmt", FMTS)
def test_graph_replay_equals_eager_fused_step(fmt, fused_step):
    model = base._model()
    model.prepare_decode_weights(fmt)
    prompt = base._prompt(2, base._chunk() - 3)
    eager, fed = base._decode_8(model, prompt)
    replay, _ = base._decode_8(model, prompt, graph=True, feed=fed)
    assert torch.equal(eager, replay)


@pytest.mark.parametrize("norm", ["rms_norm", "layer_norm"])
def test_switch_reset_and_layer_norm_fallback(norm, fused_step):
    # on then off equals never switched; layer_norm ignores the switch
    cfg = {k: dict(variant=norm) for k in (
        "attention_norm_config", "ffn_norm_config", "lm_head_norm_config")}
    model, fresh = base._model(**cfg), base._model(**cfg)
    for m in (model, fresh):
        m.prepare_decode_weights("fp8_e4m3")
    prompt = base._prompt(2, base._chunk() - 3)
    on, fed = base._decode_8(model, prompt)
    fused_step.set_decode_fused_step(False)
    a, _ = base._decode_8(model, prompt, feed=fed)
    b, _ = base._decode_8(fresh, prompt, feed=fed)
    assert torch.equal(a, b)
    assert torch.equal(on, a) == (norm == "layer_norm")
