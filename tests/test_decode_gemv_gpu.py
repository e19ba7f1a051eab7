"""`skinny_linear` (csrc/decode_gemv.hip) and the prepared-decode-weight route
of GPT2LLM on the GPU.

Shapes are the smallest at which the kernel can go wrong.  Edges of its own
tiling, from the constants of decode_gemv.hip:

* GEMV_PASS_BYTES = 64 lanes x 16 bytes: one pass of a wave covers 1024 e4m3
  or 512 bf16 elements of K  ->  K in {496, 512, 528} next to the issue's
  {1008, 1024, 1040};
* the main loop takes U passes per trip, gemv_unroll(MT) = 4 (M <= 2) or 2
  (M >= 3): 4096 / 2048 e4m3 and 2048 / 1024 bf16 elements  ->  K in
  {2032, 2048, 2064, 4080, 4096, 4112};
* rows per workgroup = 4 waves x gemv_rows(MT) = 8 (M <= 2) or 16 (M >= 3),
  rows per wave 2 or 4  ->  N in {7, 8, 9, 15, 16, 17} next to the issue's;
* MT in {1, 2, 4, 8}: M = 3 and 5 run with clamped spare batch rows.
"""

import pytest
import torch

from tests import decode_gemv_oracles as go
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["fp8_e4m3", "bf16"]
MS = [1, 2, 3, 5, 8]
KS = [16, 48, 496, 512, 528, 1008, 1024, 1040, 2032, 2048, 2064, 2560, 4080,
      4096, 4112]
NS = [1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257]
ONE = 0x38     # e4m3 code of 1.0


def _sl():
    from modalities_amd.ops import skinny_linear
    return skinny_linear


# ------------------------------------------------------------- fp64 oracle
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", KS)
def test_random_against_fp64_over_k(fmt, K):
    """Every K edge at every M, N = 17 (a partial workgroup at both row
    tilings), with bias."""
    worst = {}
    for M in MS:
        args = go.make_case(M, 17, K, fmt, True, seed=K + M, device=DEV)
        r = go.check_skinny_linear(_sl(), *args)
        worst[f"M{M}"] = r["y"]
    ko.require(f"skinny_linear {fmt} K{K}", worst)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N", NS)
def test_random_against_fp64_over_n(fmt, N):
    """Every N edge at every M, K = 1040 (one full pass and a tail of one
    chunk for e4m3; two passes and a tail for bf16), no bias."""
    worst = {}
    for M in MS:
        args = go.make_case(M, N, 1040, fmt, False, seed=N + M, device=DEV)
        r = go.check_skinny_linear(_sl(), *args)
        worst[f"M{M}"] = r["y"]
    ko.require(f"skinny_linear {fmt} N{N}", worst)


# ------------------------------------------------------- exact / structural
def _all_code_weight(N, K):
    """[N, K] e4m3 codes that differ along k and n (no NaN code)."""
    codes = go.all_valid_codes()
    idx = (torch.arange(K)[None, :] * 7 + torch.arange(N)[:, None] * 13) \
        % codes.numel()
    return go.e4m3_codes(codes[idx]).contiguous()


@pytest.mark.parametrize("fmt", FMTS)
def test_exact_selection_by_one_hot_rows(fmt):
    """x rows are one-hots, a different k per batch row: y[m, n] must be
    bf16(scale[n] * wq[n, k]) bit for bit.  The ks cover every byte position
    of a 16-byte load (k = 0..15), lanes of the first pass, the second pass
    and the last chunk of K = 1040."""
    K, N = 1040, 9
    ks = list(range(16)) + [16, 31, 511, 512, 1023] + list(range(1024, 1040))
    wq = _all_code_weight(N, K)
    scale = torch.exp2(torch.arange(N).float() - 4)
    if fmt == "bf16":
        w, sc = (wq.float() * scale[:, None]).to(torch.bfloat16), None
        want_all = w.float()
    else:
        w, sc = wq, scale
        want_all = wq.float() * scale[:, None]
    w = w.to(DEV)
    sc = None if sc is None else sc.to(DEV)
    for i in range(0, len(ks), 8):
        sel = ks[i:i + 8]
        x = torch.zeros(len(sel), K, dtype=torch.bfloat16)
        for m, k in enumerate(sel):
            x[m, k] = 1.0
        y = _sl()(x.to(DEV), w, sc, None).cpu()
        # + 0.0: the code 0x80 is -0.0, and a sum of it with the +0.0
        # products of the other k is +0.0 in IEEE arithmetic
        want = (want_all[:, sel].t() + 0.0).to(torch.bfloat16)
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), \
            (fmt, sel)


@pytest.mark.parametrize("K", [16, 1040, 2560, 5120])
@pytest.mark.parametrize("M", [1, 8])
def test_exact_counting(M, K):
    """x = 1, every weight 1.0, power-of-two scales: y[n] == K * scale[n]
    exactly (each K here has at most 8 significant bits, so it is a bf16
    value; 5120 is one main-loop trip of four passes plus one tail pass for
    e4m3 at M <= 2).  A dropped or doubled chunk changes the count."""
    N = 17
    assert float(torch.tensor(float(K)).to(torch.bfloat16)) == K
    scale = torch.exp2(torch.arange(N).float() - 8)
    x = torch.ones(M, K, dtype=torch.bfloat16, device=DEV)
    wq = go.e4m3_codes(torch.full((N, K), ONE, dtype=torch.uint8)).to(DEV)
    y = _sl()(x, wq, scale.to(DEV), None).cpu().float()
    assert torch.equal(y, (K * scale)[None, :].expand(M, N))
    wb = torch.ones(N, K, dtype=torch.bfloat16, device=DEV)
    yb = _sl()(x, wb, None, None).cpu().float()
    assert torch.equal(yb, torch.full((M, N), float(K)))


@pytest.mark.parametrize("fmt", FMTS)
def test_row_is_bit_identical_for_every_m_and_place(fmt):
    x, w, sc, b = go.make_case(8, 65, 2560, fmt, True, seed=21, device=DEV)
    y8 = _sl()(x, w, sc, b)
    for r in (0, 3, 7):
        y1 = _sl()(x[r:r + 1], w, sc, b)
        assert torch.equal(y1[0], y8[r]), (fmt, r, "M = 1")
    # the same rows elsewhere: reversed batch, and batches of 2, 3, 5
    yr = _sl()(x.flip(0).contiguous(), w, sc, b)
    assert torch.equal(yr.flip(0), y8)
    for M in (2, 3, 5):
        ym = _sl()(x[8 - M:].contiguous(), w, sc, b)
        assert torch.equal(ym, y8[8 - M:]), (fmt, M)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("pad", [32, 6])
def test_strided_x_rows(fmt, pad):
    """x as a view into a wider buffer (what the fused-QKV split gives):
    pad = 32 keeps the rows 16-byte aligned and is read in place, pad = 6
    does not and is copied by the wrapper."""
    x, w, sc, b = go.make_case(5, 33, 1040, fmt, True, seed=31, x_pad=pad,
                               device=DEV)
    assert not x.is_contiguous()
    ko.require(f"skinny_linear strided {fmt} pad{pad}",
               go.check_skinny_linear(_sl(), x, w, sc, b))
    assert torch.equal(_sl()(x, w, sc, b), _sl()(x.contiguous(), w, sc, b))


def test_bias_is_added_before_the_single_rounding():
    x, w, sc, b = go.make_case(3, 17, 528, "fp8_e4m3", True, seed=41,
                               device=DEV)
    with_b = _sl()(x, w, sc, b)
    without = _sl()(x, w, sc, None)
    ref, _ = go.skinny_reference(x.cpu(), w.cpu(), sc.cpu(), b.cpu())
    ko.require("bias", go.check_skinny_linear(_sl(), x, w, sc, b))
    late = (without.float() + b.float()).to(torch.bfloat16)
    assert not torch.equal(with_b, late), "the case cannot tell the two apart"
    assert (with_b.cpu().double() - ref).abs().sum() \
        < (late.cpu().double() - ref).abs().sum()


def test_argument_errors():
    sl = _sl()
    x, w, sc, b = go.make_case(2, 8, 32, "fp8_e4m3", True, seed=5, device=DEV)
    with pytest.raises(ValueError, match="M must be"):
        sl(x.repeat(5, 1)[:9], w, sc, b)
    w24 = w.view(torch.uint8)[:, :24].contiguous().view(go.E4M3)
    with pytest.raises(ValueError, match="multiple of 16"):
        sl(x[:, :24], w24, sc, b)
    with pytest.raises(TypeError):
        sl(x.float(), w, sc, b)
    with pytest.raises(TypeError):
        sl(x, w.float(), sc, b)
    with pytest.raises(TypeError):
        sl(x, w, sc.double(), b)
    with pytest.raises(TypeError):
        sl(x, w, sc, b.float())
    with pytest.raises(ValueError, match="is on"):
        sl(x, w.cpu(), sc, b)
    with pytest.raises(ValueError, match="is on"):
        sl(x, w, sc.cpu(), b)
    with pytest.raises(ValueError, match="is on"):
        sl(x, w, sc, b.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        sl(x, w.t().contiguous().t(), sc, b)
    # the extension itself refuses what would read out of bounds
    from modalities_amd.ops.backend import hip_ext
    ext = hip_ext()
    assert ext.skinny_linear_max_m() == 8
    with pytest.raises(RuntimeError, match="M must be"):
        ext.skinny_linear(x.repeat(5, 1)[:9].contiguous(), w, sc, b)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.skinny_linear(x[:, :24].contiguous(), w24, sc, b)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.skinny_linear(x, w.t().contiguous().t(), sc, b)
    with pytest.raises(RuntimeError, match="scale"):
        ext.skinny_linear(x, w, sc[:-1].contiguous(), b)
    with pytest.raises(RuntimeError, match="scale"):
        ext.skinny_linear(x, w, None, b)


# -------------------------------------------------------------------- model
def _chunk():
    from modalities_amd.ops.backend import hip_ext
    return hip_ext().decode_attn_kv_chunk()


def _model(**kw):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    torch.manual_seed(3)
    cfg = dict(vocab_size=128, n_layer=2, n_embd=512, ffn_hidden=1024,
               n_head_q=4, n_head_kv=2, fused_qkv=True,
               sequence_length=_chunk() + 32, seed=7, dropout=0.0)
    cfg.update(kw)
    return GPT2LLM(GPT2LLMConfig(**cfg)).to(DEV).to(torch.bfloat16).eval()


def _prompt(B, T):
    g = torch.Generator().manual_seed(9)
    return torch.randint(0, 128, (B, T), generator=g).to(DEV)


def _dequantized_copy(model):
    import copy
    from modalities_amd.ops.decode_linear import get_prepared
    ref = copy.deepcopy(model)
    ref.clear_decode_weights()
    with torch.no_grad():
        for a, b in zip(model._decode_linears(), ref._decode_linears()):
            p = get_prepared(a)
            if p is not None and p.scale is not None:
                b.weight.copy_((p.w.float() * p.scale[:, None]))
    return ref


def _decode_8(model, prompt, graph=False, feed=None, prefill=None):
    """8 single-token steps after the prefill, across a decode-chunk edge.
    feed: the tokens to feed (so two models decode the same text).
    prefill: the model that fills the cache (default: `model`)."""
    from modalities_amd.inference.text_generation import DecodeGraph
    B = prompt.shape[0]
    logits, fed = [], []
    with torch.no_grad():
        cache = model.new_kv_cache(B, max_len=_chunk() + 16)
        out = (prefill or model).forward_cached({"input_ids": prompt},
                                                cache)["logits"]
        g = DecodeGraph(model, cache, "input_ids", "logits") if graph else None
        for i in range(8):
            nxt = out[:, -1, :].argmax(-1, keepdim=True) if feed is None \
                else feed[i]
            fed.append(nxt)
            if g is not None:
                out = g.step(nxt)
            else:
                out = model.forward_cached({"input_ids": nxt}, cache)["logits"]
            logits.append(out.clone())
    return torch.cat(logits, 1), fed


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("variant", [
    dict(),
    dict(fused_qkv=False, activation_type="gelu", bias=True),
])
def test_prepared_model_matches_dequantized_copy(fmt, variant, monkeypatch):
    from modalities_amd.ops import decode_linear as dl
    model = _model(**variant)
    model.prepare_decode_weights(fmt)
    ref = _dequantized_copy(model)
    prompt = _prompt(2, _chunk() - 3)
    # the prefill stays on the resident bf16 weights: `model` fills both
    # caches, only the single-token steps differ
    want, fed = _decode_8(ref, prompt, prefill=model)
    calls = []
    real = dl.skinny_linear
    monkeypatch.setattr(dl, "skinny_linear",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    got, _ = _decode_8(model, prompt, feed=fed)
    assert len(calls) == 8 * len(model._decode_linears())
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-2,
                               atol=2e-2)


@pytest.mark.parametrize("fmt", FMTS)
def test_graph_replay_equals_eager_prepared_step(fmt):
    model = _model()
    model.prepare_decode_weights(fmt)
    prompt = _prompt(2, _chunk() - 3)
    eager, fed = _decode_8(model, prompt)
    replay, _ = _decode_8(model, prompt, graph=True, feed=fed)
    assert torch.equal(eager, replay)


def test_option_unset_is_bit_identical_to_a_never_prepared_model():
    model, fresh = _model(), _model()
    prompt = _prompt(2, _chunk() - 3)
    model.prepare_decode_weights("fp8_e4m3")
    _decode_8(model, prompt)
    model.clear_decode_weights()
    a, fed = _decode_8(model, prompt)
    b, _ = _decode_8(fresh, prompt, feed=fed)
    assert torch.equal(a, b)


def test_generate_tokens_with_fp8_weights_under_graph_replay(monkeypatch):
    """The public route: decode_weight_format on the inference component
    prepares the model before the prefill, the captured step launches the
    skinny GEMM, and the replayed text equals the eagerly decoded one."""
    from modalities_amd.inference import text_generation as tg
    from modalities_amd.ops import decode_linear as dl
    from modalities_amd.tokenization.tokenizer_wrapper import CharTokenizer
    model = _model(vocab_size=260)
    made, calls = [], []
    real_graph, real_sl = tg.DecodeGraph, dl.skinny_linear

    class Spy(real_graph):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.steps = 0
            made.append(self)

        def step(self, next_ids):
            self.steps += 1
            return super().step(next_ids)
    monkeypatch.setattr(tg, "DecodeGraph", Spy)
    monkeypatch.setattr(dl, "skinny_linear",
                        lambda *a, **k: calls.append(1) or real_sl(*a, **k))
    kw = dict(prompt_template="{text}", sequence_length=24, temperature=0.0,
              device=torch.device(DEV), decode_weight_format="fp8_e4m3")
    with_graph = tg.TextInferenceComponent(model, CharTokenizer(), **kw)
    assert model.decode_weight_format is None
    a = with_graph.generate_tokens("hello world")
    assert model.decode_weight_format == "fp8_e4m3"
    assert len(made) == 1 and made[0].steps >= 1, "no token from a replay"
    # the warm-up step and the captured step each launch every linear
    assert len(calls) == 2 * len(model._decode_linears())
    without = tg.TextInferenceComponent(model, CharTokenizer(),
                                        use_decode_graph=False, **kw)
    assert a == without.generate_tokens("hello world")
