"""`skinny_linear_mfma` (csrc/decode_gemv_mfma.hip) and the batch-9..32 route of
a prepared GPT2LLM on the GPU, against the fp64 oracle of decode_gemv_oracles.

Shapes are the smallest at which the kernel can go wrong, from its constants:

* a wave step is 4 k-groups x 16 bytes of a weight row: 64 e4m3 or 32 bf16
  elements of K  ->  K in {16, 32, 48, 64, 80};
* a workgroup round is MFMA_GEMV_KSPLIT = 8 wave steps: 512 e4m3 / 256 bf16
  ->  K in {240, 256, 272, 496, 512, 528};
* a trip of the K loop is MFMA_GEMV_LOADS = 8 steps of every wave, 4096 e4m3 /
  2048 bf16 elements; shorter K takes the predicated trip only  ->  K = 2560
  (bf16: one full trip and a tail) and K = 4112, 5120 (e4m3: the same);
* a workgroup owns 16 * RT weight rows, RT = 2 from SKINNY_MFMA_FILL_WGS = 192
  workgroups of 32 rows on; N in {15..17, 31..33} are the edges of one and
  two row tiles, N = 6112 / 6113 the last RT = 1 and the first RT = 2 size
  (the latter with a partial last workgroup);
* MTILES = 1 up to M = 16, 2 up to 32: M = 9 and 17 run with clamped spare
  batch columns.

The tiny model and its decode loop (_model, _prompt, _chunk, _decode_8,
_dequantized_copy) are imported from test_decode_gemv_gpu, so that the two
files decode the same model; the oracle modules stay as they are.
"""

import pytest
import torch

from tests import decode_gemv_oracles as go
from tests import kernel_oracles as ko
from tests.test_decode_gemv_gpu import (_chunk, _decode_8, _dequantized_copy,
                                        _model, _prompt)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMTS = ["fp8_e4m3", "bf16"]
MS = [1, 9, 16, 17, 32]
KS = [16, 32, 48, 64, 80, 240, 256, 272, 496, 512, 528, 1040, 2560, 4112]
NS = [1, 15, 16, 17, 31, 32, 33, 257, 6112, 6113]
ONE = 0x38     # e4m3 code of 1.0


def _sl():
    from modalities_amd.ops import skinny_linear_mfma
    return skinny_linear_mfma


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", KS)
def test_random_against_fp64_over_k(fmt, K):
    worst = {}
    for M in MS:
        args = go.make_case(M, 33, K, fmt, True, seed=K + M, device=DEV)
        worst[f"M{M}"] = go.check_skinny_linear(_sl(), *args)["y"]
    ko.require(f"skinny_linear_mfma {fmt} K{K}", worst)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N", NS)
def test_random_against_fp64_over_n(fmt, N):
    worst = {}
    for M in MS:
        args = go.make_case(M, N, 1040, fmt, False, seed=N + M, device=DEV)
        worst[f"M{M}"] = go.check_skinny_linear(_sl(), *args)["y"]
    ko.require(f"skinny_linear_mfma {fmt} N{N}", worst)


@pytest.mark.parametrize("fmt", FMTS)
def test_exact_selection_by_one_hot_rows(fmt):
    """32 one-hot x rows, a different k each: y[m, n] must be bf16(scale[n] *
    wq[n, k]) bit for bit.  The ks cover every byte of a 16-byte load (0..15),
    every k-group (16, 32, 48 e4m3; 8, 16, 24 bf16), every K-split wave (64 w
    e4m3, 32 w bf16), the second round (517; 320.. for bf16) and the last,
    partial wave step of K = 1040."""
    # N = 254 and a stride of 13 (coprime to 254) along n: every selected k
    # meets every valid code
    K, N = 1040, 254
    ks = list(range(16)) + [16, 32, 48] + list(range(64, 512, 64)) \
        + [96, 160, 224, 517, 1024, 1039]
    assert len(set(ks)) == 32
    codes = go.all_valid_codes()
    idx = (torch.arange(K)[None, :] * 7 + torch.arange(N)[:, None] * 13) \
        % codes.numel()
    wq = go.e4m3_codes(codes[idx]).contiguous()
    assert all(wq.view(torch.uint8)[:, k].unique().numel() == 254 for k in ks)
    scale = torch.exp2((torch.arange(N) % 9).float() - 4)
    want_all = wq.float() * scale[:, None]
    if fmt == "bf16":
        w, sc = want_all.to(torch.bfloat16).to(DEV), None
    else:
        w, sc = wq.to(DEV), scale.to(DEV)
    x = torch.zeros(32, K, dtype=torch.bfloat16)
    x[torch.arange(32), ks] = 1.0
    y = _sl()(x.to(DEV), w, sc, None).cpu()
    # + 0.0: the code 0x80 is -0.0, and a sum of it with the +0.0 products of
    # the other k is +0.0 in IEEE arithmetic
    want = (want_all[:, ks].t() + 0.0).to(torch.bfloat16)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("K", [16, 1040, 2560, 5120])
@pytest.mark.parametrize("M", [9, 32])
def test_exact_counting(M, K):
    """x = 1, every weight 1.0, power-of-two scales: y[n] == K * scale[n]
    exactly.  A dropped or doubled chunk changes the count."""
    N = 17
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
    x, w, sc, b = go.make_case(32, 65, 2560, fmt, True, seed=21, device=DEV)
    y32 = _sl()(x, w, sc, b)
    for r in (0, 15, 16, 31):
        assert torch.equal(_sl()(x[r:r + 1], w, sc, b)[0], y32[r]), (fmt, r)
    assert torch.equal(_sl()(x.flip(0).contiguous(), w, sc, b).flip(0), y32)
    for M in (9, 16, 17):
        ym = _sl()(x[32 - M:].contiguous(), w, sc, b)
        assert torch.equal(ym, y32[32 - M:]), (fmt, M)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("pad", [32, 6])
def test_strided_x_rows(fmt, pad):
    """pad = 32 keeps the rows 16-byte aligned and is read in place, pad = 6
    does not and is copied by the wrapper."""
    x, w, sc, b = go.make_case(17, 33, 1040, fmt, True, seed=31, x_pad=pad,
                               device=DEV)
    assert not x.is_contiguous()
    ko.require(f"skinny_linear_mfma strided {fmt} pad{pad}",
               go.check_skinny_linear(_sl(), x, w, sc, b))
    assert torch.equal(_sl()(x, w, sc, b), _sl()(x.contiguous(), w, sc, b))


def test_argument_errors():
    from modalities_amd.ops.backend import hip_ext
    sl, ext = _sl(), hip_ext()
    x, w, sc, b = go.make_case(33, 8, 32, "fp8_e4m3", True, seed=5, device=DEV)
    assert ext.skinny_linear_mfma_max_m() == 32
    with pytest.raises(ValueError, match="M must be"):
        sl(x, w, sc, b)
    with pytest.raises(RuntimeError, match="M must be"):
        ext.skinny_linear_mfma(x, w, sc, b)
    w24 = w.view(torch.uint8)[:, :24].contiguous().view(go.E4M3)
    with pytest.raises(ValueError, match="multiple of 16"):
        sl(x[:9, :24], w24, sc, b)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.skinny_linear_mfma(x[:9, :24].contiguous(), w24, sc, b)
    with pytest.raises(ValueError, match="is on"):
        sl(x[:9], w.cpu(), sc, b)
    with pytest.raises(RuntimeError, match="w must be"):
        ext.skinny_linear_mfma(x[:9], w.cpu(), sc, b)
    with pytest.raises(ValueError, match="contiguous"):
        sl(x[:9], w.t().contiguous().t(), sc, b)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.skinny_linear_mfma(x[:9], w.t().contiguous().t(), sc, b)


def _spies(monkeypatch):
    from modalities_amd.ops import decode_linear as dl
    calls = {"skinny_linear": 0, "skinny_linear_mfma": 0}
    for name in calls:
        def spy(*a, _real=getattr(dl, name), _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(dl, name, spy)
    return calls


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B", [12, 20])
def test_prepared_model_matches_dequantized_copy(fmt, B, monkeypatch):
    """8 decode steps across a decode-chunk edge at a batch of one and of two
    batch tiles; at batch 12 the replayed graph equals the eager step."""
    model = _model()
    model.prepare_decode_weights(fmt)
    ref = _dequantized_copy(model)
    prompt = _prompt(B, _chunk() - 3)
    want, fed = _decode_8(ref, prompt, prefill=model)
    calls = _spies(monkeypatch)
    got, _ = _decode_8(model, prompt, feed=fed)
    assert calls == {"skinny_linear": 0, "skinny_linear_mfma":
                     8 * len(model._decode_linears())}
    torch.testing.assert_close(got.float(), want.float(), rtol=2e-2,
                               atol=2e-2)
    if B == 12:
        replay, _ = _decode_8(model, prompt, graph=True, feed=fed)
        assert torch.equal(got, replay)


def test_batch_four_keeps_the_valu_kernel(monkeypatch):
    model = _model()
    model.prepare_decode_weights("fp8_e4m3")
    calls = _spies(monkeypatch)
    _decode_8(model, _prompt(4, _chunk() - 3))
    assert calls == {"skinny_linear": 8 * len(model._decode_linears()),
                     "skinny_linear_mfma": 0}
