"""GPU tests: document-masked causal attention (the DOC instantiations of
the v2 kernels) against the fp64 oracles of tests/docmask_oracles.py, with
document layouts placed at the kernels' tile edges (wave 32 q rows, kv
sub-tile 64, kv stage 128, workgroup 256, dKdV q stage 64 / 32 at fused
D = 80).  tests/test_docmask_oracles_cpu.py proves on the CPU that these
checkers reject the subtly wrong masks.

Worst measured error / bound on an MI355X (every check asserts <= 1; the
bounds are those of tests/kernel_oracles.py, none is fitted to a kernel):

  case family                          worst error / bound
  -----------------------------------  ----------------------------------------
  fwd, random, all layouts x D         o 0.57   lse 0.014
  bwd, random, all layouts x D         dq 0.74  dk 0.63  dv 0.48
  bwd with dlse                        dq 0.48  dk 0.60  dv 0.48
  counting V                           count 0.094 (of 0.5 key)  lse-log n 0.010
  flash_attention wrapper              o 0.50; gradients bit-identical to the
                                       direct entry point
  V view in a joint buffer (fwd)       o 0.48   lse 0.012
  attn_bwd_qkvjoint_doc                dq 0.56  dk 0.63  dv 0.48, sentinel intact
  fused_qkv_rope_attention (64/80)     o 0.52   dq 0.34  dk 0.25  dv 0.48
  leakage (o, lse, dq, dk, dv)         bit-identical; T300 one-key rows o == v

  backward kernel / emulation error ratio: dv 1.0 everywhere; dq up to 1.6,
  dk up to 1.4 (the bound allows 2).
"""

import functools

import pytest
import torch

from tests import docmask_oracles as dm
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"
BF16 = torch.bfloat16
DS = [64, 80, 128]


def _tri(T):
    """Document lengths 1, 2, 3, ... to the end."""
    out, s, n = [], 0, 1
    while s < T:
        out.append(s)
        s += n
        n += 1
    return out


# name -> (T, one list of document starts per batch row, Hq, Hkv)
LAYOUTS = {
    "T1": (1, [[0]], 2, 1),
    "T257_one_doc": (257, [[0]], 2, 1),
    "T300_every_pos": (300, [list(range(300))], 2, 1),
    "T777_0_700": (777, [[0, 700]], 2, 1),
    # boundary inside a wave; kv tiles 0-1 fully masked for the later rows
    # before their first visible key
    "T520_0_300": (520, [[0, 300]], 2, 1),
    "T300_len_1_2_3": (300, [_tri(300)], 2, 1),
    # last document ends at a T that is no multiple of 32
    "T333_0_200": (333, [[0, 200]], 2, 1),
    # fwd loop starts late, dKdV q range ends early; GQA cursor wrap; a
    # different layout in batch row 1
    "T1024_gqa_4_2": (1024, [[0, 512, 768], [0, 100, 900]], 4, 2),
    "T1024_gqa_8_1": (1024, [[0, 512, 768], [0, 100, 900]], 8, 1),
}
for _s in (63, 64, 65, 127, 128, 129, 255, 256, 257):
    LAYOUTS[f"T520_0_{_s}"] = (520, [[0, _s]], 2, 1)
NAMES = list(LAYOUTS)
DLSE_CASES = ("T520_0_300", "T1024_gqa_4_2")


def _start(name):
    T, lay, _, _ = LAYOUTS[name]
    return dm.layouts_to_start(lay, T, DEV)


@functools.lru_cache(maxsize=None)
def _case(name, D, dlse=False):
    """Inputs + fp64 reference + emulation, computed once per (layout, D)."""
    T, lay, Hq, Hkv = LAYOUTS[name]
    B = len(lay)
    inp = ko.attn_random_inputs(B, T, T, Hq, Hkv, D, DEV, seed=T * 3 + D)
    g = None
    if dlse:
        g = torch.randn(B, Hq, T, generator=ko._gen(T)).to(DEV)
    return dm.DocCase(inp, _start(name), dlse=g)


def _fwd(q, k, v, start):
    return tuple(EXT.attn_fwd_doc_v2(q, k, v, True, 0, start))


def _bwd(do, q, k, v, o, lse, start, end, dlse=None):
    return tuple(EXT.attn_bwd_doc_v2(do, q, k, v, o, lse, True, 0, start, end,
                                     dlse))


# --------------------------------------------------------- fp64 oracle checks
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("D", DS)
def test_doc_random_vs_fp64(D, name):
    case = _case(name, D)
    r, o, lse = dm.check_doc_fwd(_fwd, case)
    ko.require(f"doc/D{D}/{name}/fwd", r)
    ko.require(f"doc/D{D}/{name}/bwd", dm.check_doc_bwd(_bwd, case))
    if name == "T300_every_pos":
        # one visible key per row: P = 1 exactly, o is v bit for bit
        rep = case.q.shape[2] // case.v.shape[2]
        assert torch.equal(o, case.v.repeat_interleave(rep, dim=2))


@pytest.mark.parametrize("name", DLSE_CASES)
@pytest.mark.parametrize("D", DS)
def test_doc_backward_with_dlse(D, name):
    case = _case(name, D, dlse=True)
    ko.require(f"doc_dlse/D{D}/{name}", dm.check_doc_bwd(_bwd, case))


@pytest.mark.parametrize("name", ["T520_0_300", "T520_0_65", "T520_0_257",
                                  "T1024_gqa_4_2", "T1024_gqa_8_1"])
@pytest.mark.parametrize("D", DS)
def test_doc_counting(D, name):
    """Uniform attention over a one-hot V counts the visible keys of every
    row: a skipped or extra tile, a late loop start one tile off or a mask
    off by one moves a count by 1."""
    _, _, Hq, Hkv = LAYOUTS[name]
    ko.require(f"doc_count/D{D}/{name}",
               dm.check_doc_counting(_fwd, D, _start(name), DEV, Hq, Hkv))


@pytest.mark.parametrize("name", ["T1", "T520_0_300", "T1024_gqa_4_2"])
@pytest.mark.parametrize("D", DS)
def test_doc_through_flash_attention(D, name):
    """The public wrapper: o within the fp64 bound; its autograd gradients
    are those of the direct entry point on the kernel's own (o, lse),
    doc_end derived by the wrapper."""
    from modalities_amd.ops.attention import flash_attention
    case = _case(name, D)
    q, k, v = (t.clone().requires_grad_(True)
               for t in (case.q, case.k, case.v))
    o = flash_attention(q, k, v, causal=True, doc_start=case.start)
    r, _, _ = dm.check_doc_fwd(lambda *_: (o.detach(), case.ref["lse"]), case)
    ko.require(f"doc_wrapper/D{D}/{name}", {"o": r["o"]})
    o.backward(case.do)
    o2, lse2 = _fwd(case.q, case.k, case.v, case.start)
    assert torch.equal(o.detach(), o2)
    want = _bwd(case.do, case.q, case.k, case.v, o2, lse2, case.start,
                case.end)
    for got, w, n in zip((q.grad, k.grad, v.grad), want, ("dq", "dk", "dv")):
        assert torch.equal(got, w), n


# -------------------------------------------------------------------- leakage
@pytest.mark.parametrize("name", ["T520_0_300", "T520_0_129", "T333_0_200",
                                  "T1024_gqa_4_2"])
@pytest.mark.parametrize("D", DS)
def test_doc_no_leak_bitwise(D, name):
    """Replacing q/k/v rows of the first document by other finite values
    leaves o, lse, dq, dk, dv of every later document's rows bit-identical:
    a masked score contributes an exact 0, never a small number."""
    case = _case(name, D)
    T, lay, Hq, Hkv = LAYOUTS[name]
    # rows of batch row b at or after its second document start
    later = torch.zeros(len(lay), T, dtype=torch.bool, device=DEV)
    for b, l in enumerate(lay):
        later[b, sorted(l)[1]:] = True
    g = ko._gen(99)
    q2, k2, v2 = case.q.clone(), case.k.clone(), case.v.clone()
    for t, H in ((q2, Hq), (k2, Hkv), (v2, Hkv)):
        other = ko.bf(torch.randn(len(lay), T, H, D, generator=g) * 3).to(DEV)
        t[~later] = other[~later]
    o1, lse1 = _fwd(case.q, case.k, case.v, case.start)
    o2, lse2 = _fwd(q2, k2, v2, case.start)
    assert torch.equal(o1[later], o2[later])
    assert torch.equal(lse1.transpose(1, 2)[later], lse2.transpose(1, 2)[later])
    assert not torch.equal(o1[~later], o2[~later])
    g1 = _bwd(case.do, case.q, case.k, case.v, o1, lse1, case.start, case.end)
    g2 = _bwd(case.do, q2, k2, v2, o2, lse2, case.start, case.end)
    for a, b_, n in zip(g1, g2, ("dq", "dk", "dv")):
        assert torch.equal(a[later], b_[later]), n


# -------------------------------------------------- joint QKV buffer / fused
@pytest.mark.parametrize("D", DS)
def test_doc_bwd_qkvjoint_writes_only_the_dv_block(D):
    """V read in place from a joint [B, T, Cq+2Ckv] buffer; dV goes into its
    column block of a sentinel-filled joint gradient buffer and every other
    element still holds the sentinel."""
    name = "T1024_gqa_4_2"
    case = _case(name, D)
    T, lay, Hq, Hkv = LAYOUTS[name]
    B = len(lay)
    Cq, Ckv = Hq * D, Hkv * D
    Ctot = Cq + 2 * Ckv + 16
    joint = torch.zeros(B, T, Cq + 2 * Ckv, dtype=BF16, device=DEV)
    joint[..., Cq + Ckv:] = case.v.reshape(B, T, Ckv)
    v_view = joint[..., Cq + Ckv:].view(B, T, Hkv, D)
    assert not v_view.is_contiguous()
    r, _, _ = dm.check_doc_fwd(lambda q, k, v, s: _fwd(q, k, v_view, s), case)
    ko.require(f"doc_vjoint/D{D}/fwd", r)
    SENT = 7.0
    dqkv = torch.full((B, T, Ctot), SENT, dtype=BF16, device=DEV)
    col = Cq + Ckv

    def bwd(do, q, k, v, o_, lse_, start, end):
        dq, dk = EXT.attn_bwd_qkvjoint_doc(do, q, k, v_view, o_, lse_, True,
                                           0, start, end, dqkv, col)
        return dq, dk, dqkv[..., col:col + Ckv].reshape(B, T, Hkv, D)

    ko.require(f"doc_qkvjoint/D{D}", dm.check_doc_bwd(bwd, case))
    outside = torch.cat([dqkv[..., :col], dqkv[..., col + Ckv:]], -1)
    assert (outside == SENT).all(), "wrote outside the dv block"


@pytest.mark.parametrize("D", [64, 80])
def test_doc_fused_qkv_rope_attention_vs_fp64(D):
    """fused_qkv_rope_attention with the document mask against an fp64
    split + RoPE + attention reference; bounds as in
    test_fused_qkv_rope_attention_vs_fp64."""
    import math
    from modalities_amd.ops.attention import fused_qkv_rope_attention
    from modalities_amd.ops.rope import precompute_rope_cos_sin
    g = torch.Generator().manual_seed(D)
    B, T, Hq, Hkv = 2, 300, 4, 2
    start = dm.layouts_to_start([[0, 130, 257], [0, 65]], T, DEV)
    C, KV = Hq * D, Hkv * D
    cos, sin = precompute_rope_cos_sin(T, D, device=DEV)
    qkv = ko.bf(torch.randn(B, T, C + 2 * KV, generator=g)).to(DEV)
    do = ko.bf(torch.randn(B, T, Hq, D, generator=g)).to(DEV)
    a = qkv.clone().requires_grad_(True)
    y = fused_qkv_rope_attention(a, cos, sin, Hq, Hkv, D, doc_start=start)
    y.backward(do)

    qs, ks, vs = qkv.split([C, KV, KV], dim=-1)
    qb = ko.bf(ko.rope_ref64(qs.reshape(B, T, Hq, D), cos, sin, False)[0])
    kb = ko.bf(ko.rope_ref64(ks.reshape(B, T, Hkv, D), cos, sin, False)[0])
    case = dm.DocCase(dict(q=qb, k=kb, do=do,
                           v=vs.reshape(B, T, Hkv, D).contiguous()), start)
    r, _, _ = dm.check_doc_fwd(lambda *_: (y.detach(), case.ref["lse"]), case)
    ko.require(f"doc_fused_qkv/D{D}/fwd", {"o": r["o"]})
    ref, res = case.ref, {}
    got = dict(zip(("dq", "dk", "dv"), a.grad.split([C, KV, KV], dim=-1)))
    for n, H in (("dq", Hq), ("dk", Hkv), ("dv", Hkv)):
        rr = ref[n]
        if n != "dv":
            rr = ko.rope_ref64(rr, cos, sin, True)[0]
        rot = 1.0 if n == "dv" else math.sqrt(2.0)
        peak = ref[n].abs().max().item()
        bound = rot * (2 * case.emul_err[n] + ko.BF16_ULP * peak * 2.0 ** -4
                       + ko.F32_SLACK * ref["C_" + n]) \
            + (0.0 if n == "dv" else ko.BF16_ULP * rot * peak)
        err = (got[n].reshape(B, T, H, D).double() - rr).abs().max().item()
        res[n] = err / bound
    ko.require(f"doc_fused_qkv/D{D}/bwd", res)


# ------------------------------------------------------- argument validation
@pytest.mark.parametrize("D", [64])
def test_doc_rejects_bad_arguments(D):
    from modalities_amd.ops.attention import (flash_attention,
                                              fused_qkv_rope_attention)
    B, T, H = 2, 64, 2
    q = torch.randn(B, T, H, D, device=DEV).to(BF16)
    ds = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    o, lse = _fwd(q, q, q, ds)
    bad = {
        "dtype": ds.long(),
        "shape": ds[:, :T - 1].contiguous(),
        "batch": ds[:1].contiguous(),
        "stride": torch.zeros(T, B, dtype=torch.int32, device=DEV).t(),
        "device": ds.cpu(),
    }
    for what, d in bad.items():
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            flash_attention(q, q, q, doc_start=d)
        with pytest.raises(RuntimeError):
            EXT.attn_fwd_doc(q, q, q, True, 0, d)
        with pytest.raises(RuntimeError):
            EXT.attn_fwd_doc_v2(q, q, q, True, 0, d)
        with pytest.raises(RuntimeError):
            EXT.attn_bwd_doc_v2(q, q, q, q, o, lse, True, 0, d, ds, None)
        with pytest.raises(RuntimeError):
            EXT.attn_bwd_doc_v2(q, q, q, q, o, lse, True, 0, ds, d, None)
    # Tq != Tkv, nonzero offset, causal=False: wrapper and extension
    qs, dss = q[:, :32].contiguous(), ds[:, :32].contiguous()
    with pytest.raises(ValueError, match="Tq == Tkv"):
        flash_attention(qs, q, q, doc_start=dss)
    with pytest.raises(RuntimeError, match="Tq == Tkv"):
        EXT.attn_fwd_doc_v2(qs, q, q, True, 0, dss)
    with pytest.raises(ValueError, match="q_offset"):
        flash_attention(q, q, q, q_offset=1, doc_start=ds)
    with pytest.raises(RuntimeError, match="q_offset"):
        EXT.attn_fwd_doc_v2(q, q, q, True, 1, ds)
    with pytest.raises(ValueError, match="causal"):
        flash_attention(q, q, q, causal=False, doc_start=ds)
    with pytest.raises(RuntimeError, match="causal"):
        EXT.attn_fwd_doc_v2(q, q, q, False, 0, ds)
    with pytest.raises(RuntimeError, match="causal"):
        EXT.attn_bwd_doc_v2(q, q, q, q, o, lse, False, 0, ds, ds, None)
    qkv = torch.randn(B, T, 3 * H * D, device=DEV).to(BF16)
    from modalities_amd.ops.rope import precompute_rope_cos_sin
    cos, sin = precompute_rope_cos_sin(T, D, device=DEV)
    with pytest.raises(TypeError, match="int32"):
        fused_qkv_rope_attention(qkv, cos, sin, H, H, D, doc_start=ds.long())
    # the v1 generation has no document mask
    assert EXT.get_attn_impl() == 2
    EXT.set_attn_impl(1)
    try:
        with pytest.raises(RuntimeError, match="v2"):
            flash_attention(q, q, q, doc_start=ds)
        with pytest.raises(RuntimeError, match="v2"):
            fused_qkv_rope_attention(qkv, cos, sin, H, H, D, doc_start=ds)
        with pytest.raises(RuntimeError, match="v2"):
            EXT.attn_fwd_doc(q, q, q, True, 0, ds)
        with pytest.raises(RuntimeError, match="v2"):
            EXT.attn_bwd_doc(q, q, q, q, o, lse, True, 0, ds, ds, None)
    finally:
        EXT.set_attn_impl(2)
    torch.cuda.synchronize()
    # and the good call still works after all the refusals
    o2, _ = _fwd(q, q, q, ds)
    assert torch.equal(o, o2)


# ------------------------------------------------- custom op: dlse, selective AC
def test_doc_custom_op_backward_accepts_grad_lse():
    name, D = "T520_0_300", 64
    case = _case(name, D, dlse=True)
    q, k, v = (t.clone().requires_grad_(True)
               for t in (case.q, case.k, case.v))
    o, lse = torch.ops.modalities_amd.flash_attention_doc(
        q, k, v, case.start, case.end)
    torch.autograd.backward([o, lse], [case.do, case.dlse])
    want = _bwd(case.do, case.q, case.k, case.v, o.detach(), lse.detach(),
                case.start, case.end, case.dlse)
    for got, w in zip((q.grad, k.grad, v.grad), want):
        assert torch.equal(got, w)
    # the lse gradient is not ignored
    no_dlse = _bwd(case.do, case.q, case.k, case.v, o.detach(), lse.detach(),
                   case.start, case.end)
    assert not torch.equal(q.grad, no_dlse[0])
    # lse alone (grad_o is None)
    q.grad = None
    o, lse = torch.ops.modalities_amd.flash_attention_doc(
        q, k, v, case.start, case.end)
    lse.backward(case.dlse)
    assert torch.isfinite(q.grad.float()).all()


def test_doc_op_is_saved_under_selective_op_checkpointing():
    """Under selective-op activation checkpointing the document-masked
    attention is saved: the backward does not run its forward again."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.training.activation_checkpointing import (
        ActivationCheckpointingVariant, apply_activation_checkpointing_)

    calls = []

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func is torch.ops.modalities_amd.flash_attention_doc.default:
                calls.append(1)
            return func(*args, **(kwargs or {}))

    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=128, n_layer=2, n_head_q=2, n_head_kv=2,
                        n_embd=128, ffn_hidden=256, sequence_length=64,
                        attention_document_masking=True, eod_token_id=5)
    model = GPT2LLM(cfg).to(DEV).to(BF16)
    apply_activation_checkpointing_(
        model, ActivationCheckpointingVariant.SELECTIVE_OP_ACTIVATION_CHECKPOINTING)
    ids = torch.randint(6, 128, (2, 64), device=DEV)
    ids[:, 20] = 5
    with Count():
        out = model({"input_ids": ids})["logits"]
        n_fwd = len(calls)
        out.float().sum().backward()
    assert n_fwd == cfg.n_layer
    assert len(calls) == n_fwd, "attention was recomputed, not saved"
    assert model.wte.weight.grad is not None


# ---------------------------------------------------------------- model level
@pytest.mark.parametrize("fused", [False, True])
def test_doc_model_bf16_no_leak_bitwise(fused):
    """Tiny bf16 GPT2LLM on the GPU with the flag on: logits at B's
    positions do not change, bit for bit, when A's tokens are replaced.
    Both runs have the same shapes, so hipBLASLt runs the same kernels."""
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    torch.manual_seed(0)
    EOD, V, T = 5, 256, 300
    cfg = GPT2LLMConfig(vocab_size=V, n_layer=2, n_head_q=4, n_head_kv=2,
                        n_embd=256, ffn_hidden=512, sequence_length=T,
                        fused_qkv=fused, attention_document_masking=True,
                        eod_token_id=EOD)
    model = GPT2LLM(cfg).to(DEV).to(BF16)
    g = ko._gen(3)
    nb = 171                                       # B starts inside a wave
    b = torch.randint(6, V, (1, T - nb), generator=g)
    a1 = torch.randint(6, V, (1, nb - 1), generator=g)
    a2 = torch.randint(6, V, (1, nb - 1), generator=g)
    eod = torch.tensor([[EOD]])
    ids1 = torch.cat([a1, eod, b], 1).to(DEV)
    ids2 = torch.cat([a2, eod, b], 1).to(DEV)
    with torch.no_grad():
        l1 = model({"input_ids": ids1})["logits"]
        l2 = model({"input_ids": ids2})["logits"]
    assert torch.isfinite(l1.float()).all()
    assert torch.equal(l1[:, nb:], l2[:, nb:])
    assert not torch.equal(l1[:, :nb], l2[:, :nb])
