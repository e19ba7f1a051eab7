"""CPU tests for the LayerNorm feature: the fp64 oracle of
tests/layernorm_oracles.py accepts the fp32 emulation of a correct kernel and
rejects each deliberate mutant on exactly its own key; the LayerNorm module is
a drop-in for nn.LayerNorm (bit-identical on the CPU, same state dict), and
GPT2 / ViT / CoCa build their norms from it."""

import pytest
import torch
import torch.nn as nn

from modalities_amd.ops import LayerNorm, layer_norm
from modalities_amd.ops.layer_norm import LayerNorm as LayerNormDirect
from tests import layernorm_oracles as lo

SHAPES = [(1, 8), (3, 64), (7, 200), (7, 1000), (257, 64), (7, 8192)]
EPS = [1e-5, 1e-6]


def _bwd(mut=None):
    return lambda dy, x, w, m, r, hb: lo.torch_layernorm_bwd(
        dy, x, w, m, r, hb, mut=mut)


def _fwd(mut=None):
    return lambda x, w, b, eps: lo.torch_layernorm_fwd(x, w, b, eps, mut=mut)


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,H", SHAPES)
def test_correct_emulation_accepted(N, H, bias, eps):
    r = lo.check_layernorm(_fwd(), _bwd(), N, H, eps, "cpu", bias=bias)
    assert set(r) == {"mean", "rstd", "y", "dx", "dw"} | ({"db"} if bias else set())
    lo.require(f"layernorm_emul/N{N}/H{H}/bias{bias}/eps{eps}", r)


def _only_rejected_on(ratios, key):
    bad = sorted(k for k, v in ratios.items() if not v <= 1.0)
    assert bad == [key], f"expected only {key!r} above 1: {ratios}"


@pytest.mark.parametrize("eps", EPS)
def test_mutant_var_one_pass_rejected_on_rstd(eps):
    """E[x^2] - mean^2 at H = 1000: on the constant row the cancellation
    noise of the two sums is far above eps.  (At small H the sums are exact
    and the mutant is indistinguishable: not required there.)"""
    r = lo.check_layernorm(_fwd("var_one_pass"), _bwd(), 7, 1000, eps, "cpu")
    print(r)
    _only_rejected_on(r, "rstd")
    assert r["rstd"] > 100.0


def test_mutant_drop_mean_g_rejected_on_dx():
    r = lo.check_layernorm(_fwd(), _bwd("drop_mean_g"), 3, 64, 1e-5, "cpu")
    print(r)
    _only_rejected_on(r, "dx")
    assert r["dx"] > 100.0


@pytest.mark.parametrize("mut,key", [("dw_last_row", "dw"),
                                     ("db_last_row", "db")])
def test_mutant_last_row_rejected(mut, key):
    r = lo.check_layernorm(_fwd(), _bwd(mut), 3, 200, 1e-5, "cpu")
    print(r)
    _only_rejected_on(r, key)


def test_oracle_forward_only_and_op_checker():
    r = lo.check_layernorm(_fwd(), None, 7, 200, 1e-5, "cpu")
    assert set(r) == {"mean", "rstd", "y"}
    x, w, b, dy = lo.layernorm_inputs(6, 80, "cpu")
    x4, dy4 = x.view(1, 2, 3, 80), dy.view(1, 2, 3, 80)

    # (torch's own CPU bf16 layer_norm keeps mean / rstd in bf16 for the
    # backward and does not meet these bounds; the emulation does)
    class Emul(torch.autograd.Function):
        mut = None

        @staticmethod
        def forward(ctx, x_, w_, b_, eps):
            y, m, r = lo.torch_layernorm_fwd(x_.reshape(-1, 80), w_, b_, eps)
            ctx.save_for_backward(x_, w_, m, r)
            return y.view(x_.shape)

        @staticmethod
        def backward(ctx, dy_):
            x_, w_, m, r = ctx.saved_tensors
            dx, dw, db = lo.torch_layernorm_bwd(
                dy_.reshape(-1, 80), x_.reshape(-1, 80), w_, m, r, True,
                mut=Emul.mut)
            return dx.view(x_.shape), lo.bf(dw), lo.bf(db), None

    lo.require("layernorm_op/emul", lo.check_layernorm_op(
        Emul.apply, x4, w, b, dy4, 1e-5))
    Emul.mut = "drop_mean_g"
    _only_rejected_on(lo.check_layernorm_op(Emul.apply, x4, w, b, dy4, 1e-5),
                      "dx")


# ------------------------------------------------------------------ module
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("bias", [True, False])
def test_module_matches_nn_layernorm_bitwise(dtype, bias):
    torch.manual_seed(0)
    H = 48
    ref = nn.LayerNorm(H, eps=1e-6, bias=bias, dtype=dtype)
    new = LayerNorm(H, eps=1e-6, bias=bias, dtype=dtype)
    assert new.bias is None if not bias else new.bias is not None
    with torch.no_grad():
        ref.weight.copy_(torch.randn(H))
        if bias:
            ref.bias.copy_(torch.randn(H))
    new.load_state_dict(ref.state_dict())
    x = torch.randn(2, 5, H).to(dtype)
    dy = torch.randn(2, 5, H).to(dtype)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = ref(xa), new(xb)
    ya.backward(dy)
    yb.backward(dy)
    assert yb.dtype == dtype and torch.equal(ya, yb)
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(ref.weight.grad, new.weight.grad)
    if bias:
        assert torch.equal(ref.bias.grad, new.bias.grad)


@pytest.mark.parametrize("bias", [True, False])
def test_module_state_dict_interchanges_with_nn_layernorm(bias):
    ref = nn.LayerNorm(32, eps=1e-5, bias=bias)
    new = LayerNorm(32, eps=1e-5, bias=bias)
    sd_ref, sd_new = ref.state_dict(), new.state_dict()
    assert list(sd_ref) == list(sd_new)
    assert [v.shape for v in sd_ref.values()] == [v.shape for v in sd_new.values()]
    assert [n for n, _ in new.named_parameters()] == \
        [n for n, _ in ref.named_parameters()]
    with torch.no_grad():
        new.weight.mul_(3.0)
    ref.load_state_dict(new.state_dict())      # new -> nn
    assert torch.equal(ref.weight, new.weight)
    with torch.no_grad():
        ref.weight.add_(1.0)
    new.load_state_dict(ref.state_dict())      # nn -> new
    assert torch.equal(ref.weight, new.weight)


def test_module_construction_and_reset():
    m = LayerNorm(16, eps=1e-6, bias=True, device="cpu", dtype=torch.bfloat16)
    assert m.weight.dtype == torch.bfloat16 and m.bias.dtype == torch.bfloat16
    assert torch.equal(m.weight, torch.ones(16, dtype=torch.bfloat16))
    assert torch.equal(m.bias, torch.zeros(16, dtype=torch.bfloat16))
    assert "16" in m.extra_repr() and "eps=1e-06" in m.extra_repr() \
        and "bias=True" in m.extra_repr()
    with torch.no_grad():
        m.weight.fill_(7.0)
        m.bias.fill_(7.0)
    m.reset_parameters()
    assert torch.equal(m.weight, torch.ones_like(m.weight))
    assert torch.equal(m.bias, torch.zeros_like(m.bias))
    # the meta-device flow: build on meta, materialise, reset_parameters()
    meta = LayerNorm(16, bias=False, device="meta")
    assert meta.weight.is_meta and meta.bias is None
    real = meta.to_empty(device="cpu")
    real.reset_parameters()
    assert torch.equal(real.weight, torch.ones(16))
    assert LayerNorm is LayerNormDirect


def test_functional_falls_back_to_torch_on_cpu():
    torch.manual_seed(1)
    x, w, b = torch.randn(3, 100), torch.randn(100), torch.randn(100)
    F = torch.nn.functional
    assert torch.equal(layer_norm(x, w, b, 1e-5),
                       F.layer_norm(x, (100,), w, b, 1e-5))
    assert torch.equal(layer_norm(x, w), F.layer_norm(x, (100,), w, None, 1e-5))


# ------------------------------------------------------------------ models
@pytest.mark.parametrize("bias", [True, False])
def test_gpt2_layer_norm_variant_uses_the_module(bias):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    norm = dict(variant="layer_norm", eps=1e-5, bias=bias)
    torch.manual_seed(0)
    model = GPT2LLM(GPT2LLMConfig(
        vocab_size=64, n_layer=2, n_head_q=2, n_head_kv=2, n_embd=32,
        ffn_hidden=64, sequence_length=16, use_qk_norm=True,
        attention_norm_config=norm, ffn_norm_config=norm,
        lm_head_norm_config=norm))
    norms = [model.lm_head_norm]
    for blk in model.blocks:
        norms += [blk.attention_norm, blk.ffn_norm, blk.attn.q_norm,
                  blk.attn.k_norm]
    for n in norms:
        assert type(n) is LayerNorm
        assert (n.bias is not None) == bias and n.eps == 1e-5
    assert model.blocks[0].attn.q_norm.weight.shape == (16,)
    assert not any(isinstance(m, nn.LayerNorm) for m in model.modules())
    keys = set(model.state_dict())
    assert "blocks.0.attention_norm.weight" in keys
    assert ("blocks.0.attention_norm.bias" in keys) == bias
    assert ("blocks.1.attn.k_norm.bias" in keys) == bias
    ids = torch.randint(0, 64, (2, 16))
    out = model({"input_ids": ids})["logits"]
    assert out.shape == (2, 16, 64)
    out.float().mean().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


VIT_KEYS = [
    'blocks.0.attention.c_proj.bias', 'blocks.0.attention.c_proj.weight',
    'blocks.0.attention.wk.bias', 'blocks.0.attention.wk.weight',
    'blocks.0.attention.wq.bias', 'blocks.0.attention.wq.weight',
    'blocks.0.attention.wv.bias', 'blocks.0.attention.wv.weight',
    'blocks.0.mlp.fc1.bias', 'blocks.0.mlp.fc1.weight',
    'blocks.0.mlp.fc2.bias', 'blocks.0.mlp.fc2.weight',
    'blocks.0.norm1.bias', 'blocks.0.norm1.weight',
    'blocks.0.norm2.bias', 'blocks.0.norm2.weight',
    'embedding_fn.cls_token', 'embedding_fn.conv.bias',
    'embedding_fn.conv.weight', 'head.bias', 'head.weight',
    'norm.bias', 'norm.weight', 'positional_embedding_fn.weight']


COCA_KEYS = [
    'attn_pool.attn.c_proj.bias',
    'attn_pool.attn.c_proj.weight',
    'attn_pool.attn.wk.bias',
    'attn_pool.attn.wk.weight',
    'attn_pool.attn.wq.bias',
    'attn_pool.attn.wq.weight',
    'attn_pool.attn.wv.bias',
    'attn_pool.attn.wv.weight',
    'attn_pool.norm.bias',
    'attn_pool.norm.weight',
    'attn_pool.queries',
    'lm_head.weight',
    'logit_scale',
    'multimodal_decoder.blocks.0.attn.c_proj.bias',
    'multimodal_decoder.blocks.0.attn.c_proj.weight',
    'multimodal_decoder.blocks.0.attn.wk.bias',
    'multimodal_decoder.blocks.0.attn.wk.weight',
    'multimodal_decoder.blocks.0.attn.wq.bias',
    'multimodal_decoder.blocks.0.attn.wq.weight',
    'multimodal_decoder.blocks.0.attn.wv.bias',
    'multimodal_decoder.blocks.0.attn.wv.weight',
    'multimodal_decoder.blocks.0.cross_attn.c_proj.bias',
    'multimodal_decoder.blocks.0.cross_attn.c_proj.weight',
    'multimodal_decoder.blocks.0.cross_attn.wk.bias',
    'multimodal_decoder.blocks.0.cross_attn.wk.weight',
    'multimodal_decoder.blocks.0.cross_attn.wq.bias',
    'multimodal_decoder.blocks.0.cross_attn.wq.weight',
    'multimodal_decoder.blocks.0.cross_attn.wv.bias',
    'multimodal_decoder.blocks.0.cross_attn.wv.weight',
    'multimodal_decoder.blocks.0.mlp.fc1.bias',
    'multimodal_decoder.blocks.0.mlp.fc1.weight',
    'multimodal_decoder.blocks.0.mlp.fc2.bias',
    'multimodal_decoder.blocks.0.mlp.fc2.weight',
    'multimodal_decoder.blocks.0.norm1.bias',
    'multimodal_decoder.blocks.0.norm1.weight',
    'multimodal_decoder.blocks.0.norm2.bias',
    'multimodal_decoder.blocks.0.norm2.weight',
    'multimodal_decoder.blocks.0.norm_cross.bias',
    'multimodal_decoder.blocks.0.norm_cross.weight',
    'norm.bias',
    'norm.weight',
    'text_decoder.blocks.0.attn.c_proj.bias',
    'text_decoder.blocks.0.attn.c_proj.weight',
    'text_decoder.blocks.0.attn.wk.bias',
    'text_decoder.blocks.0.attn.wk.weight',
    'text_decoder.blocks.0.attn.wq.bias',
    'text_decoder.blocks.0.attn.wq.weight',
    'text_decoder.blocks.0.attn.wv.bias',
    'text_decoder.blocks.0.attn.wv.weight',
    'text_decoder.blocks.0.mlp.fc1.bias',
    'text_decoder.blocks.0.mlp.fc1.weight',
    'text_decoder.blocks.0.mlp.fc2.bias',
    'text_decoder.blocks.0.mlp.fc2.weight',
    'text_decoder.blocks.0.norm1.bias',
    'text_decoder.blocks.0.norm1.weight',
    'text_decoder.blocks.0.norm2.bias',
    'text_decoder.blocks.0.norm2.weight',
    'text_decoder.wpe.weight',
    'text_decoder.wte.weight',
    'vision_encoder.blocks.0.attention.c_proj.bias',
    'vision_encoder.blocks.0.attention.c_proj.weight',
    'vision_encoder.blocks.0.attention.wk.bias',
    'vision_encoder.blocks.0.attention.wk.weight',
    'vision_encoder.blocks.0.attention.wq.bias',
    'vision_encoder.blocks.0.attention.wq.weight',
    'vision_encoder.blocks.0.attention.wv.bias',
    'vision_encoder.blocks.0.attention.wv.weight',
    'vision_encoder.blocks.0.mlp.fc1.bias',
    'vision_encoder.blocks.0.mlp.fc1.weight',
    'vision_encoder.blocks.0.mlp.fc2.bias',
    'vision_encoder.blocks.0.mlp.fc2.weight',
    'vision_encoder.blocks.0.norm1.bias',
    'vision_encoder.blocks.0.norm1.weight',
    'vision_encoder.blocks.0.norm2.bias',
    'vision_encoder.blocks.0.norm2.weight',
    'vision_encoder.embedding_fn.conv.bias',
    'vision_encoder.embedding_fn.conv.weight',
    'vision_encoder.norm.bias',
    'vision_encoder.norm.weight',
    'vision_encoder.positional_embedding_fn.weight',
]


def test_vit_norms_are_the_module_and_keys_unchanged():
    from modalities_amd.models.vision_transformer import VisionTransformer
    torch.manual_seed(0)
    v = VisionTransformer(img_size=32, n_classes=10, n_layer=1, n_head=2,
                          n_embd=16, ffn_hidden=32, patch_size=16,
                          patch_stride=16)
    for n in (v.norm, v.blocks[0].norm1, v.blocks[0].norm2):
        assert type(n) is LayerNorm and n.eps == 1e-5 and n.bias is not None
    assert sorted(v.state_dict()) == VIT_KEYS
    out = v({"images": torch.randn(2, 3, 32, 32)})["cls_token"]
    assert out.shape == (2, 10)
    out.sum().backward()
    assert v.norm.weight.grad is not None


def test_coca_norms_are_the_module_and_keys_unchanged():
    from modalities_amd.models.coca import CoCa
    torch.manual_seed(0)
    c = CoCa(vocab_size=64, text_block_size=8, n_layer_text=1,
             n_layer_multimodal_text=1, n_head=2, n_embd=16, ffn_hidden=32,
             n_pool_head=2, n_vision_queries=4,
             vision_encoder_config=dict(img_size=32, n_layer=1))
    blk = c.multimodal_decoder.blocks[0]
    for n in (c.norm, c.attn_pool.norm, blk.norm1, blk.norm_cross, blk.norm2,
              c.text_decoder.blocks[0].norm1, c.vision_encoder.norm):
        assert type(n) is LayerNorm and n.eps == 1e-5 and n.bias is not None
    assert not any(isinstance(m, nn.LayerNorm) for m in c.modules())
    assert len(COCA_KEYS) == 80
    assert sorted(c.state_dict()) == COCA_KEYS
    out = c({"images": torch.randn(2, 3, 32, 32),
             "input_ids": torch.randint(0, 64, (2, 8))})
    out["logits"].sum().backward()
    assert c.norm.weight.grad is not None
