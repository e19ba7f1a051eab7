"""GPU numerics tests: every HIP kernel vs a plain PyTorch fp32 reference.

All tests require an MI355X (marked gpu; run via gpurun)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"


def bf(x):
    return x.to(torch.bfloat16)


# ---------------- MFMA layout probe ----------------------------------------
def test_mfma_probe_32x32x16():
    torch.manual_seed(0)
    # asymmetric operands (guide: symmetric B hides transposed layouts)
    a = torch.randn(32, 16, device=DEV) * torch.arange(1, 17, device=DEV) * 0.1
    b = torch.randn(16, 32, device=DEV) + torch.arange(32, device=DEV) * 0.05
    d = EXT.mfma_probe_32x32x16(a.contiguous(), b.contiguous())
    ref = a.to(torch.bfloat16).float() @ b.to(torch.bfloat16).float()
    torch.testing.assert_close(d, ref, rtol=1e-2, atol=1e-2)


# ---------------- RMSNorm ---------------------------------------------------
@pytest.mark.parametrize("shape", [(128, 2560), (1024, 2560), (64, 128)])
def test_rmsnorm_fwd_bwd(shape):
    torch.manual_seed(1)
    N, H = shape
    x = torch.randn(N, H, device=DEV)
    w = torch.randn(H, device=DEV) * 0.1 + 1.0
    xb, wb = bf(x).requires_grad_(True), bf(w).requires_grad_(True)
    y, invrms = EXT.rmsnorm_fwd(xb, wb, 1e-6)

    xf = xb.detach().float().requires_grad_(True)
    wf = wb.detach().float().requires_grad_(True)
    ref = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * wf
    torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=2e-2)

    dy = torch.randn_like(ref)
    ref.backward(dy)
    dx, dw = EXT.rmsnorm_bwd(bf(dy), xb.detach(), wb.detach(), invrms)
    torch.testing.assert_close(dx.float(), xf.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dw.float(), wf.grad, rtol=5e-2,
                               atol=0.05 * wf.grad.abs().max().item() + 1e-3)


# ---------------- RoPE ------------------------------------------------------
def test_rope_fwd_inverse():
    from modalities_amd.ops.rope import precompute_rope_cos_sin, _rope_ref
    torch.manual_seed(2)
    B, T, H, D = 2, 64, 4, 128
    x = torch.randn(B, T, H, D, device=DEV)
    cos, sin = precompute_rope_cos_sin(T, D, device=DEV)
    y = EXT.rope_fwd(bf(x), cos, sin, False)
    ref = _rope_ref(bf(x), cos, sin)
    torch.testing.assert_close(y.float(), ref.float(), rtol=2e-2, atol=2e-2)
    # inverse rotation roundtrips
    back = EXT.rope_fwd(y, cos, sin, True)
    torch.testing.assert_close(back.float(), bf(x).float(), rtol=3e-2, atol=3e-2)


# ---------------- SiLU*mul --------------------------------------------------
def test_silu_mul():
    torch.manual_seed(3)
    g = torch.randn(128, 512, device=DEV)
    u = torch.randn(128, 512, device=DEV)
    out = EXT.silu_mul_fwd(bf(g), bf(u))
    ref = torch.nn.functional.silu(bf(g).float()) * bf(u).float()
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)

    gf = bf(g).float().requires_grad_(True)
    uf = bf(u).float().requires_grad_(True)
    (torch.nn.functional.silu(gf) * uf).backward(torch.ones_like(ref))
    dg, du = EXT.silu_mul_bwd(bf(torch.ones_like(ref)), bf(g), bf(u))
    torch.testing.assert_close(dg.float(), gf.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(du.float(), uf.grad, rtol=3e-2, atol=3e-2)


# ---------------- Cross entropy --------------------------------------------
def test_cross_entropy():
    torch.manual_seed(4)
    N, V = 512, 50304
    logits = torch.randn(N, V, device=DEV) * 2
    targets = torch.randint(0, V, (N,), device=DEV)
    targets[5] = -100
    lb = bf(logits)
    losses, lse = EXT.cross_entropy_fwd(lb, targets, -100)
    n_valid = (targets != -100).sum()
    got = losses.sum() / n_valid

    lf = lb.float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lf, targets, ignore_index=-100)
    torch.testing.assert_close(got, ref.detach(), rtol=1e-2, atol=1e-3)

    ref.backward()
    scale = torch.tensor(1.0 / n_valid.item(), device=DEV)
    dlogits = EXT.cross_entropy_bwd(lb, targets, lse, scale, -100)
    # the softmax part of the gradient is ~1/(N*V) = 4e-8 per element: the
    # absolute tolerance sits far below it, so a kernel that dropped that
    # part (writing only the target column) fails
    torch.testing.assert_close(dlogits.float(), lf.grad, rtol=5e-2, atol=1e-10)


# ---------------- Flash attention -------------------------------------------
def ref_attention(q, k, v, causal=True):
    B, T, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    att = qf @ kf.transpose(-2, -1) / math.sqrt(D)
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool, device=q.device).tril()
        att = att.masked_fill(~mask, float("-inf"))
    att = att.softmax(-1)
    return (att @ vf).permute(0, 2, 1, 3)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("B,T,Hq,Hkv,D", [
    (2, 128, 4, 4, 128),
    (2, 256, 4, 2, 128),
    (1, 200, 4, 1, 128),   # T not a multiple of 128
    (2, 256, 4, 2, 64),
    (1, 4096, 2, 2, 128),  # long sequence
    (2, 256, 4, 2, 80),    # the reference 2.7B head_dim (v2 only)
    (1, 300, 4, 4, 80),
])
def test_attn_fwd(B, T, Hq, Hkv, D, impl):
    if impl == 1 and D == 80:
        pytest.skip("head_dim 80 is v2-only")
    torch.manual_seed(5)
    q = bf(torch.randn(B, T, Hq, D, device=DEV))
    k = bf(torch.randn(B, T, Hkv, D, device=DEV))
    v = bf(torch.randn(B, T, Hkv, D, device=DEV))
    fwd = EXT.attn_fwd_v1 if impl == 1 else EXT.attn_fwd_v2
    o, lse = fwd(q, k, v, True, 0)
    ref = ref_attention(q, k, v)
    torch.testing.assert_close(o.float(), ref, rtol=3e-2, atol=3e-2)
    # lse check
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(Hq // Hkv, dim=1)
    att = qf @ kf.transpose(-2, -1) / math.sqrt(D)
    mask = torch.ones(T, T, dtype=torch.bool, device=DEV).tril()
    att = att.masked_fill(~mask, float("-inf"))
    ref_lse = att.logsumexp(-1)  # [B,Hq,T]
    torch.testing.assert_close(lse, ref_lse, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("impl", [1, 2])
@pytest.mark.parametrize("B,T,Hq,Hkv,D", [
    (2, 128, 4, 4, 128),
    (2, 256, 4, 2, 128),
    (1, 200, 4, 1, 128),
    (2, 256, 4, 2, 64),
    (2, 256, 4, 2, 80),
    (1, 300, 4, 4, 80),
    (2, 192, 8, 2, 80),    # GQA at the reference head_dim
    (1, 1024, 2, 2, 128),
])
def test_attn_bwd(B, T, Hq, Hkv, D, impl):
    if impl == 1 and D == 80:
        pytest.skip("head_dim 80 is v2-only")
    torch.manual_seed(6)
    q = bf(torch.randn(B, T, Hq, D, device=DEV))
    k = bf(torch.randn(B, T, Hkv, D, device=DEV))
    v = bf(torch.randn(B, T, Hkv, D, device=DEV))
    do = bf(torch.randn(B, T, Hq, D, device=DEV))

    fwd = EXT.attn_fwd_v1 if impl == 1 else EXT.attn_fwd_v2
    bwd = EXT.attn_bwd_v1 if impl == 1 else EXT.attn_bwd_v2
    o, lse = fwd(q, k, v, True, 0)
    dq, dk, dv = bwd(do, q, k, v, o, lse, True, 0)

    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    ref = ref_attention(qf, kf, vf)
    ref.backward(do.float())

    torch.testing.assert_close(dq.float(), qf.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dk.float(), kf.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dv.float(), vf.grad, rtol=5e-2, atol=5e-2)


# ---------------- AdamW -----------------------------------------------------
def test_fused_adamw_masked():
    torch.manual_seed(7)
    n = 4096
    p = torch.randn(n, device=DEV)
    g = torch.randn(n, device=DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    mask = (torch.rand(n, device=DEV) > 0.5).float()
    pr, mr, vr = p.clone(), m.clone(), v.clone()

    lr, b1, b2, eps, wd = 1e-3, 0.9, 0.95, 1e-8, 0.1
    for step in (1, 2, 3):
        bc1, bc2 = 1 - b1**step, 1 - b2**step
        EXT.fused_adamw_masked(p, g, m, v, mask, lr, b1, b2, eps, wd, bc1, bc2)
        # torch reference
        pr.mul_(1 - lr * wd * mask)
        mr.mul_(b1).add_(g, alpha=1 - b1)
        vr.mul_(b2).addcmul_(g, g, value=1 - b2)
        pr.add_(-lr / bc1 * mr / ((vr / bc2).sqrt() + eps))
    torch.testing.assert_close(p, pr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m, mr, rtol=1e-5, atol=1e-6)


def test_multi_tensor_norm_scale():
    torch.manual_seed(8)
    ts = [torch.randn(256, device=DEV), torch.randn(512, device=DEV)]
    ref = torch.sqrt(sum(t.pow(2).sum() for t in ts))
    got = EXT.multi_tensor_sqsum(ts).sqrt()
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    s = torch.tensor(0.5, device=DEV)
    refs = [t * 0.5 for t in ts]
    EXT.multi_tensor_scale(ts, s)
    for t, r in zip(ts, refs):
        torch.testing.assert_close(t, r)


# ---------------- end-to-end training step on GPU ---------------------------
def test_gpt2_training_step_gpu():
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    from modalities_amd.optimizers.optimizer_factory import get_adam_w

    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=512, n_layer=2, n_head_q=4, n_head_kv=2,
                        n_embd=512, ffn_hidden=2048, sequence_length=256)
    model = GPT2LLM(cfg)
    dev = torch.device(DEV)
    sharded = XGMIShardedModel.from_transformer(model, dev, blocks_per_unit=1,
                                                param_dtype=torch.bfloat16)
    opt = get_adam_w(sharded, lr=5e-4)
    from modalities_amd.ops import fused_cross_entropy
    losses = []
    g = torch.Generator().manual_seed(42)
    ids = torch.randint(0, 512, (2, 257), generator=g).to(dev)
    x, y = ids[:, :-1], ids[:, 1:]  # same batch: memorization must drive loss down
    for i in range(10):
        out = sharded({"input_ids": x})
        loss = fused_cross_entropy(out["logits"], y)
        loss.backward()
        sharded.backward_epilogue()
        sharded.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 0.5, losses


@pytest.mark.gpu
def test_attn_fwd_forced_rescale():
    """Force the defer-max RESCALE branch (guide rule 26: the branch is rare
    on bounded random data): a spiked K row makes the tile max jump past
    RESCALE_THR=8 at a chosen late tile; output must still match fp32 ref."""
    torch.manual_seed(9)
    B, T, Hq, Hkv, D = 1, 1024, 2, 2, 128
    q = bf(torch.randn(B, T, Hq, D, device=DEV))
    k = bf(torch.randn(B, T, Hkv, D, device=DEV))
    v = bf(torch.randn(B, T, Hkv, D, device=DEV))
    # spike: K row 700 strongly aligned with every q (rank-1 spike)
    direction = torch.randn(D, device=DEV)
    direction = direction / direction.norm()
    k[:, 700] = bf(direction * 60.0)
    q[:, 701:] = bf(q[:, 701:].float() + direction * 2.0)
    o, lse = EXT.attn_fwd(q, k, v, True)
    ref = ref_attention(q, k, v)
    torch.testing.assert_close(o.float(), ref, rtol=3e-2, atol=3e-2)


@pytest.mark.gpu
def test_hipgraph_step_matches_eager():
    """Three graph-replayed training steps must match three eager steps
    (same data, same init): validates the capture of the full step incl.
    the device-resident Adam step counter."""
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.ops import fused_cross_entropy
    from modalities_amd.parallel.fsdp import XGMIShardedModel

    def build():
        torch.manual_seed(0)
        cfg = GPT2LLMConfig(vocab_size=512, n_layer=2, n_head_q=4, n_head_kv=4,
                            n_embd=256, ffn_hidden=512, sequence_length=256)
        model = GPT2LLM(cfg)
        sharded = XGMIShardedModel.from_transformer(
            model, torch.device(DEV), blocks_per_unit=1,
            param_dtype=torch.bfloat16)
        opt = get_adam_w(sharded, lr=1e-3, weight_decay=0.1)
        return sharded, opt

    def batches():
        g = torch.Generator().manual_seed(7)
        return [torch.randint(0, 512, (2, 257), generator=g).to(DEV)
                for _ in range(5)]

    def run_step(sharded, opt, ids):
        out = sharded({"input_ids": ids[:, :-1]})
        loss = fused_cross_entropy(out["logits"], ids[:, 1:])
        loss.backward()
        sharded.backward_epilogue()
        sharded.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad()
        return loss

    # eager reference: 2 warmup + 3 measured steps
    sharded, opt = build()
    data = batches()
    eager_losses = [run_step(sharded, opt, ids).item() for ids in data]

    # graph: warmup on side stream (2 steps), capture, replay 3
    sharded, opt = build()
    data = batches()
    static = torch.zeros_like(data[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for ids in data[:2]:
            static.copy_(ids)
            run_step(sharded, opt, static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    static.copy_(data[2])
    with torch.cuda.graph(graph):
        static_loss = run_step(sharded, opt, static)
    # capture RECORDS but does not execute: every batch (incl. the captured
    # one) is fed through replay
    graph_losses = []
    for ids in data[2:]:
        static.copy_(ids)
        graph.replay()
        torch.cuda.synchronize()
        graph_losses.append(static_loss.item())

    assert eager_losses[2:] == pytest.approx(graph_losses, rel=2e-2), \
        (eager_losses, graph_losses)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [128, 80])
@pytest.mark.parametrize("Tq,Tkv,off", [(128, 512, 0), (128, 512, 128),
                                        (128, 512, 384), (100, 300, 100)])
def test_attn_offset_causal_fwd_bwd(Tq, Tkv, off, D):
    """Context-parallel shape: local q chunk at global key offset `off`
    against full keys (offset-causal). fwd + bwd vs fp32 reference."""
    from modalities_amd.ops.attention import _attention_ref
    torch.manual_seed(11)
    B, Hq, Hkv = 2, 4, 2
    q = bf(torch.randn(B, Tq, Hq, D, device=DEV))
    k = bf(torch.randn(B, Tkv, Hkv, D, device=DEV))
    v = bf(torch.randn(B, Tkv, Hkv, D, device=DEV))
    do = bf(torch.randn(B, Tq, Hq, D, device=DEV))

    o, lse = EXT.attn_fwd(q, k, v, True, off)
    ref = _attention_ref(q.cpu(), k.cpu(), v.cpu(), causal=True, q_offset=off)
    torch.testing.assert_close(o.float().cpu(), ref.float(),
                               rtol=3e-2, atol=3e-2)

    dq, dk, dv = EXT.attn_bwd(do, q, k, v, o, lse, True, off)
    qf = q.float().cpu().requires_grad_(True)
    kf = k.float().cpu().requires_grad_(True)
    vf = v.float().cpu().requires_grad_(True)
    refb = _attention_ref(qf, kf, vf, causal=True, q_offset=off)
    refb.backward(do.float().cpu())
    torch.testing.assert_close(dq.float().cpu(), qf.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dk.float().cpu(), kf.grad, rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(dv.float().cpu(), vf.grad, rtol=5e-2, atol=5e-2)


@pytest.mark.gpu
def test_ring_partial_flash_with_lse():
    """The ring-CP building block on the HIP path: _flash_with_lse with
    q_offset = Tkv (full, unmasked attention against a remote K/V chunk)
    and the online-softmax merge of two partials equal one full causal
    attention over the concatenated K/V."""
    from modalities_amd.parallel.cp import _flash_with_lse, _merge_partials
    from modalities_amd.ops.attention import _attention_ref
    torch.manual_seed(11)
    B, Tl, Hq, Hkv, D = 2, 128, 4, 2, 128
    dev = "cuda"
    q1 = torch.randn(B, Tl, Hq, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn(B, 2 * Tl, Hkv, D, device=dev, dtype=torch.bfloat16)
    v = torch.randn(B, 2 * Tl, Hkv, D, device=dev, dtype=torch.bfloat16)
    # rank-1's view: full attention over chunk 0, causal over chunk 1
    o_full, lse_full = _flash_with_lse(q1, k[:, :Tl], v[:, :Tl], Tl)
    o_diag, lse_diag = _flash_with_lse(q1, k[:, Tl:], v[:, Tl:], 0)
    o, _ = _merge_partials(o_full.float(), lse_full, o_diag.float(), lse_diag)
    ref = _attention_ref(q1, k, v, causal=True, q_offset=Tl)
    torch.testing.assert_close(o.to(torch.bfloat16), ref, rtol=2e-2, atol=2e-2)


@pytest.mark.gpu
def test_deferred_clip_scale_matches_eager():
    """The gscale argument of the fused devstep kernel (deferred grad-clip
    coefficient) must give bit-identical results to pre-scaling the grads
    with multi_tensor_scale_ and stepping without gscale. (Kernel-level
    check: full-model reruns are not bitwise reproducible — fp32 atomics
    in the backward reductions.)"""
    from modalities_amd.ops.backend import hip_ext
    torch.manual_seed(5)
    n = 4096 * 3
    dev = DEV
    p0 = torch.randn(n, device=dev)
    g0 = torch.randn(n, device=dev)
    m0 = torch.randn(n, device=dev).abs() * 0.01
    v0 = torch.randn(n, device=dev).abs() * 0.001
    mask = (torch.rand(n, device=dev) > 0.3).float()
    step = torch.tensor(3, dtype=torch.int32, device=dev)
    scale = torch.tensor(0.0371, device=dev)
    args = dict(lr=3e-4, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)

    def run(pre_scale):
        p, g, m, v = (t.clone() for t in (p0, g0, m0, v0))
        out = torch.empty(n, device=dev, dtype=torch.bfloat16)
        if pre_scale:
            hip_ext().multi_tensor_scale([g], scale)
            gs = None
        else:
            gs = scale
        hip_ext().fused_adamw_masked_devstep(
            p, g, m, v, mask, step, out, gs, args["lr"], args["b1"],
            args["b2"], args["eps"], args["wd"])
        return p, m, v, out

    a, b = run(False), run(True)
    for ta, tb in zip(a, b):
        torch.testing.assert_close(ta, tb, rtol=0, atol=0)

@pytest.mark.gpu
def test_fused_qkv_rope_attention_matches_unfused():
    """The joint-buffer fused path (slice RoPE + attention with in-place
    dqkv assembly) must match split + rope_apply + flash_attention in both
    output and the gradient w.r.t. the joint QKV activation."""
    from modalities_amd.ops.attention import fused_qkv_rope_attention
    from modalities_amd.ops.rope import precompute_rope_cos_sin, rope_apply
    from modalities_amd.ops.attention import flash_attention
    torch.manual_seed(3)
    B, T, Hq, Hkv, D = 2, 256, 4, 2, 128
    C, KV = Hq * D, Hkv * D
    cos, sin = precompute_rope_cos_sin(T, D, device=DEV)
    qkv = torch.randn(B, T, C + 2 * KV, device=DEV, dtype=torch.bfloat16)

    a = qkv.clone().requires_grad_(True)
    y_f = fused_qkv_rope_attention(a, cos, sin, Hq, Hkv, D)
    do = torch.randn_like(y_f)
    y_f.backward(do)

    b = qkv.clone().requires_grad_(True)
    q, k, v = b.split([C, KV, KV], dim=-1)
    q = rope_apply(q.reshape(B, T, Hq, D).contiguous(), cos, sin)
    k = rope_apply(k.reshape(B, T, Hkv, D).contiguous(), cos, sin)
    y_u = flash_attention(q, k, v.reshape(B, T, Hkv, D).contiguous(),
                          causal=True)
    y_u.backward(do)

    torch.testing.assert_close(y_f, y_u, rtol=0, atol=0)
    torch.testing.assert_close(a.grad, b.grad, rtol=0, atol=0)


def test_silu_mul_joint_gpu():
    from modalities_amd.ops.swiglu import silu_mul_joint
    torch.manual_seed(12)
    wv = bf(torch.randn(4, 8, 256, device=DEV)).requires_grad_(True)
    y = silu_mul_joint(wv)
    g, u = wv[..., :128].float(), wv[..., 128:].float()
    ref = torch.nn.functional.silu(g) * u
    torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=2e-2)
    do = bf(torch.randn_like(y))
    y.backward(do)
    wv2 = wv.detach().float().requires_grad_(True)
    g2, u2 = wv2[..., :128], wv2[..., 128:]
    (torch.nn.functional.silu(g2) * u2).backward(do.float())
    torch.testing.assert_close(wv.grad.float(), wv2.grad, rtol=3e-2, atol=3e-2)


def test_flash_attention_custom_op_and_selective_ac_save():
    """flash_attention goes through the torch.library op on the HIP path
    (dispatcher-visible) and the selective-op AC save-list contains it —
    its output is SAVED, not recomputed."""
    import torch

    from modalities_amd.ops.attention import _ensure_custom_op, flash_attention
    from modalities_amd.training.activation_checkpointing import _get_save_list
    assert _ensure_custom_op()
    assert torch.ops.modalities_amd.flash_attention.default in _get_save_list()
    torch.manual_seed(3)
    q = bf(torch.randn(1, 128, 2, 128, device=DEV)).requires_grad_(True)
    k = bf(torch.randn(1, 128, 2, 128, device=DEV)).requires_grad_(True)
    v = bf(torch.randn(1, 128, 2, 128, device=DEV)).requires_grad_(True)
    y = flash_attention(q, k, v, causal=True)
    y.sum().backward()
    assert q.grad is not None and k.grad is not None and v.grad is not None

    # end-to-end: a selective-op checkpointed block trains
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.training.activation_checkpointing import (
        ActivationCheckpointingVariant, apply_activation_checkpointing_)
    torch.manual_seed(0)
    model = GPT2LLM(GPT2LLMConfig(
        vocab_size=512, n_layer=2, n_head_q=4, n_head_kv=4, n_embd=512,
        ffn_hidden=2048, sequence_length=256)).to(DEV).bfloat16()
    apply_activation_checkpointing_(
        model, ActivationCheckpointingVariant.SELECTIVE_OP_ACTIVATION_CHECKPOINTING)
    ids = torch.randint(0, 512, (2, 256), device=DEV)
    out = model({"input_ids": ids})["logits"]
    out.float().mean().backward()
    assert model.wte.weight.grad is not None


@pytest.mark.gpu
def test_two_stream_linear_row_bound_matches_plain():
    """Above _TWO_STREAM_MAX_ROWS the linear backward must take the plain
    sequential path (two chip-filling hipBLASLt kernels co-running on
    concurrent streams can wedge the device — the mbs>=3 hang), and its
    gradients must match nn.Linear on both sides of the bound."""
    import torch.nn as nn

    from modalities_amd.ops import linear as tsl

    torch.manual_seed(0)
    for rows in (4096, tsl._TWO_STREAM_MAX_ROWS + 64):
        ref = nn.Linear(256, 512, bias=True, device=DEV, dtype=torch.bfloat16)
        two = tsl.TwoStreamLinear(256, 512, bias=True, device=DEV,
                                  dtype=torch.bfloat16)
        with torch.no_grad():
            two.weight.copy_(ref.weight)
            two.bias.copy_(ref.bias)
        x1 = torch.randn(rows, 256, device=DEV, dtype=torch.bfloat16,
                         requires_grad=True)
        x2 = x1.detach().clone().requires_grad_(True)
        ref(x1).float().square().mean().backward()
        two(x2).float().square().mean().backward()
        torch.cuda.synchronize()
        torch.testing.assert_close(x1.grad, x2.grad, rtol=0, atol=0)
        torch.testing.assert_close(ref.weight.grad, two.weight.grad,
                                   rtol=0, atol=0)
        torch.testing.assert_close(ref.bias.grad, two.bias.grad, rtol=0, atol=0)


@pytest.mark.gpu
def test_kv_cache_decode_matches_full_reforward_gpu():
    """KV-cache decode on the HIP flash path (q_offset attention against
    the cache prefix) must match the full re-forward in bf16."""
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig

    torch.manual_seed(3)
    model = GPT2LLM(GPT2LLMConfig(
        vocab_size=128, n_layer=2, n_head_q=4, n_head_kv=2, n_embd=512,
        ffn_hidden=1024, sequence_length=256, seed=7, dropout=0.0,
        fused_qkv=True)).to(DEV).to(torch.bfloat16).eval()

    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, 128, (2, 100), generator=g).to(DEV)

    with torch.no_grad():
        cache = model.new_kv_cache(2, max_len=160)
        out_c = model.forward_cached({"input_ids": prompt}, cache)["logits"]
        ref = model({"input_ids": prompt})["logits"]
        torch.testing.assert_close(out_c.float(), ref.float(),
                                   rtol=2e-2, atol=2e-2)
        ids = prompt
        for _ in range(8):
            nxt = ref[:, -1, :].argmax(-1, keepdim=True)
            ids = torch.cat([ids, nxt], dim=1)
            ref = model({"input_ids": ids})["logits"]
            out_c = model.forward_cached({"input_ids": nxt}, cache)["logits"]
            torch.testing.assert_close(out_c[:, -1].float(),
                                       ref[:, -1].float(),
                                       rtol=2e-2, atol=2e-2)
