"""Context parallelism (CP): sequence-sharded attention for long contexts.

The reference only plumbs a cp mesh dimension with NO compute implementation
(reference: src/modalities/running_env/fsdp/device_mesh.py:23,92-145; no ring
attention / Ulysses anywhere — SURVEY.md §5 long-context). This module
implements CP natively for the MI355X node topology: K/V are all-gathered
along the sequence over the CP group (on an 8-GPU fully-connected xGMI node
one all-gather uses all 7 links in parallel; KV bytes per layer at seq 8192 /
GQA-20 heads are ~84 MB — transfer hides behind the block's attention
compute), and each rank computes its Q chunk against the full K/V with an
OFFSET-causal mask (rank r's queries sit at global positions
[r*T_local, (r+1)*T_local)) — on device this runs the K1 HIP flash kernels,
which support Tq != Tkv and the query offset natively.

Memory: block activations, attention state and logits stay 1/cp of the full
sequence; only the transient K/V gather and the embedding output are full-T.
"""

from typing import Optional

import torch
import torch.distributed as dist

from modalities_amd.ops.attention import flash_attention
from modalities_amd.parallel.tp import _GatherSeq


class _SliceSeqPartial(torch.autograd.Function):
    """Replicated -> seq-sharded with PARTIAL backward: grad is zero outside
    this rank's chunk (no communication). This keeps every parameter's CP
    gradient partial — summed across the CP group they equal the full-seq
    gradient, uniformly for embeddings and block weights — so the CP grad
    sync is one all-reduce(SUM) over the cp group (`cp_grad_allreduce_`).

    (TP's _SliceSeq all-gathers instead, because TP replicates the
    downstream compute; CP does not.)"""

    @staticmethod
    def forward(ctx, x, group, dim):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        ctx.dim, ctx.world, ctx.rank = dim, world, rank
        ctx.full_size = x.shape[dim]
        return x.chunk(world, dim=dim)[rank].contiguous()

    @staticmethod
    def backward(ctx, grad):
        shape = list(grad.shape)
        shape[ctx.dim] = ctx.full_size
        full = grad.new_zeros(shape)
        chunk = ctx.full_size // ctx.world
        idx = [slice(None)] * grad.dim()
        idx[ctx.dim] = slice(ctx.rank * chunk, (ctx.rank + 1) * chunk)
        full[tuple(idx)] = grad
        return full, None, None


def cp_attention(q_local: torch.Tensor, k_local: torch.Tensor,
                 v_local: torch.Tensor, group, cp_rank: int, cp_size: int
                 ) -> torch.Tensor:
    """q/k/v: [B, T_local, H, D] (this rank's seq chunk). Returns the local
    attention output [B, T_local, Hq, D]. Backward reduce-scatters dK/dV."""
    if cp_size == 1:
        return flash_attention(q_local, k_local, v_local, causal=True)
    k_full = _GatherSeq.apply(k_local, group, 1)
    v_full = _GatherSeq.apply(v_local, group, 1)
    q_offset = cp_rank * q_local.shape[1]
    return flash_attention(q_local, k_full, v_full, causal=True,
                           q_offset=q_offset)


class _AllToAllSeqHead(torch.autograd.Function):
    """Ulysses exchange: [B, T/cp, H, D] (seq-sharded) <-> [B, T, H/cp, D]
    (head-sharded). One all-to-all over the CP group each direction; on a
    fully-connected 8-GPU xGMI node the 7 pairwise transfers run in
    parallel. Backward is the inverse exchange. gloo (CPU tests) has no
    all_to_all: emulated with all_gather + local slice."""

    @staticmethod
    def _exchange(x, group, to_heads: bool):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        B, T_in, H_in, D = x.shape
        if to_heads:
            # split heads into `world` groups; send seq-chunk i of head-group j
            send = [x[:, :, j * (H_in // world):(j + 1) * (H_in // world)]
                    .contiguous() for j in range(world)]
        else:
            # split seq back into chunks
            send = [c.contiguous() for c in x.chunk(world, dim=1)]
        recv = [torch.empty_like(send[0]) for _ in range(world)]
        backend = dist.get_backend(group) if group is not None else dist.get_backend()
        if backend == "gloo":
            for j in range(world):
                gathered = [torch.empty_like(send[j]) for _ in range(world)]
                dist.all_gather(gathered, send[j], group=group)
                if j == rank:
                    recv = gathered
        else:
            dist.all_to_all(recv, send, group=group)
        return torch.cat(recv, dim=1 if to_heads else 2)

    @staticmethod
    def forward(ctx, x, group, to_heads):
        ctx.group, ctx.to_heads = group, to_heads
        return _AllToAllSeqHead._exchange(x, group, to_heads)

    @staticmethod
    def backward(ctx, grad):
        return (_AllToAllSeqHead._exchange(grad.contiguous(), ctx.group,
                                           not ctx.to_heads), None, None)


def cp_attention_ulysses(q_local, k_local, v_local, group, cp_rank: int,
                         cp_size: int) -> torch.Tensor:
    """Ulysses-style CP: all-to-all scatters HEADS and gathers the full
    sequence, each rank runs plain causal attention on H/cp heads, then the
    inverse all-to-all restores seq sharding. Requires Hq % cp == 0 and
    Hkv % cp == 0 (GQA kv heads must still split)."""
    if cp_size == 1:
        return flash_attention(q_local, k_local, v_local, causal=True)
    Hq, Hkv = q_local.shape[2], k_local.shape[2]
    if Hq % cp_size or Hkv % cp_size:
        raise ValueError(f"Ulysses CP needs Hq ({Hq}) and Hkv ({Hkv}) "
                         f"divisible by cp={cp_size}")
    qh = _AllToAllSeqHead.apply(q_local, group, True)   # [B, T, Hq/cp, D]
    kh = _AllToAllSeqHead.apply(k_local, group, True)
    vh = _AllToAllSeqHead.apply(v_local, group, True)
    oh = flash_attention(qh, kh, vh, causal=True)
    return _AllToAllSeqHead.apply(oh, group, False)     # [B, T/cp, Hq, D]


class _CPAttentionForward:
    """Replacement forward for CausalSelfAttention under CP: x is this
    rank's seq chunk; rope tables are sliced at the rank's global offset."""

    def __init__(self, attn, group, cp_rank: int, cp_size: int,
                 variant: str = "allgather"):
        self.attn = attn
        self.group = group
        self.cp_rank = cp_rank
        self.cp_size = cp_size
        self.variant = variant

    def __call__(self, x: torch.Tensor, rope_cos, rope_sin) -> torch.Tensor:
        attn = self.attn
        B, Tl, C = x.shape
        off = self.cp_rank * Tl
        kv_dim = attn.head_dim * attn.n_head_kv
        if getattr(attn, "fused_qkv", False):
            qkv = attn.qkv_attn(x)
            q, k, v = qkv.split([C, kv_dim, kv_dim], dim=-1)
            q = q.view(B, Tl, attn.n_head_q, attn.head_dim)
            k = k.view(B, Tl, attn.n_head_kv, attn.head_dim)
            v = v.view(B, Tl, attn.n_head_kv, attn.head_dim)
        else:
            q = attn.q_attn(x).view(B, Tl, attn.n_head_q, attn.head_dim)
            k = attn.k_attn(x).view(B, Tl, attn.n_head_kv, attn.head_dim)
            v = attn.v_attn(x).view(B, Tl, attn.n_head_kv, attn.head_dim)
        if attn.q_norm is not None:
            q = attn.q_norm(q)
            k = attn.k_norm(k)
        if rope_cos is not None:
            from modalities_amd.ops import rope_apply
            q = rope_apply(q, rope_cos[off:off + Tl], rope_sin[off:off + Tl])
            k = rope_apply(k, rope_cos[off:off + Tl], rope_sin[off:off + Tl])
        if self.variant == "ulysses":
            y = cp_attention_ulysses(q, k, v, self.group, self.cp_rank,
                                     self.cp_size)
        elif self.variant == "ring":
            y = cp_attention_ring(q, k, v, self.group, self.cp_rank,
                                  self.cp_size)
        else:
            y = cp_attention(q, k, v, self.group, self.cp_rank, self.cp_size)
        y = y.reshape(B, Tl, attn.n_head_q * attn.head_dim)
        return attn.resid_dropout(attn.c_proj(y))


def get_gpt2_context_parallel_model(model, device_mesh=None, group=None,
                                    cp_rank: Optional[int] = None,
                                    cp_size: Optional[int] = None,
                                    variant: str = "allgather"):
    """Patch a GPT2LLM for CP: the model still takes FULL input_ids; the
    residual stream is seq-sliced after the embedding dropout; every
    attention runs offset-causal against all-gathered K/V; logits come back
    seq-sharded [B, T/cp, V] — slice the targets identically
    (`slice_targets_for_cp`)."""
    if device_mesh is not None:
        from modalities_amd.parallel.mesh import ParallelismDegrees
        dim = device_mesh.dims[ParallelismDegrees.CP]
        group, cp_rank, cp_size = dim.group, dim.rank, dim.size
    if cp_size in (None, 1):
        return model
    from modalities_amd.models.gpt2 import refuse_document_masking
    refuse_document_masking(model, "context parallelism")
    if variant not in ("allgather", "ulysses", "ring"):
        raise ValueError(f"Unknown CP variant {variant!r}")
    for block in model.blocks:
        block.attn.forward = _CPAttentionForward(block.attn, group, cp_rank,
                                                 cp_size, variant=variant)
    model.drop.register_forward_hook(
        lambda mod, args, out: _SliceSeqPartial.apply(out, group, 1))
    model._cp_info = (group, cp_rank, cp_size)
    return model


def slice_targets_for_cp(targets: torch.Tensor, cp_rank: int, cp_size: int
                         ) -> torch.Tensor:
    return targets.chunk(cp_size, dim=1)[cp_rank]


@torch.no_grad()
def cp_grad_allreduce_(model, group) -> None:
    """Sum partial CP gradients across the cp group (call after backward +
    backward_epilogue, before the optimizer). With the sharding engine the
    accumulated grads live on the flat per-unit shards; otherwise on
    p.grad."""
    units = getattr(model, "units", None)
    if units is not None:  # XGMIShardedModel: reduce the flat grad shards
        for u in units:
            dist.all_reduce(u.grad_shard, group=group)
        return
    for p in model.parameters():
        if p.grad is not None:
            dist.all_reduce(p.grad, group=group)


class _RingExchange(torch.autograd.Function):
    """One ring step: send the stacked [2, B, Tl, H, D] K/V chunk to rank+1,
    receive from rank-1 (the xGMI p2p link pattern — each step uses one
    neighbor link while attention computes). Backward reverses the ring
    direction, relaying the chunk's gradient back toward its owner."""

    @staticmethod
    def _shift(x, group, direction: int):
        world = dist.get_world_size(group)
        rank = dist.get_rank(group)
        ranks = dist.get_process_group_ranks(group) if group is not None \
            else list(range(world))
        dst = ranks[(rank + direction) % world]
        src = ranks[(rank - direction) % world]
        recv = torch.empty_like(x)
        send_op = dist.P2POp(dist.isend, x.contiguous(), dst, group=group)
        recv_op = dist.P2POp(dist.irecv, recv, src, group=group)
        for work in dist.batch_isend_irecv([send_op, recv_op]):
            work.wait()
        return recv

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        return _RingExchange._shift(x, group, +1)

    @staticmethod
    def backward(ctx, grad):
        return _RingExchange._shift(grad.contiguous(), ctx.group, -1), None


class _GraphTie(torch.autograd.Function):
    """Identity on `out` that adds a zero-gradient dependency on `aux`."""

    @staticmethod
    def forward(ctx, out, aux):
        ctx.aux_shape = aux.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        return grad, grad.new_zeros(ctx.aux_shape)


def _merge_partials(o_a, lse_a, o_b, lse_b):
    """Online-softmax combination of two partial attentions (o in
    [B,T,H,D], lse in [B,H,T]). Merged in fp32 (the lse weights are fp32;
    multiplying bf16 partials by them would silently promote the output)
    and cast back to the partials' dtype by the caller."""
    lse_new = torch.logaddexp(lse_a, lse_b)
    w_a = torch.exp(lse_a - lse_new).permute(0, 2, 1).unsqueeze(-1)
    w_b = torch.exp(lse_b - lse_new).permute(0, 2, 1).unsqueeze(-1)
    return o_a.float() * w_a + o_b.float() * w_b, lse_new


class _FlashWithLse(torch.autograd.Function):
    """K1 kernel pair returning (o, lse), differentiable in BOTH outputs:
    the ring merge weights exp(lse_s - lse_new) make the loss depend on lse,
    and d(lse)/d(score) = P, so dS gains P * dlse — the backward kernels
    take it folded into delta (delta - dlse)."""

    @staticmethod
    def forward(ctx, q, k, v, q_offset):
        from modalities_amd.ops.backend import hip_ext
        o, lse = hip_ext().attn_fwd(q, k, v, True, q_offset)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.q_offset = q_offset
        # an unused output (lse of a lone partial) arrives as None, not zeros
        ctx.set_materialize_grads(False)
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        from modalities_amd.ops.backend import hip_ext
        q, k, v, o, lse = ctx.saved_tensors
        if do is None:
            do = torch.zeros_like(o)
        if dlse is not None:
            dlse = dlse.contiguous()
        dq, dk, dv = hip_ext().attn_bwd(do.contiguous(), q, k, v, o, lse,
                                        True, ctx.q_offset, dlse)
        return dq, dk, dv, None


def _flash_with_lse(q, k, v, q_offset):
    """flash attention that also returns lse (natural log), differentiably.
    On device this is the K1 kernel pair; on CPU a fp32 composed path."""
    from modalities_amd.ops.backend import use_hip
    if use_hip(q, k, v):
        return _FlashWithLse.apply(q.contiguous(), k.contiguous(),
                                   v.contiguous(), q_offset)
    # composed fp32 path (CPU tests): compute scores once, derive o and lse
    import math
    B, T, Hq, D = q.shape
    S, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qf = q.permute(0, 2, 1, 3).float()
    kf = k.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    vf = v.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    att = qf @ kf.transpose(-2, -1) / math.sqrt(D)
    mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(q_offset)
    att = att.masked_fill(~mask, float("-inf"))
    lse = att.logsumexp(-1)                                  # [B,Hq,T]
    o = (att.softmax(-1) @ vf).permute(0, 2, 1, 3).to(q.dtype)
    return o, lse


def _ring_local_attention(q_local, kv_at_step, cp_rank: int, cp_size: int,
                          flash_with_lse=None) -> torch.Tensor:
    """One rank's ring math, free of any process group. kv_at_step(s) returns
    the stacked [2, B, Tl, Hkv, D] K/V chunk this rank holds at step s (chunk
    (cp_rank - s) mod cp_size); it is called for EVERY s in 0..cp_size-1, in
    order, so a communicating provider issues its exchanges identically on
    all ranks. Partials: skipped for chunks after the rank's own, causal
    (q_offset 0) for its own, unmasked (q_offset Tl) for earlier ones;
    merged with the online-softmax rule and cast back to the input dtype.
    flash_with_lse defaults to the production kernel pair; the test oracles
    substitute an emulation and mutants."""
    flash_with_lse = flash_with_lse or _flash_with_lse
    Tl = q_local.shape[1]
    o = lse = None
    for s in range(cp_size):
        kv_cur = kv_at_step(s)
        chunk = (cp_rank - s) % cp_size
        if chunk <= cp_rank:
            off = Tl if chunk < cp_rank else 0  # full vs diagonal-causal
            o_s, lse_s = flash_with_lse(q_local, kv_cur[0], kv_cur[1], off)
            if o is None:
                o, lse = o_s, lse_s
            else:
                o, lse = _merge_partials(o, lse, o_s, lse_s)
    return o.to(q_local.dtype)


def cp_attention_ring(q_local, k_local, v_local, group, cp_rank: int,
                      cp_size: int) -> torch.Tensor:
    """Ring CP (SURVEY.md §7 stage 9): K/V chunks rotate around the ring;
    at step s this rank holds chunk (cp_rank - s) mod cp_size and computes
    a partial attention — full (unmasked) for chunks strictly before its
    queries, causal for its own chunk, skipped for later chunks — merging
    partials with the online-softmax rule. The unmasked case reuses the
    offset-causal kernel with q_offset = Tkv (mask allows every key)."""
    if cp_size == 1:
        return flash_attention(q_local, k_local, v_local, causal=True)
    # K and V travel as ONE stacked tensor: a single sequential exchange
    # chain keeps every rank's backward collectives in the same order (two
    # independent chains could interleave k/v sends differently per rank).
    kv_cur = torch.stack((k_local, v_local))
    held_step = 0

    def kv_at_step(s):
        # called with s = 0 .. cp_size-1 in order: one exchange per new step
        nonlocal kv_cur, held_step
        while held_step < s:  # rotate K/V to the next rank
            kv_cur = _RingExchange.apply(kv_cur, group)
            held_step += 1
        return kv_cur

    o = _ring_local_attention(q_local, kv_at_step, cp_rank, cp_size)
    # Tie the output to the end of the exchange chain: ranks whose queries
    # never attend to a received chunk still must run that exchange's
    # backward (it relays the K/V grads around the ring) — without the tie
    # their autograd graph skips it and the ring deadlocks. Cast back to
    # the input dtype: merged partials are fp32 (ADVICE r1 #1 — on the bf16
    # GPU path every rank that merged >=2 partials would otherwise hand
    # fp32 activations to the following c_proj GEMM).
    return _GraphTie.apply(o, kv_cur)
