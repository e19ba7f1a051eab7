"""Flash-style causal attention (K1): MFMA/LDS-tiled fwd+bwd, GQA-aware.

HIP kernels: csrc/attention_v2.hip is the perf path (8 waves, 2 waves/SIMD;
head_dim 64/80/128); csrc/attention_fwd.hip / csrc/attention_bwd.hip are the
v1 generation kept for A/B (head_dim 64/128), selected with set_attn_impl /
MA_ATTN_IMPL. Both use online-softmax tiling per the CDNA4 guide (swapped
QK^T for lane-local softmax rows, ds_read_b64_tr_b16 for V; v1 XOR-swizzles
the K LDS image, v2 pads the LDS pitch). The backward takes an optional dlse
(gradient of the log-sum-exp output), folded into the delta preprocess.

Replaces both attention paths of the reference (reference:
src/modalities/models/gpt2/gpt2_model.py:595-658 — flash_attn_func wheel and
torch SDPA) with a single native kernel; GQA without K/V head repetition
(the reference's PYTORCH_FLASH path materializes repeated KV heads,
gpt2_model.py:550-593).

Layout: q [B, T, Hq, D]; k, v [B, T, Hkv, D]; Hq % Hkv == 0. Causal only
(decoder LM pretraining); the CPU fallback handles the general case for
tests.

Document masking (packed sequences): with doc_start [B, T] int32 given,
query i sees exactly the keys doc_start[b, i] <= j <= i. `document_starts`
derives it from the token ids (the eod token belongs to the document it
ends). The v2 kernels take the bound per softmax row and its key-side mirror
doc_end[b, j] (last query of j's document) in the dK/dV kernel; they skip
the tiles outside a document, so the work falls from T^2/2 to about T*L/2
for documents of length L. Positions are not reset at document starts.

Decoding (csrc/attention_decode.hip): `decode_attention` is single-token
attention over a preallocated KV cache, split over the keys (one workgroup
per batch row, kv head and chunk of keys, then a combine launch), with the
per-row lengths in a device tensor; `decode_rope_append` rotates the new
token's q and k at a device-side position and appends k and v to the cache
in one launch. Neither takes a host-side position, so a decode step can be
captured once into a hipGraph and replayed per token. `set_decode_attention`
/ MA_DECODE_ATTN=0 switch the model back to the prefill kernel for A/B."""

import math
import os
import weakref
from typing import Optional

import torch

from modalities_amd.ops.backend import use_hip, hip_ext


def document_starts(input_ids: torch.Tensor, eod_token_id: int) -> torch.Tensor:
    """int32 [B, T]: start[b, i] = max({0} U {p + 1 : p < i and
    input_ids[b, p] == eod}) -- the first position of the document that
    token i belongs to (an eod token closes its own document). Device-side
    ops only: no host sync, capturable in a hipGraph."""
    if input_ids.dim() != 2:
        raise ValueError("document_starts: input_ids must be [B, T]")
    B, T = input_ids.shape
    pos = torch.arange(T, dtype=torch.int32, device=input_ids.device)
    after_eod = torch.zeros(B, T, dtype=torch.bool, device=input_ids.device)
    after_eod[:, 1:] = input_ids[:, :-1] == eod_token_id
    first = torch.where(after_eod, pos, torch.zeros_like(pos))
    return torch.cummax(first, dim=1).values.contiguous()


def document_ends(doc_start: torch.Tensor) -> torch.Tensor:
    """int32 [B, T]: end[b, j] = the last i with start[b, i] == start[b, j]
    (the key-side bound the dK/dV kernel needs). Device-side ops only."""
    B, T = doc_start.shape
    pos = torch.arange(T, dtype=torch.int32, device=doc_start.device)
    last = torch.ones(B, T, dtype=torch.bool, device=doc_start.device)
    last[:, :-1] = doc_start[:, 1:] != doc_start[:, :-1]
    cand = torch.where(last, pos, torch.full_like(pos, T - 1))
    return torch.cummin(cand.flip(1), dim=1).values.flip(1).contiguous()


_DOC_END_CACHE = None  # (weakref(doc_start), its version, doc_end)


def _document_ends_cached(doc_start: torch.Tensor) -> torch.Tensor:
    """document_ends, derived once per doc_start tensor: every layer of a
    model hands over the same tensor, and so does a checkpoint recompute."""
    global _DOC_END_CACHE
    c = _DOC_END_CACHE
    if c is not None and c[0]() is doc_start and c[1] == doc_start._version:
        return c[2]
    doc_end = document_ends(doc_start)
    _DOC_END_CACHE = (weakref.ref(doc_start), doc_start._version, doc_end)
    return doc_end


def _doc_visible(doc_start: torch.Tensor) -> torch.Tensor:
    """bool [B, 1, T, T]: key j visible to query i iff start[b,i] <= j <= i."""
    T = doc_start.shape[1]
    j = torch.arange(T, device=doc_start.device)
    return ((j[None, None, :] >= doc_start[:, :, None])
            & (j[None, None, :] <= j[None, :, None]))[:, None]


def _check_doc_args(q, k, causal, q_offset, doc_start):
    if not causal:
        raise ValueError("doc_start requires causal=True")
    if q.shape[1] != k.shape[1]:
        raise ValueError(f"doc_start requires Tq == Tkv, got {q.shape[1]} "
                         f"and {k.shape[1]}")
    if q_offset not in (None, 0):
        raise ValueError(f"doc_start requires q_offset 0 or None, got {q_offset}")
    if not isinstance(doc_start, torch.Tensor) or doc_start.dtype != torch.int32:
        raise TypeError("doc_start must be an int32 tensor")
    if doc_start.device != q.device:
        raise ValueError(f"doc_start is on {doc_start.device}, q on {q.device}")
    if tuple(doc_start.shape) != (q.shape[0], q.shape[1]):
        raise ValueError(f"doc_start must be [B, T] = "
                         f"{(q.shape[0], q.shape[1])}, got {tuple(doc_start.shape)}")
    if not doc_start.is_contiguous():
        raise ValueError("doc_start must be contiguous")


def _require_v2_for_doc():
    if hip_ext().get_attn_impl() != 2:
        raise RuntimeError("document masking needs the v2 attention kernels; "
                           "the v1 generation is selected (set_attn_impl / "
                           "MA_ATTN_IMPL)")


def _attention_ref(q, k, v, causal=True, q_offset=None, doc_start=None):
    # q: [B, T, Hq, D], k/v: [B, S, Hkv, D] -> [B, T, Hq, D]; fp32 compute.
    # q_offset: global position of q row 0 relative to k row 0 (context
    # parallelism); default aligns the q block to the END of the keys.
    # doc_start: int32 [B, T] document mask (dense here).
    B, T, Hq, D = q.shape
    S, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qf = q.permute(0, 2, 1, 3).float()                      # [B,Hq,T,D]
    kf = k.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    vf = v.permute(0, 2, 1, 3).float().repeat_interleave(rep, dim=1)
    att = qf @ kf.transpose(-2, -1) / math.sqrt(D)          # [B,Hq,T,S]
    if causal:
        diag = (S - T) if q_offset is None else q_offset
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(diag)
        att = att.masked_fill(~mask, float("-inf"))
    if doc_start is not None:
        att = att.masked_fill(~_doc_visible(doc_start), float("-inf"))
    att = att.softmax(-1)
    out = att @ vf                                          # [B,Hq,T,D]
    return out.permute(0, 2, 1, 3).to(q.dtype)


class _FlashAttnHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, q_offset):
        o, lse = hip_ext().attn_fwd(q, k, v, causal, q_offset)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal = causal
        ctx.q_offset = q_offset
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = hip_ext().attn_bwd(do.contiguous(), q, k, v, o, lse,
                                        ctx.causal, ctx.q_offset)
        return dq, dk, dv, None, None


# ---------------------------------------------------------------------------
# Dispatcher-visible registration: a raw autograd.Function is opaque to
# torch dispatch, so selective-op activation checkpointing could never SAVE
# the attention output (it was always recomputed).
# Registering the op through torch.library lets the AC save-list match it.
# ---------------------------------------------------------------------------

_CUSTOM_OP_READY = False


def _ensure_custom_op():
    global _CUSTOM_OP_READY
    if _CUSTOM_OP_READY:
        return True
    try:
        @torch.library.custom_op("modalities_amd::flash_attention",
                                 mutates_args=())
        def _op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                causal: bool, q_offset: int) -> tuple[torch.Tensor, torch.Tensor]:
            o, lse = hip_ext().attn_fwd(q, k, v, causal, q_offset)
            return o, lse

        @_op.register_fake
        def _(q, k, v, causal, q_offset):
            B, T, Hq, _ = q.shape
            return (torch.empty_like(q),
                    q.new_empty((B, Hq, T), dtype=torch.float32))

        def _setup(ctx, inputs, output):
            q, k, v, causal, q_offset = inputs
            ctx.save_for_backward(q, k, v, output[0], output[1])
            ctx.causal = causal
            ctx.q_offset = q_offset
            # flash_attention drops lse: its grad arrives as None, not zeros
            ctx.set_materialize_grads(False)

        def _bwd(ctx, grad_o, grad_lse):
            q, k, v, o, lse = ctx.saved_tensors
            if grad_o is None:
                grad_o = torch.zeros_like(o)
            if grad_lse is not None:
                grad_lse = grad_lse.contiguous()
            dq, dk, dv = hip_ext().attn_bwd(grad_o.contiguous(), q, k, v, o,
                                            lse, ctx.causal, ctx.q_offset,
                                            grad_lse)
            return dq, dk, dv, None, None

        _op.register_autograd(_bwd, setup_context=_setup)

        # document-masked variant: a second op, so the schema above stays
        # as it is (causal, offset 0 and Tq == Tkv are implied)
        @torch.library.custom_op("modalities_amd::flash_attention_doc",
                                 mutates_args=())
        def _op_doc(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    doc_start: torch.Tensor, doc_end: torch.Tensor
                    ) -> tuple[torch.Tensor, torch.Tensor]:
            o, lse = hip_ext().attn_fwd_doc(q, k, v, True, 0, doc_start)
            return o, lse

        @_op_doc.register_fake
        def _(q, k, v, doc_start, doc_end):
            B, T, Hq, _ = q.shape
            return (torch.empty_like(q),
                    q.new_empty((B, Hq, T), dtype=torch.float32))

        def _setup_doc(ctx, inputs, output):
            q, k, v, doc_start, doc_end = inputs
            ctx.save_for_backward(q, k, v, output[0], output[1], doc_start,
                                  doc_end)
            ctx.set_materialize_grads(False)

        def _bwd_doc(ctx, grad_o, grad_lse):
            q, k, v, o, lse, doc_start, doc_end = ctx.saved_tensors
            if grad_o is None:
                grad_o = torch.zeros_like(o)
            if grad_lse is not None:
                grad_lse = grad_lse.contiguous()
            dq, dk, dv = hip_ext().attn_bwd_doc(
                grad_o.contiguous(), q, k, v, o, lse, True, 0, doc_start,
                doc_end, grad_lse)
            return dq, dk, dv, None, None

        _op_doc.register_autograd(_bwd_doc, setup_context=_setup_doc)
        _CUSTOM_OP_READY = True
    except Exception:  # older torch without torch.library.custom_op
        _CUSTOM_OP_READY = False
    return _CUSTOM_OP_READY


class _FlashAttnDocHip(torch.autograd.Function):
    """Document-masked attention without torch.library (older torch)."""

    @staticmethod
    def forward(ctx, q, k, v, doc_start, doc_end):
        o, lse = hip_ext().attn_fwd_doc(q, k, v, True, 0, doc_start)
        ctx.save_for_backward(q, k, v, o, lse, doc_start, doc_end)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, doc_start, doc_end = ctx.saved_tensors
        dq, dk, dv = hip_ext().attn_bwd_doc(do.contiguous(), q, k, v, o, lse,
                                            True, 0, doc_start, doc_end)
        return dq, dk, dv, None, None


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    causal: bool = True,
                    q_offset: Optional[int] = None,
                    doc_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal flash attention. q: [B,T,Hq,D]; k,v: [B,S,Hkv,D].

    q_offset (context parallelism): global key position of q row 0; None =
    classic alignment (q block ends at the last key, i.e. offset S-T).
    The HIP kernels handle Tq != Tkv and offsets natively.

    doc_start (packed sequences): contiguous int32 [B, T] on q's device,
    non-decreasing with doc_start[b, i] <= i (see `document_starts`); query
    i then sees exactly the keys doc_start[b, i] <= j <= i. Needs
    causal=True, Tq == Tkv, an offset of 0 or None, and the v2 kernels."""
    if doc_start is not None:
        _check_doc_args(q, k, causal, q_offset, doc_start)
        if use_hip(q, k, v):
            _require_v2_for_doc()
            doc_end = _document_ends_cached(doc_start)
            if _ensure_custom_op():
                o, _ = torch.ops.modalities_amd.flash_attention_doc(
                    q.contiguous(), k.contiguous(), v.contiguous(),
                    doc_start, doc_end)
                return o
            return _FlashAttnDocHip.apply(q.contiguous(), k.contiguous(),
                                          v.contiguous(), doc_start, doc_end)
        if q.is_cuda:
            rep = q.shape[2] // k.shape[2]
            y = torch.nn.functional.scaled_dot_product_attention(
                q.transpose(1, 2),
                k.transpose(1, 2).repeat_interleave(rep, dim=1),
                v.transpose(1, 2).repeat_interleave(rep, dim=1),
                attn_mask=_doc_visible(doc_start))
            return y.transpose(1, 2)
        return _attention_ref(q, k, v, True, doc_start=doc_start)
    if use_hip(q, k, v):
        off = q_offset
        if off is None:
            off = k.shape[1] - q.shape[1]  # classic alignment (q at the end)
        if _ensure_custom_op():
            o, _ = torch.ops.modalities_amd.flash_attention(
                q.contiguous(), k.contiguous(), v.contiguous(), causal, off)
            return o
        return _FlashAttnHip.apply(q.contiguous(), k.contiguous(),
                                   v.contiguous(), causal, off)
    if q.is_cuda:
        # SDPA fallback (MODALITIES_AMD_FORCE_EAGER debug path)
        B, T, Hq, D = q.shape
        S, Hkv = k.shape[1], k.shape[2]
        rep = Hq // Hkv
        qt = q.transpose(1, 2)
        kt = k.transpose(1, 2).repeat_interleave(rep, dim=1)
        vt = v.transpose(1, 2).repeat_interleave(rep, dim=1)
        diag = (S - T) if q_offset is None else q_offset
        mask = torch.ones(T, S, dtype=torch.bool, device=q.device).tril(
            diag if causal else S)
        y = torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, attn_mask=mask)
        return y.transpose(1, 2)
    return _attention_ref(q, k, v, causal, q_offset=q_offset)


class _FusedQKVRopeAttn(torch.autograd.Function):
    """Fused split + RoPE + flash attention over a joint QKV activation
    [B, T, Cq+Ck+Cv] (HIP path only).

    Forward RoPEs the q/k column blocks straight out of the joint tensor
    (slice-aware rope kernel: no .contiguous() copies of the slices).
    Backward assembles the joint dqkv gradient in place: the attention
    backward stores dv directly into its column block, and the inverse-RoPE
    kernel scatters dq/dk into theirs — eliminating the per-layer backward
    torch.cat (measured 2.5 ms/step on the 2.7B config) plus the forward
    q/k slice copies."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, Hq, Hkv, D, doc_start=None, doc_end=None):
        ext = hip_ext()
        B, T, _ = qkv.shape
        C, KV = Hq * D, Hkv * D
        qkv = qkv.contiguous()
        q = ext.rope_fwd_slice(qkv, cos, sin, 0, Hq, D, False)
        k = ext.rope_fwd_slice(qkv, cos, sin, C, Hkv, D, False)
        # V stays a row-strided view into the joint activation: the v2
        # kernels read it in place (no per-layer 2*B*T*KV copy)
        v = qkv[..., C + KV:].view(B, T, Hkv, D)
        if doc_start is None:
            o, lse = ext.attn_fwd(q, k, v, True, 0)
            ctx.save_for_backward(q, k, v, o, lse, cos, sin)
        else:
            o, lse = ext.attn_fwd_doc(q, k, v, True, 0, doc_start)
            ctx.save_for_backward(q, k, v, o, lse, cos, sin, doc_start,
                                  doc_end)
        ctx.dims = (Hq, Hkv, D)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, cos, sin, *doc = ctx.saved_tensors
        Hq, Hkv, D = ctx.dims
        C, KV = Hq * D, Hkv * D
        B, T = q.shape[0], q.shape[1]
        ext = hip_ext()
        dqkv = torch.empty(B, T, C + 2 * KV, dtype=q.dtype, device=q.device)
        if doc:
            dq, dk = ext.attn_bwd_qkvjoint_doc(do.contiguous(), q, k, v, o,
                                               lse, True, 0, doc[0], doc[1],
                                               dqkv, C + KV)
        else:
            dq, dk = ext.attn_bwd_qkvjoint(do.contiguous(), q, k, v, o, lse,
                                           True, 0, dqkv, C + KV)
        ext.rope_bwd_slice(dq, cos, sin, dqkv, 0)
        ext.rope_bwd_slice(dk, cos, sin, dqkv, C)
        return dqkv, None, None, None, None, None, None, None


def fused_qkv_rope_attention(qkv: torch.Tensor, cos: torch.Tensor,
                             sin: torch.Tensor, n_head_q: int, n_head_kv: int,
                             head_dim: int,
                             doc_start: Optional[torch.Tensor] = None
                             ) -> torch.Tensor:
    """Causal flash attention taking the joint QKV projection output
    directly; returns [B, T, n_head_q, head_dim]. HIP/GPU only — callers
    fall back to split + rope_apply + flash_attention elsewhere.
    doc_start: the document mask of `flash_attention`, same contract."""
    if doc_start is None:
        return _FusedQKVRopeAttn.apply(qkv, cos, sin, n_head_q, n_head_kv,
                                       head_dim)
    if qkv.dim() != 3:
        raise ValueError("qkv must be [B, T, Cq + 2*Ckv]")
    _check_doc_args(qkv, qkv, True, 0, doc_start)
    _require_v2_for_doc()
    return _FusedQKVRopeAttn.apply(qkv, cos, sin, n_head_q, n_head_kv,
                                   head_dim, doc_start,
                                   _document_ends_cached(doc_start))


# ---------------------------------------------------------------------------
# Decoding: split-KV single-token attention over a KV cache
# ---------------------------------------------------------------------------

_DECODE_ATTN = os.environ.get("MA_DECODE_ATTN", "1") != "0"

DECODE_HEAD_DIMS = (64, 80, 128)


def set_decode_attention(on: bool) -> None:
    """Route single-token decode steps through the split-KV decode kernels
    (default) or, with False, through the prefill kernel as before (A/B).
    MA_DECODE_ATTN=0 sets the initial value."""
    global _DECODE_ATTN
    _DECODE_ATTN = bool(on)


def decode_attention_enabled() -> bool:
    return _DECODE_ATTN


def _check_index_arg(name, t, ref, B):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name} must be an int32 tensor")
    if t.device != ref.device:
        raise ValueError(f"{name} is on {t.device}, q on {ref.device}")
    if tuple(t.shape) != (B,):
        raise ValueError(f"{name} must be [B] = {(B,)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_decode_args(q, k_cache, v_cache, kv_lens):
    if q.dim() != 4 or q.shape[1] != 1:
        raise ValueError(f"q must be [B, 1, Hq, D], got {tuple(q.shape)}")
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape:
        raise ValueError("k_cache and v_cache must be [B, Lmax, Hkv, D] of "
                         f"one shape, got {tuple(k_cache.shape)} and "
                         f"{tuple(v_cache.shape)}")
    B, _, Hq, D = q.shape
    if k_cache.shape[0] != B or k_cache.shape[3] != D:
        raise ValueError(f"caches {tuple(k_cache.shape)} do not match q "
                         f"{tuple(q.shape)}")
    if D not in DECODE_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {DECODE_HEAD_DIMS}, got {D}")
    Hkv = k_cache.shape[2]
    if Hkv == 0 or Hq % Hkv != 0:
        raise ValueError(f"Hq ({Hq}) must be a multiple of Hkv ({Hkv})")
    if k_cache.device != q.device or v_cache.device != q.device:
        raise ValueError("q and the caches must be on one device")
    _check_index_arg("kv_lens", kv_lens, q, B)


def _decode_attention_ref(q, k_cache, v_cache, kv_lens):
    """Plain fp32 reference, one batch row at a time (reads the lengths on
    the host)."""
    Lmax = k_cache.shape[1]
    o = torch.zeros_like(q)
    for b, n in enumerate(kv_lens.tolist()):
        n = min(max(n, 0), Lmax)
        if n > 0:
            o[b:b + 1] = _attention_ref(q[b:b + 1], k_cache[b:b + 1, :n],
                                        v_cache[b:b + 1, :n], causal=True)
    return o


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor,
                     kv_lens: torch.Tensor) -> torch.Tensor:
    """Single-token attention over a KV cache. q: [B,1,Hq,D] (rows may be
    strided); k_cache, v_cache: [B,Lmax,Hkv,D], read in place through their
    strides; kv_lens: contiguous int32 [B] on q's device. Row b attends to
    cache rows 0 .. kv_lens[b]-1 (clamped to [0, Lmax]; 0 gives zeros) and
    nothing at or beyond the length is read. Returns o [B,1,Hq,D].
    D in {64, 80, 128}; inference only (no autograd)."""
    _check_decode_args(q, k_cache, v_cache, kv_lens)
    if use_hip(q, k_cache, v_cache, kv_lens):
        o, _ = hip_ext().decode_attn_fwd(q, k_cache, v_cache, kv_lens)
        return o
    return _decode_attention_ref(q, k_cache, v_cache, kv_lens)


def _decode_rope_append_ref(q, k, v, cos, sin, pos, k_cache, v_cache):
    Lmax = k_cache.shape[1]
    ok = (pos >= 0) & (pos < Lmax)
    idx = pos.clamp(0, Lmax - 1).long()
    if cos is not None:
        D = q.shape[-1]
        c = torch.cat([cos[idx], cos[idx]], dim=-1).view(-1, 1, 1, D).float()
        s = torch.cat([sin[idx], sin[idx]], dim=-1).view(-1, 1, 1, D).float()

        def rot(x):
            x1, x2 = x.float().chunk(2, dim=-1)
            return (x.float() * c + torch.cat((-x2, x1), dim=-1) * s
                    ).to(x.dtype)
        q_out, k = rot(q), rot(k)
    else:
        q_out = q.clone()
    q_out = torch.where(ok.view(-1, 1, 1, 1), q_out, torch.zeros_like(q_out))
    rows = ok.nonzero().flatten()
    k_cache[rows, idx[rows]] = k[rows, 0]
    v_cache[rows, idx[rows]] = v[rows, 0]
    return q_out.contiguous()


def decode_rope_append(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                       cos: Optional[torch.Tensor],
                       sin: Optional[torch.Tensor], pos: torch.Tensor,
                       k_cache: torch.Tensor,
                       v_cache: torch.Tensor) -> torch.Tensor:
    """One decode step's RoPE and cache append. q: [B,1,Hq,D]; k, v:
    [B,1,Hkv,D] (rows may be strided views, e.g. into the fused-QKV
    projection output); cos/sin: fp32 [>=Lmax, D/2] tables or None (no
    rotation); pos: contiguous int32 [B] on q's device. Rotates q and k at
    table row pos[b], stores the rotated k and v to cache[b, pos[b]] and
    returns the rotated q (contiguous). A row with pos[b] outside [0, Lmax)
    leaves the cache untouched and returns zeros for q."""
    if q.dim() != 4 or q.shape[1] != 1 or k.shape != v.shape \
            or k.dim() != 4 or k.shape[:2] != q.shape[:2] \
            or k.shape[3] != q.shape[3]:
        raise ValueError("q must be [B,1,Hq,D] and k, v [B,1,Hkv,D], got "
                         f"{tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    B, _, _, D = q.shape
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape \
            or (k_cache.shape[0], k_cache.shape[2], k_cache.shape[3]) \
            != (B, k.shape[2], D):
        raise ValueError(f"caches {tuple(k_cache.shape)} / "
                         f"{tuple(v_cache.shape)} do not match k "
                         f"{tuple(k.shape)}")
    if (cos is None) != (sin is None):
        raise ValueError("give both RoPE tables or neither")
    if cos is not None and (cos.shape[0] < k_cache.shape[1]
                            or cos.shape != sin.shape
                            or cos.shape[1] != D // 2):
        raise ValueError("cos/sin must be [>=Lmax, D/2], got "
                         f"{tuple(cos.shape)} for Lmax={k_cache.shape[1]}")
    _check_index_arg("pos", pos, q, B)
    if use_hip(q, k, v, k_cache, v_cache, pos):
        return hip_ext().decode_rope_append(q, k, v, cos, sin, pos, k_cache,
                                            v_cache)
    return _decode_rope_append_ref(q, k, v, cos, sin, pos, k_cache, v_cache)
