"""Token sampling from a row of logits: temperature, top-k, top-p and the
draw, as one op that writes the next id where the decode step reads it.

`sample_logits(logits, u, out_ids, temperature, top_k, top_p)` takes one
uniform number per row from the caller (`torch.rand`, which a hipGraph capture
replays with fresh numbers) and is otherwise a pure function: the same row and
the same u give the same id at every batch position, row stride and run.

Semantics (the torch route below is their reference, in fp32):

1. temperature <= 0: the lowest index among the maxima (greedy).
2. z = logits / temperature, in fp32 from the stored value.
3. top-k (0 < top_k < V): keep z >= kth, kth the k-th largest z; ties at the
   border all stay.
4. top-p (0 < top_p < 1): pr = softmax over the top-k survivors; G(i) = the
   mass of the survivors with z strictly greater than z_i; keep i iff
   G(i) <= top_p. The top token always stays (G = 0) and a class of equal z
   stays or goes whole.
5. w = pr * keep, c = the inclusive prefix sum of w in vocabulary order: the
   smallest i with w_i > 0 and c_i > u * c_last. When rounding leaves no such
   i (u * c_last rounds up to c_last), the last i with w_i > 0.

On the GPU this is csrc/sample_logits.hip: one workgroup per row, radix
selects for the two thresholds instead of a sort, one scan for the draw. The
kernel finds the thresholds on the stored values, whose order a division by
a positive temperature keeps; its sums are fp32 in a fixed order, so it
agrees with this reference up to fp32 rounding of the masses (measured
against fp64 in tests/test_sampling_gpu.py, profiles/sampling.md)."""

from typing import Optional

import torch

from modalities_amd.ops.backend import hip_ext, use_hip


def _check_sample_args(logits, u, out_ids):
    for name, t in (("logits", logits), ("u", u), ("out_ids", out_ids)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"sample_logits: {name} must be a tensor")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"sample_logits: logits must be bf16 or fp32, got "
                        f"{logits.dtype}")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"sample_logits: logits must be a non-empty [B, V], "
                         f"got {tuple(logits.shape)}")
    if logits.stride(1) != 1 and logits.shape[1] > 1:
        raise ValueError("sample_logits: logits must have unit stride in V")
    B = logits.shape[0]
    if u.dtype != torch.float32:
        raise TypeError(f"sample_logits: u must be fp32, got {u.dtype}")
    if tuple(u.shape) != (B,) or not u.is_contiguous():
        raise ValueError(f"sample_logits: u must be contiguous [B] = {(B,)}, "
                         f"got {tuple(u.shape)}")
    if out_ids.dtype != torch.int64:
        raise TypeError(f"sample_logits: out_ids must be int64, got "
                        f"{out_ids.dtype}")
    if tuple(out_ids.shape) not in ((B,), (B, 1)):
        raise ValueError(f"sample_logits: out_ids must be [B] or [B, 1] with "
                         f"B = {B}, got {tuple(out_ids.shape)}")
    if u.device != logits.device or out_ids.device != logits.device:
        raise ValueError(f"sample_logits: logits on {logits.device}, u on "
                         f"{u.device}, out_ids on {out_ids.device}")


def _sample_logits_ref(logits: torch.Tensor, u: torch.Tensor,
                       temperature: float, top_k: int, top_p: float,
                       dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The semantics of the module docstring in plain torch, computed in
    `dtype`; returns int64 [B]."""
    x = logits.to(dtype)
    V = x.shape[1]
    idx = torch.arange(V, device=x.device)
    if temperature <= 0:
        return torch.where(x == x.amax(-1, keepdim=True), idx, V).amin(-1)
    z = x / temperature
    keep = torch.ones_like(z, dtype=torch.bool)
    if 0 < top_k < V:
        keep = z >= torch.topk(z, top_k, dim=-1).values[:, -1:]
    pr = torch.softmax(z.masked_fill(~keep, float("-inf")), dim=-1)
    if 0.0 < top_p < 1.0:
        order = torch.argsort(z, dim=-1, descending=True, stable=True)
        zs, ps = z.gather(-1, order), pr.gather(-1, order)
        before = ps.cumsum(-1) - ps          # mass ahead of a sorted slot
        # a slot's class starts at the first slot of equal z
        start = torch.searchsorted((-zs).contiguous(), (-zs).contiguous())
        g = torch.empty_like(z).scatter_(-1, order, before.gather(-1, start))
        keep = keep & (g <= top_p)
    w = pr * keep
    c = w.cumsum(-1)
    hit = (w > 0) & (c > u.to(dtype)[:, None] * c[:, -1:])
    first = torch.where(hit, idx, V).amin(-1)
    last = torch.where(w > 0, idx, -1).amax(-1)
    return torch.where(first < V, first, last)


def sample_logits(logits: torch.Tensor, u: torch.Tensor,
                  out_ids: torch.Tensor, temperature: float = 1.0,
                  top_k: Optional[int] = None,
                  top_p: Optional[float] = None) -> torch.Tensor:
    """Sample one id per row of `logits` into `out_ids` (module docstring).

    logits: [B, V] bf16 or fp32, unit stride in V, any row stride and
    alignment (a `[:, -1, :]` view of [B, T, V] is read in place). u: fp32
    [B] in [0, 1). out_ids: int64 [B] or [B, 1], written in place and
    returned. top_k None or <= 0, or >= V: no top-k; top_p None or outside
    (0, 1): no top-p; temperature <= 0: greedy. Logits must hold no NaN and
    no +inf. Inference only (no autograd)."""
    _check_sample_args(logits, u, out_ids)
    temperature = float(temperature)
    top_k = 0 if top_k is None else int(top_k)
    top_p = 0.0 if top_p is None else float(top_p)
    if use_hip(logits, u, out_ids):
        hip_ext().sample_logits(logits, u, out_ids, temperature, top_k, top_p)
    else:
        ids = _sample_logits_ref(logits, u, temperature, top_k, top_p)
        out_ids.copy_(ids.view(out_ids.shape))
    return out_ids
