"""Oracles and checkers for document-masked causal attention (no GPU needed).

The contract: with ``start`` int32 [B, T] (``document_starts``), query i of
batch row b sees exactly the keys ``start[b, i] <= j <= i``.  The backward
kernels take the key-side mirror ``end[b, j]`` (last query of j's document)
for dK/dV, so the emulation below masks dQ from ``start`` and dK/dV from
``end`` -- an off-by-one in either array is a different, detectable error.

Everything is built on tests/kernel_oracles.py: ``ratio``, ``require``,
``_expand``, ``_reduce_rep``, ``bf`` and the bound formulas of its docstring
are reused unchanged; no new tolerance is introduced.  The counting check
allows 0.5 of a key and 1e-4 on ``lse = log n_i`` as ``check_attn_counting``
does.
"""

import math

import torch

from tests import kernel_oracles as ko
from tests.kernel_oracles import (BF16_ULP, F32_SLACK, F32_TINY, INF, _expand,
                                  _reduce_rep, bf, ratio)


# --------------------------------------------------------------------------
# layouts
# --------------------------------------------------------------------------
def layout_start(starts, T, device="cpu"):
    """List of document start positions -> int32 [T] start per position."""
    starts = sorted(set(int(s) for s in starts))
    assert starts and starts[0] == 0 and starts[-1] < T
    out = torch.zeros(T, dtype=torch.int32)
    for s in starts:
        out[s:] = s
    return out.to(device)


def layouts_to_start(layouts, T, device="cpu"):
    """One list of starts per batch row -> int32 [B, T], contiguous."""
    return torch.stack([layout_start(l, T) for l in layouts]).to(
        device).contiguous()


def start_to_end(start):
    """Plain loop: end[b, j] = last i with start[b, i] == start[b, j]."""
    s = start.cpu()
    B, T = s.shape
    end = torch.empty_like(s)
    for b in range(B):
        last = T - 1
        for j in range(T - 1, -1, -1):
            if j < T - 1 and s[b, j + 1] != s[b, j]:
                last = j
            end[b, j] = last
    return end.to(start.device).contiguous()


def python_document_starts(ids, eod):
    """The definition, as a plain loop: start[i] = max({0} U {p + 1 : p < i
    and ids[p] == eod})."""
    out = []
    for row in ids.tolist():
        cur, r = 0, []
        for i, t in enumerate(row):
            r.append(cur)
            if t == eod:
                cur = i + 1
        out.append(r)
    return torch.tensor(out, dtype=torch.int32).reshape(ids.shape)


def start_mask(start):
    """bool [B,1,T,T]: j visible to i iff start[b,i] <= j <= i."""
    T = start.shape[1]
    i = torch.arange(T, device=start.device)
    return ((i[None, None, :] >= start[:, :, None].long())
            & (i[None, None, :] <= i[None, :, None]))[:, None]


def end_mask(end):
    """bool [B,1,T,T]: i sees j iff j <= i <= end[b,j] (the key-side view)."""
    T = end.shape[1]
    i = torch.arange(T, device=end.device)
    return ((i[None, :, None] <= end[:, None, :].long())
            & (i[None, None, :] <= i[None, :, None]))[:, None]


# --------------------------------------------------------------------------
# fp64 reference
# --------------------------------------------------------------------------
def doc_ref64(q, k, v, start, do=None, dlse=None):
    """attn_ref64 with the document mask; same keys."""
    B, T, Hq, D = q.shape
    Hkv = k.shape[2]
    sc = 1.0 / math.sqrt(D)
    qd = q.double().permute(0, 2, 1, 3)
    kd, vd = _expand(k.double(), Hq), _expand(v.double(), Hq)
    mask = start_mask(start)
    s = (qd @ kd.transpose(-1, -2)) * sc
    smax = s.masked_fill(~mask, 0.0).abs().max().item()
    s = s.masked_fill(~mask, -INF)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    r = dict(o=(P @ vd).permute(0, 2, 1, 3), lse=lse, smax=smax,
             absPV=(P @ vd.abs()).permute(0, 2, 1, 3))
    if do is not None:
        dod = do.double().permute(0, 2, 1, 3)
        dP = dod @ vd.transpose(-1, -2)
        delta = (dod * (P @ vd)).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        E = P * (dod.abs() @ vd.abs().transpose(-1, -2)
                 + (dod.abs() * (P @ vd.abs())).sum(-1, keepdim=True))
        if dlse is not None:
            dl = dlse.double()[..., None]
            dS = P * (dP - delta + dl)
            E = E + P * dl.abs()
        r["dq"] = ((dS @ kd) * sc).permute(0, 2, 1, 3)
        r["dk"] = _reduce_rep((dS.transpose(-1, -2) @ qd) * sc, Hkv)
        r["dv"] = _reduce_rep(P.transpose(-1, -2) @ dod, Hkv)
        r["C_dq"] = ((E @ kd.abs()) * sc).max().item()
        r["C_dk"] = _reduce_rep((E.transpose(-1, -2) @ qd.abs()) * sc,
                                Hkv).max().item()
        r["C_dv"] = _reduce_rep(P.transpose(-1, -2) @ dod.abs(),
                                Hkv).max().item()
    return r


# --------------------------------------------------------------------------
# fp32/bf16 emulations and their mutants
# --------------------------------------------------------------------------
FWD_MUTANTS = ("ignore_mask", "start_plus1", "start_minus1",
               "skip_start_tile", "batch0_layout")
BWD_MUTANTS = FWD_MUTANTS + ("end_plus1", "end_minus1")


def _mutate_start(start, mut):
    T = start.shape[1]
    i = torch.arange(T, device=start.device, dtype=start.dtype)[None]
    if mut == "ignore_mask":
        return torch.zeros_like(start)
    if mut == "start_plus1":      # first key of a document dropped
        return start + 1
    if mut == "start_minus1":     # the previous document's eod leaks in
        return (start - 1).clamp(min=0)
    if mut == "batch0_layout":
        return start[:1].expand_as(start).contiguous()
    return start


def _mutated_start_mask(start, mut, tile):
    mask = start_mask(_mutate_start(start, mut))
    if mut == "skip_start_tile":
        # the kv tile holding a document start that is not tile-aligned is
        # skipped for the rows of that document
        T = start.shape[1]
        j = torch.arange(T, device=start.device)
        s = start.long()
        t0 = (s // tile) * tile                                   # [B,T]
        in_tile = ((j[None, None, :] >= t0[:, :, None])
                   & (j[None, None, :] < t0[:, :, None] + tile))
        drop = in_tile & ((s % tile) != 0)[:, :, None]
        mask = mask & ~drop[:, None]
    return mask


def torch_doc_fwd(q, k, v, start, mut=None, tile=64, thr=8.0):
    """torch_attn_fwd (fp32 tiled online softmax with the defer-max rule, P
    rounded to bf16 before PV, bf16 output) under the document mask; a row
    may meet fully masked tiles before its first visible key."""
    B, T, Hq, D = q.shape
    qf = q.float().permute(0, 2, 1, 3)
    kf, vf = _expand(k.float(), Hq), _expand(v.float(), Hq)
    mask = _mutated_start_mask(start, mut, tile)
    s = (qf @ kf.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    m = torch.full((B, Hq, T, 1), -INF, device=q.device)
    l = torch.zeros(B, Hq, T, 1, device=q.device)
    acc = torch.zeros(B, Hq, T, D, device=q.device)
    for j0 in range(0, T, tile):
        mk = mask[..., j0:j0 + tile]
        st = s[..., j0:j0 + tile].masked_fill(~mk, -INF)
        tmax = st.amax(-1, keepdim=True)
        m_new = torch.where(tmax > m + thr, tmax, m)
        m_new = torch.where(torch.isinf(m), tmax, m_new)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m),
                            torch.exp(m - m_new))
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        p = torch.where(mk, torch.exp(st - safe), torch.zeros_like(st))
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + bf(p).float() @ vf[..., j0:j0 + tile, :]
        m = m_new
    o = bf((acc / l).permute(0, 2, 1, 3))
    return o, (m + torch.log(l))[..., 0]


def torch_doc_bwd(do, q, k, v, o, lse, start, end, mut=None, dlse=None,
                  tile=64):
    """torch_attn_bwd under the document mask.  Like the kernels, dQ is
    masked from `start` (a bound per query row) and dK/dV from `end` (a
    bound per key row)."""
    B, T, Hq, D = q.shape
    Hkv = k.shape[2]
    sc = 1.0 / math.sqrt(D)
    qf = q.float().permute(0, 2, 1, 3)
    kf, vf = _expand(k.float(), Hq), _expand(v.float(), Hq)
    dof = do.float().permute(0, 2, 1, 3)
    of = o.float().permute(0, 2, 1, 3)
    mq = _mutated_start_mask(start, mut, tile)
    if mut in FWD_MUTANTS:
        mk_ = mq                    # the same wrong mask on the key side
    else:
        e = end
        if mut == "end_plus1":
            e = (end + 1).clamp(max=T - 1)
        elif mut == "end_minus1":
            e = end - 1
        mk_ = end_mask(e)
    s = (qf @ kf.transpose(-1, -2)) * sc
    P = torch.exp(s - lse.float()[..., None])
    dP = dof @ vf.transpose(-1, -2)
    delta = (dof * of).sum(-1, keepdim=True)
    if dlse is not None:
        delta = delta - dlse.float()[..., None]
    dS = P * (dP - delta)
    zero = torch.zeros_like(P)
    dS_q = bf(torch.where(mq, dS, zero)).float()
    dS_k = bf(torch.where(mk_, dS, zero)).float()
    P_k = bf(torch.where(mk_, P, zero)).float()
    dq = ((dS_q @ kf) * sc).permute(0, 2, 1, 3)
    dk = _reduce_rep((dS_k.transpose(-1, -2) @ qf) * sc, Hkv)
    dv = _reduce_rep(P_k.transpose(-1, -2) @ dof, Hkv)
    return bf(dq), bf(dk), bf(dv)


# --------------------------------------------------------------------------
# case + checkers
# --------------------------------------------------------------------------
class DocCase:
    """Inputs + layout + fp64 reference + fp32/bf16 emulation, computed once
    and left unchanged."""

    def __init__(self, inp, start, backward=True, dlse=None):
        self.q, self.k, self.v, self.do = inp["q"], inp["k"], inp["v"], inp["do"]
        self.start = start.contiguous()
        self.end = start_to_end(start)
        self.dlse = dlse
        self.ref = doc_ref64(self.q, self.k, self.v, self.start,
                             self.do if backward else None, dlse)
        self.emul_err = None
        if backward:
            ref = self.ref
            self.o_in = bf(ref["o"]).contiguous()
            self.lse_in = ref["lse"].float().contiguous()
            e = torch_doc_bwd(self.do, self.q, self.k, self.v, self.o_in,
                              self.lse_in, self.start, self.end, dlse=dlse)
            self.emul_err = {n: (t.double() - ref[n]).abs().max().item()
                             for n, t in zip(("dq", "dk", "dv"), e)}


def check_doc_fwd(attn, case):
    """attn(q, k, v, start) -> (o, lse).  Same ratios as check_attn_fwd.
    Returns (ratios, o, lse)."""
    o, lse = attn(case.q, case.k, case.v, case.start)
    r = case.ref
    res = {"o": ratio((o.double() - r["o"]).abs(),
                      3 * BF16_ULP * r["absPV"] + F32_TINY),
           "lse": ratio((lse.double() - r["lse"]).abs(),
                        1e-4 + 2.0 ** -21 * r["smax"])}
    return res, o, lse


def check_doc_bwd(attn_bwd, case, which=("dq", "dk", "dv")):
    """attn_bwd(do, q, k, v, o, lse, start, end[, dlse]) -> (dq, dk, dv),
    handed the rounded reference o and lse.  Same ratios as check_attn_bwd."""
    extra = () if case.dlse is None else (case.dlse,)
    got = dict(zip(("dq", "dk", "dv"),
                   attn_bwd(case.do, case.q, case.k, case.v, case.o_in,
                            case.lse_in, case.start, case.end, *extra)))
    r, res = case.ref, {}
    for n in which:
        err = (got[n].double() - r[n]).abs().max().item()
        if math.isnan(err):
            err = INF
        e = case.emul_err[n]
        bound = 2 * e + BF16_ULP * r[n].abs().max().item() * 2.0 ** -4 \
            + F32_SLACK * r["C_" + n] + F32_TINY
        res[n] = err / bound
        res["~" + n + "/emul"] = err / e if e > 0 else 0.0
    return res


def check_doc_counting(attn, D, start, device, Hq=2, Hkv=1, seed=0):
    """q = 0, v[j] = e_(j mod D): o[b,i,:,d] * n_i counts the visible keys
    with j mod D == d and lse[b,:,i] = log n_i, n_i = i - start[b,i] + 1.
    One missing/extra key moves a count by 1.0; the check allows 0.5."""
    B, T = start.shape
    g = ko._gen(seed)
    q = torch.zeros(B, T, Hq, D, dtype=torch.bfloat16, device=device)
    k = bf(torch.randn(B, T, Hkv, D, generator=g)).to(device)
    j = torch.arange(T)
    v = torch.zeros(B, T, Hkv, D)
    v[:, j, :, j % D] = 1.0
    v = bf(v).to(device)
    o, lse = attn(q, k, v, start)
    i = torch.arange(T, device=device)
    st = start.long()
    n = (i[None, :] - st + 1).double()                          # [B,T]
    cum = torch.cumsum(v[0, :, 0].double(), 0)                   # [T,D]
    cum0 = torch.cat([torch.zeros(1, D, dtype=torch.float64, device=device),
                      cum], 0)                                   # cum0[t] = sum_{j<t}
    counts = cum0[i + 1][None] - cum0[st]                        # [B,T,D]
    err = (o.double() * n[:, :, None, None] - counts[:, :, None, :]).abs()
    return {"count": ratio(err, 0.5),
            "lse_log_n": ratio((lse.double() - torch.log(n)[:, None, :]).abs(),
                               1e-4)}
