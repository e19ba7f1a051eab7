"""Oracles for the split-KV decode attention and the fused RoPE + cache
append (no GPU needed).

The fp64 reference and every error bound are those of
tests/kernel_oracles.py, unchanged: a batch row of length S is an
``AttnCase(inp, off=S-1, backward=False)`` over the first S cache rows,
judged by ``check_attn_fwd`` (random data) and ``check_attn_counting``
(q = 0, one-hot V: a missing or extra key moves a count by 1, 0.5 is
allowed).  The decode kernel rounds nothing to bf16 before the output, so
it sits well inside the prefill bound ``3 * 2^-8 (P|V|)``.

A decode implementation is a callable ``dec(q, kc, vc, lens, chunk) ->
(o [B,1,Hq,D] bf16, lse [B,Hq,1] fp32)``: the HIP kernel on the GPU,
``torch_decode_attn`` and its mutants on the CPU.

Cache rows at or beyond a row's length are filled on purpose (``stale``):
bf16 NaN on the GPU, so that a single read past the length poisons the
output; ones for the CPU mutants, so that an off-by-one length is a quiet
error that the counting check has to see (an extra all-ones V row moves
every count by about 1 - 1/D).
"""

import math

import torch

from tests import kernel_oracles as ko

INF = float("inf")

HEADS = [(2, 2), (4, 2), (8, 1), (16, 1)]
HEAD_DIMS = [64, 80, 128]

# Where the partial kernel changes path inside a chunk (its header): a key
# belongs to row slot (j - chunk_start) % SLOTS, and a slot takes its keys 4
# at a time, then singly.  SLOTS = 32 at D = 64 and 16 at D = 80 / 128, so
# the edges are SLOTS and 4 * SLOTS, each -1 / +0 / +1.
STRIP_EDGES = {64: (31, 32, 33, 127, 128, 129),
               80: (15, 16, 17, 63, 64, 65),
               128: (15, 16, 17, 63, 64, 65)}


def oracle_lengths(D, c):
    base = [1, 2, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1]
    return sorted(set(base) | set(STRIP_EDGES[D]))


def decode_inputs(lens, Lmax, Hq, Hkv, D, device, seed=0, stale="nan"):
    """Random bf16 q [B,1,Hq,D] and caches [B,Lmax,Hkv,D]; rows at or beyond
    lens[b] hold `stale` ("nan", "ones" or "zeros")."""
    B = len(lens)
    g = ko._gen(seed)
    mk = lambda *s: ko.bf(torch.randn(*s, generator=g))
    q, kc, vc = mk(B, 1, Hq, D), mk(B, Lmax, Hkv, D), mk(B, Lmax, Hkv, D)
    fill = {"nan": float("nan"), "ones": 1.0, "zeros": 0.0}[stale]
    for b, n in enumerate(lens):
        kc[b, max(n, 0):] = fill
        vc[b, max(n, 0):] = fill
    return dict(q=q.to(device), kc=kc.to(device), vc=vc.to(device),
                lens=torch.tensor(lens, dtype=torch.int32, device=device))


def row_case(inp, b, S):
    """The prefill oracle's view of batch row b with S visible keys."""
    return ko.AttnCase(dict(q=inp["q"][b:b + 1], k=inp["kc"][b:b + 1, :S],
                            v=inp["vc"][b:b + 1, :S], do=None),
                       off=S - 1, backward=False)


def check_decode_rows(dec, inp, chunk, cases=None):
    """One call of `dec` over the batch, each row judged by check_attn_fwd.
    Returns ({row label: ratios}, o, lse); `cases` (from `row_cases`) shares
    the fp64 references between calls."""
    o, lse = dec(inp["q"], inp["kc"], inp["vc"], inp["lens"], chunk)
    lens = inp["lens"].tolist()
    if cases is None:
        cases = row_cases(inp)
    res = {}
    for b, S in enumerate(lens):
        got = lambda q, k, v, off, b=b: (o[b:b + 1], lse[b:b + 1])
        res[f"row{b}/len{S}"] = ko.check_attn_fwd(got, cases[b])[0]
    return res, o, lse


def row_cases(inp):
    return [row_case(inp, b, S) for b, S in enumerate(inp["lens"].tolist())]


def check_decode_counting(dec, D, lens, Lmax, chunk, device, Hq=2, Hkv=1,
                          stale="nan"):
    """check_attn_counting per length; the keys sit at the head of a cache of
    Lmax rows whose other rows hold `stale`."""
    fill = {"nan": float("nan"), "ones": 1.0, "zeros": 0.0}[stale]

    def attn(q, k, v, off):
        S = k.shape[1]
        kc = torch.full((1, Lmax) + tuple(k.shape[2:]), fill,
                        dtype=k.dtype, device=k.device)
        vc = kc.clone()
        kc[:, :S], vc[:, :S] = k, v
        n = torch.tensor([S], dtype=torch.int32, device=k.device)
        return dec(q, kc, vc, n, chunk)

    return {f"count/len{S}": ko.check_attn_counting(
        attn, D, 1, S, S - 1, device, Hq=Hq, Hkv=Hkv) for S in lens}


def flatten(res):
    return {f"{k}/{n}": v for k, r in res.items() for n, v in r.items()}


def torch_decode_attn(q, kc, vc, lens, chunk, mut=None):
    """fp32 emulation of the partial / combine scheme: per chunk of `chunk`
    keys an unnormalised (m, l, acc), merged with exp(m_s - m) weights; bf16
    output.  Reads no cache row at or beyond the (possibly mutated) length.
    mut: len_plus1, len_minus1, drop_last_chunk, combine_no_rescale, gqa_mod,
    len_of_row0."""
    B, _, Hq, D = q.shape
    Lmax, Hkv = kc.shape[1], kc.shape[2]
    rep = Hq // Hkv
    idx = torch.arange(Hq, device=q.device)
    idx = idx % Hkv if mut == "gqa_mod" else idx // rep
    sc = 1.0 / math.sqrt(D)
    o = torch.zeros(B, 1, Hq, D, device=q.device)
    lse = torch.full((B, Hq, 1), -INF, device=q.device)
    ns = lens.tolist()
    for b in range(B):
        n = ns[0] if mut == "len_of_row0" else ns[b]
        n += {"len_plus1": 1, "len_minus1": -1}.get(mut, 0)
        n = min(max(n, 0), Lmax)
        if n == 0:
            continue
        qf = q[b, 0].float()                                   # [Hq, D]
        parts = []
        for j0 in range(0, n, chunk):
            kf = kc[b, j0:min(j0 + chunk, n)].float()[:, idx]  # [n_s, Hq, D]
            vf = vc[b, j0:min(j0 + chunk, n)].float()[:, idx]
            s = torch.einsum("hd,jhd->hj", qf, kf) * sc
            m = s.amax(-1, keepdim=True)
            p = torch.exp(s - m)
            parts.append((m, p.sum(-1, keepdim=True),
                          torch.einsum("hj,jhd->hd", p, vf)))
        if mut == "drop_last_chunk" and len(parts) > 1:
            parts = parts[:-1]
        M = torch.stack([p[0] for p in parts]).amax(0)
        l = torch.zeros_like(M)
        acc = torch.zeros(Hq, D, device=q.device)
        for m_s, l_s, a_s in parts:
            w = torch.ones_like(M) if mut == "combine_no_rescale" \
                else torch.exp(m_s - M)
            l = l + l_s * w
            acc = acc + a_s * w
        o[b, 0] = acc / l
        lse[b] = M + torch.log(l)
    return ko.bf(o), lse


# --------------------------------------------------------------------------
# RoPE + cache append
# --------------------------------------------------------------------------
def rope_append_inputs(pos, Lmax, Hq, Hkv, D, device, seed=0, rope=True):
    """q/k/v as views into one fused-QKV row [B, 1, (Hq + 2 Hkv) D], the RoPE
    tables, and caches holding a sentinel pattern."""
    B = len(pos)
    g = ko._gen(seed)
    qkv = ko.bf(torch.randn(B, 1, (Hq + 2 * Hkv) * D, generator=g)).to(device)
    C, KV = Hq * D, Hkv * D
    q = qkv[..., :C].view(B, 1, Hq, D)
    k = qkv[..., C:C + KV].view(B, 1, Hkv, D)
    v = qkv[..., C + KV:].view(B, 1, Hkv, D)
    cos = sin = None
    if rope:
        cos, sin = ko.rope_tables(Lmax, D, generator=g)
        cos, sin = cos.to(device), sin.to(device)
    sentinel = ko.bf(torch.randn(B, Lmax, Hkv, D, generator=g)).to(device)
    return dict(q=q, k=k, v=v, cos=cos, sin=sin,
                pos=torch.tensor(pos, dtype=torch.int32, device=device),
                kc=sentinel.clone(), vc=sentinel.flip(1).clone())


def rope_append_expected(inp, rope_apply):
    """What the step is defined as: rope_apply on the table rows sliced at
    pos[b], then an indexed copy into the cache; rows with pos outside
    [0, Lmax) leave the cache as it was and give q = 0."""
    kc, vc = inp["kc"].clone(), inp["vc"].clone()
    Lmax = kc.shape[1]
    q_out = torch.zeros_like(inp["q"]).contiguous()
    for b, p in enumerate(inp["pos"].tolist()):
        if not 0 <= p < Lmax:
            continue
        qb, kb = inp["q"][b:b + 1].contiguous(), inp["k"][b:b + 1].contiguous()
        if inp["cos"] is not None:
            c, s = inp["cos"][p:p + 1], inp["sin"][p:p + 1]
            qb, kb = rope_apply(qb, c, s), rope_apply(kb, c, s)
        q_out[b] = qb[0]
        kc[b, p] = kb[0, 0]
        vc[b, p] = inp["v"][b, 0]
    return q_out, kc, vc


def torch_rope_append(q, k, v, cos, sin, pos, kc, vc, mut=None):
    """Plain-torch step (writes into kc / vc, returns q).  mut:
    append_pos_plus1 stores k and v one row too far."""
    Lmax = kc.shape[1]
    q_out = torch.zeros_like(q).contiguous()
    for b, p in enumerate(pos.tolist()):
        if not 0 <= p < Lmax:
            continue
        qb, kb = q[b:b + 1], k[b:b + 1]
        if cos is not None:
            qb = ko.torch_rope(qb, cos[p:p + 1], sin[p:p + 1], False)
            kb = ko.torch_rope(kb, cos[p:p + 1], sin[p:p + 1], False)
        q_out[b] = qb[0]
        row = p + 1 if mut == "append_pos_plus1" else p
        if row < Lmax:
            kc[b, row] = kb[0, 0]
            vc[b, row] = v[b, 0]
    return q_out


def check_rope_append(step, inp, rope_apply):
    """step(q, k, v, cos, sin, pos, kc, vc) -> q_out, writing kc / vc in
    place.  Bit-exact against `rope_append_expected`; returns the three
    verdicts."""
    want_q, want_k, want_v = rope_append_expected(inp, rope_apply)
    kc, vc = inp["kc"].clone(), inp["vc"].clone()
    got_q = step(inp["q"], inp["k"], inp["v"], inp["cos"], inp["sin"],
                 inp["pos"], kc, vc)
    return dict(q=torch.equal(got_q, want_q), k_cache=torch.equal(kc, want_k),
                v_cache=torch.equal(vc, want_v))
