"""Plain-PyTorch oracles and checkers for the HIP kernels (no GPU needed).

Every reference is computed in fp64 from the same bf16/fp32 inputs the
kernel receives.  A checker takes callables with the kernels' signatures
(e.g. ``attn(q, k, v, q_offset) -> (o, lse)``), so the same checker serves
the HIP kernels on the GPU and the pure-torch implementations and their
deliberate mutants on the CPU (tests/test_kernel_oracles_cpu.py).

A checker returns ``{name: ratio}`` with ``ratio = max(error / bound)``; a
correct implementation has every ratio <= 1.  Keys starting with ``~`` are
informational (not asserted).  ``require`` prints and asserts them.

Error bounds are derived from the arithmetic, never tuned:

* single-rounding bf16 outputs (RoPE, SiLU*mul, RMSNorm y/dx, CE dlogits):
  ``|got-ref| <= 2^-8 |ref| + 2^-18 S``; S = sum of |terms| of the final
  expression.  One bf16 ulp (half an ulp of rounding + fp32 evaluation)
  plus 64 fp32 ulps of cancellation slack.
* fp32 reductions (invrms, CE losses/lse, RMSNorm dw, sqsum, AdamW m/v):
  ``|got-ref| <= 2^-18 sum|terms|``.
* fp32 underflow floor: an fp32 intermediate below the smallest normal
  number (2^-126) has lost precision (or was flushed), whatever the
  kernel does; every elementwise bound therefore carries an absolute term
  ``2^-126 * prod(max(1, |factor|))``.  It is ~1e-38 per unit factor and
  cannot hide an error in any value a model would use.
* attention forward: ``|o-ref| <= 3*2^-8 (P|V|)`` elementwise (2^-9 each for
  rounding P to bf16, the row-sum mismatch and output rounding; doubled);
  ``|lse-ref| <= 1e-4 + 2^-21 max|score|``.
* attention backward, per tensor: ``max|got-ref| <= 2 max|emul-ref| +
  2^-12 max|ref| + 2^-18 C``; emul = the torch fp32 computation with P and
  dS rounded to bf16 before the matmuls and bf16 outputs; C = the largest
  sum of |terms| of the fp32 accumulation (the fp32 reduction rule above;
  it only matters where the bf16 terms vanish, e.g. dq at T = 1).  With a
  gradient dlse of the lse output, dS = P (dP - delta + dlse) and the
  |terms| gain P |dlse|; the bound formula is the same.
* fast intrinsics (__expf, __powf, exp2): where a derived bound breaks on
  the GPU, ``require(..., baseline=...)`` allows 2x the error of the same
  operation done by PyTorch in fp32 (measured against the same fp64
  reference in the same normalised units) and prints both numbers.
"""

import math

import torch

BF16_ULP = 2.0 ** -8
F32_SLACK = 2.0 ** -18
F32_TINY = 2.0 ** -126
INF = float("inf")


def bf(x):
    return x.to(torch.bfloat16)


# --------------------------------------------------------------------------
# ratio / require
# --------------------------------------------------------------------------
def ratio(err, bound):
    """max(err / bound); inf for NaN errors or a positive error at bound 0."""
    err = torch.as_tensor(err).double()
    bound = torch.as_tensor(bound).double().to(err.device)
    if err.numel() == 0:
        return 0.0
    err, bound = torch.broadcast_tensors(err, bound)
    r = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    bad = torch.isnan(err) | torch.isnan(bound) | ((err > 0) & (bound <= 0))
    r = torch.where(bad, torch.full_like(r, INF), r)
    return r.max().item()


def single_rounding_ratio(got, ref, S, floor=F32_TINY):
    ref = ref.double()
    bound = BF16_ULP * ref.abs() + F32_SLACK * S.double() + floor
    return ratio((got.double() - ref).abs(), bound)


def f32_sum_ratio(got, ref, S, floor=0.0):
    return ratio((got.double() - ref.double()).abs(),
                 F32_SLACK * S.double() + floor)


def require(label, ratios, baseline=None):
    """Print every figure, then assert ratio <= 1 (or, for the keys present
    in `baseline`, <= max(1, 2 * baseline ratio): the fast-intrinsic rule)."""
    bad = {}
    parts = []
    for k, v in ratios.items():
        txt = f"{k}={v:.3g}"
        if k.startswith("~"):
            parts.append(txt)
            continue
        limit = 1.0
        if baseline is not None and k in baseline:
            limit = max(1.0, 2.0 * baseline[k])
            txt += f"(torch32={baseline[k]:.3g},limit={limit:.3g})"
        parts.append(txt)
        if not v <= limit:
            bad[k] = (v, limit)
    print(f"ORACLE {label}: " + " ".join(parts))
    assert not bad, f"{label}: error/bound above limit: {bad}"
    return ratios


def rejected(ratios):
    return any((not v <= 1.0) for k, v in ratios.items()
               if not k.startswith("~"))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------
def rope_tables(T, D, generator=None):
    """cos/sin [T, D/2] fp32 (the production table formula)."""
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float(), ang.sin().float()


def rope_ref64(x, cos, sin, neg):
    """x [B,T,H,D] bf16 -> (ref fp64, S)."""
    B, T, H, D = x.shape
    h = D // 2
    xd = x.double()
    lo, hi = xd[..., :h], xd[..., h:]
    c = cos[:T].double()[None, :, None, :]
    s = sin[:T].double()[None, :, None, :] * (-1.0 if neg else 1.0)
    ref = torch.cat([lo * c - hi * s, hi * c + lo * s], -1)
    S = torch.cat([(lo * c).abs() + (hi * s).abs(),
                   (hi * c).abs() + (lo * s).abs()], -1)
    return ref, S


def torch_rope(x, cos, sin, neg, mut=None):
    B, T, H, D = x.shape
    h = D // 2
    xf = x.float()
    if mut == "row_plus1":
        c = cos[1:T + 1][None, :, None, :]
        s = sin[1:T + 1][None, :, None, :]
    else:
        c = cos[:T][None, :, None, :]
        s = sin[:T][None, :, None, :]
    if neg:
        s = -s
    if mut == "sin_sign":
        s = -s
    if mut == "adjacent_pairs":
        lo, hi = xf[..., 0::2], xf[..., 1::2]
        out = torch.empty_like(xf)
        out[..., 0::2] = lo * c - hi * s
        out[..., 1::2] = hi * c + lo * s
        return bf(out)
    lo, hi = xf[..., :h], xf[..., h:]
    return bf(torch.cat([lo * c - hi * s, hi * c + lo * s], -1))


def check_rope(rope, B, T, H, D, neg, device, table_len=None, seed=0):
    """rope(x, cos, sin, neg) -> y, all on `device`."""
    g = _gen(seed)
    x = bf(torch.randn(B, T, H, D, generator=g) * 2).to(device)
    cos, sin = rope_tables(table_len or T + 2, D)
    cos, sin = cos.to(device), sin.to(device)
    y = rope(x, cos, sin, neg)
    ref, S = rope_ref64(x, cos, sin, neg)
    assert y.shape == ref.shape and y.dtype == torch.bfloat16
    return {"y": single_rounding_ratio(y, ref, S)}


# --------------------------------------------------------------------------
# SiLU * mul
# --------------------------------------------------------------------------
SILU_SPECIALS = [0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0,
                 100.0, -100.0, 3e4, -3e4]


def silu_inputs(numel, device, seed=0):
    """g, u, dout bf16 [numel]: random values with every pair of special
    values in the first 169 x 3 slots (when numel allows)."""
    g_ = _gen(seed)
    g = torch.randn(numel, generator=g_) * 3
    u = torch.randn(numel, generator=g_) * 2
    d = torch.randn(numel, generator=g_)
    sp = torch.tensor(SILU_SPECIALS)
    n = len(sp)
    pairs_g = sp.repeat_interleave(n)
    pairs_u = sp.repeat(n)
    k = min(numel, n * n)
    g[:k] = pairs_g[:k]
    u[:k] = pairs_u[:k]
    if numel >= 2 * n * n:   # specials in dout too, against special g
        d[n * n:2 * n * n] = pairs_u
        g[n * n:2 * n * n] = pairs_g
    return bf(g).to(device), bf(u).to(device), bf(d).to(device)


def silu_ref64(g, u, d):
    gd, ud, dd = g.double(), u.double(), d.double()
    sig = 1.0 / (1.0 + torch.exp(-gd))
    silu = gd * sig
    out = silu * ud
    dsilu = sig * (1.0 + gd * (1.0 - sig))
    S_dsilu = sig * (1.0 + gd.abs() * (1.0 - sig))
    one = torch.ones_like(gd)
    floor = F32_TINY * torch.maximum(gd.abs(), one) \
        * torch.maximum(ud.abs(), one) * torch.maximum(dd.abs(), one)
    return dict(out=out, dg=dd * ud * dsilu, S_dg=(dd * ud).abs() * S_dsilu,
                du=dd * silu, floor=floor)


def torch_silu_fwd(g, u):
    gf, uf = g.float(), u.float()
    return bf(gf * (1.0 / (1.0 + torch.exp(-gf))) * uf)


def torch_silu_bwd(d, g, u):
    df, gf, uf = d.float(), g.float(), u.float()
    sig = 1.0 / (1.0 + torch.exp(-gf))
    return (bf(df * uf * (sig * (1.0 + gf * (1.0 - sig)))),
            bf(df * (gf * sig)))


def check_silu(fwd, bwd, g, u, d):
    """fwd(g, u) -> out; bwd(d, g, u) -> (dg, du); flat bf16 tensors."""
    r = silu_ref64(g, u, d)
    out = fwd(g, u)
    dg, du = bwd(d, g, u)
    finite = all(torch.isfinite(t.float()).all().item() for t in (out, dg, du))
    return {
        "finite": 0.0 if finite else INF,
        "out": single_rounding_ratio(out, r["out"], r["out"].abs(), r["floor"]),
        "dg": single_rounding_ratio(dg, r["dg"], r["S_dg"], r["floor"]),
        "du": single_rounding_ratio(du, r["du"], r["du"].abs(), r["floor"]),
    }


# --------------------------------------------------------------------------
# RMSNorm
# --------------------------------------------------------------------------
def rmsnorm_inputs(N, H, device, seed=0):
    g = _gen(seed)
    x = torch.randn(N, H, generator=g)
    if N >= 3:
        x[1] *= 1e3
        x[2] *= 1e-3
    if N >= 5:
        x[4] = 0.0
    w = torch.randn(H, generator=g) * 0.1 + 1.0
    dy = torch.randn(N, H, generator=g)
    return bf(x).to(device), bf(w).to(device), bf(dy).to(device)


def rmsnorm_fwd_ref64(x, w, eps):
    xd, wd = x.double(), w.double()
    r = torch.rsqrt(xd.pow(2).mean(-1) + eps)
    return xd * r[:, None] * wd, r


def rmsnorm_bwd_ref64(dy, x, w, invrms):
    """dx, S_dx, dw, S_dw from the fp32 invrms the kernel is handed."""
    xd, wd, dyd = x.double(), w.double(), dy.double()
    r = invrms.double()[:, None]
    H = x.shape[1]
    t = dyd * wd * xd
    k = r ** 3 * t.sum(-1, keepdim=True) / H
    k_abs = r ** 3 * t.abs().sum(-1, keepdim=True) / H
    dx = r * wd * dyd - k * xd
    S_dx = (r * wd * dyd).abs() + k_abs * xd.abs()
    terms = dyd * xd * r
    return dx, S_dx, terms.sum(0), terms.abs().sum(0)


def torch_rmsnorm_fwd(x, w, eps, mut=None):
    xf = x.float()
    H = x.shape[1]
    if mut == "mean_vec8":
        H8 = 8 * (H // 8)
        ms = xf[:, :H8].pow(2).sum(-1) / H8
    else:
        ms = xf.pow(2).sum(-1) / H
    r = torch.rsqrt(ms + eps)
    return bf(xf * r[:, None] * w.float()), r


def torch_rmsnorm_bwd(dy, x, w, invrms, mut=None):
    xf, wf, dyf = x.float(), w.float(), dy.float()
    r = invrms[:, None]
    H = x.shape[1]
    k = r ** 3 * (dyf * wf * xf).sum(-1, keepdim=True) / H
    dx = r * wf * dyf if mut == "drop_kx" else r * wf * dyf - k * xf
    t = dyf * xf * r
    if mut == "dw_last_row":
        t = t[:-1]
    return bf(dx), t.sum(0)


def check_rmsnorm(fwd, bwd, N, H, eps, device, seed=0):
    """fwd(x, w, eps) -> (y, invrms); bwd(dy, x, w, invrms) -> (dx, dw).
    bwd=None checks the forward only (H % 8 != 0)."""
    x, w, dy = rmsnorm_inputs(N, H, device, seed)
    y, invrms = fwd(x, w, eps)
    yref, rref = rmsnorm_fwd_ref64(x, w, eps)
    out = {"y": single_rounding_ratio(y, yref, yref.abs()),
           "invrms": f32_sum_ratio(invrms, rref, rref)}
    if bwd is not None:
        r32 = rref.float()  # the backward is checked independently
        dx, dw = bwd(dy, x, w, r32)
        dxr, S_dx, dwr, S_dw = rmsnorm_bwd_ref64(dy, x, w, r32)
        out["dx"] = single_rounding_ratio(dx, dxr, S_dx)
        out["dw"] = f32_sum_ratio(dw, dwr, S_dw, floor=F32_TINY)
    return out


# --------------------------------------------------------------------------
# Cross entropy
# --------------------------------------------------------------------------
def ce_inputs(N, V, device, kind="random", ignore_index=-100, seed=0):
    """logits bf16 [N,V], targets int64 [N].  Targets cycle through column
    0, V-1 and the scalar tail (first column past the last multiple of 8)."""
    g = _gen(seed)
    logits = torch.randn(N, V, generator=g) * 2
    tail = min(V - 1, 8 * (V // 8))
    cand = [0, V - 1, tail]
    targets = torch.tensor([cand[i % 3] for i in range(N)], dtype=torch.int64)
    if kind == "big":        # +-3e4 logits
        logits = torch.where(torch.rand(N, V, generator=g) < 0.5,
                             torch.tensor(3e4), torch.tensor(-3e4))
        logits[:, ::3] = torch.randn(N, (V + 2) // 3, generator=g)
    elif kind == "neginf":   # -inf in non-target columns
        m = torch.rand(N, V, generator=g) < 0.5
        m[:, 0] = True       # a thread's FIRST element is -inf
        m[torch.arange(N), targets] = False
        logits[m] = -INF
    elif kind == "ignored":
        targets[:] = ignore_index
    elif kind == "mixed" and N >= 2:
        targets[1] = ignore_index
    return bf(logits).to(device), targets.to(device)


def ce_ref64(logits, targets, scale, ignore_index, lse32=None):
    x = logits.double()
    N, V = x.shape
    lse = torch.logsumexp(x, -1)
    m = x.max(-1).values
    S_lse = m.abs() + (lse - m).abs() + 1.0
    ign = targets == ignore_index
    tc = targets.clamp(min=0)
    xt = x.gather(1, tc[:, None])[:, 0]
    losses = torch.where(ign, torch.zeros_like(lse), lse - xt)
    S_loss = torch.where(ign, torch.zeros_like(lse), S_lse + xt.abs())
    # backward from the fp32 lse the kernel is handed
    l = (lse if lse32 is None else lse32.double())[:, None]
    p = torch.exp(x - l)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(N, device=x.device), tc] = 1.0
    onehot[ign] = 0.0
    p = torch.where(ign[:, None], torch.zeros_like(p), p)
    d = scale * (p - onehot)
    S_d = abs(scale) * (p + onehot)
    return dict(lse=lse, S_lse=S_lse, losses=losses, S_loss=S_loss, d=d,
                S_d=S_d, floor=F32_TINY * max(1.0, abs(scale)))


def torch_ce_fwd(logits, targets, ignore_index, mut=None):
    x = logits.float()
    V = x.shape[1]
    if mut == "skip_tail":
        lse = torch.logsumexp(x[:, :8 * (V // 8)], -1)
    else:
        lse = torch.logsumexp(x, -1)
    ign = targets == ignore_index
    xt = x.gather(1, targets.clamp(min=0)[:, None])[:, 0]
    return torch.where(ign, torch.zeros_like(lse), lse - xt), lse


def torch_ce_bwd(logits, targets, lse, scale, ignore_index, mut=None):
    x = logits.float()
    N, V = x.shape
    ign = targets == ignore_index
    p = torch.exp(x - lse[:, None])
    if mut == "zero_softmax":
        p = torch.zeros_like(p)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(N, device=x.device), targets.clamp(min=0)] = 1.0
    if mut != "keep_ignored":
        onehot[ign] = 0.0
        p[ign] = 0.0
    d = scale.float() * (p - onehot)
    if mut == "skip_tail":
        d[:, 8 * (V // 8):] = 0.0
    return bf(d)


def check_ce(fwd, bwd, logits, targets, scale, ignore_index=-100):
    """fwd(logits, targets, ignore) -> (losses, lse);
    bwd(logits, targets, lse, scale_tensor, ignore) -> dlogits."""
    losses, lse = fwd(logits, targets, ignore_index)
    lse32 = ce_ref64(logits, targets, scale, ignore_index)["lse"].float()
    sc = torch.tensor(scale, dtype=torch.float32, device=logits.device)
    d = bwd(logits, targets, lse32, sc, ignore_index)
    scale32 = float(sc.double())
    r = ce_ref64(logits, targets, scale32, ignore_index, lse32)
    return {"lse": f32_sum_ratio(lse, r["lse"], r["S_lse"]),
            "losses": f32_sum_ratio(losses, r["losses"], r["S_loss"]),
            "dlogits": single_rounding_ratio(d, r["d"], r["S_d"], r["floor"])}


# --------------------------------------------------------------------------
# AdamW / sqsum / scale
# --------------------------------------------------------------------------
def f32(x):
    """The value a `double` kernel argument has after its cast to float."""
    return float(torch.tensor(x, dtype=torch.float32).double())


HP = dict(lr=1e-3, eps=1e-8, wd=0.1)


def adamw_inputs(n, device, p_zero=False, seed=0):
    g_ = _gen(seed)
    p = torch.zeros(n) if p_zero else torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_)
    g[:3] = torch.tensor([0.0, 1e-8, 1e4])
    m = torch.randn(n, generator=g_) * 0.01
    v = torch.randn(n, generator=g_).abs() * 1e-3
    mask = torch.tensor([0.0, 1.0, 0.37])[torch.randint(0, 3, (n,), generator=g_)]
    mask[:4] = torch.tensor([0.0, 1.0, 0.37, 1.0])
    return [t.to(device) for t in (p, g, m, v, mask)]


def adamw_ref64(p, g, m, v, mask, t, b1, b2, lr, eps, wd, gscale=None,
                bc=None):
    """fp64 AdamW from fp32 state and float-rounded hyper-parameters (the
    kernels take them as float).  bc = (bc1, bc2) for the host-side form."""
    lr, b1, b2, eps, wd = (f32(a) for a in (lr, b1, b2, eps, wd))
    gs = 1.0 if gscale is None else float(gscale)
    bc1, bc2 = (1 - b1 ** t, 1 - b2 ** t) if bc is None else \
        (f32(bc[0]), f32(bc[1]))
    pd, gd, md, vd, wdm = (a.double() for a in (p, g, m, v, mask))
    gj = gd * gs
    p1 = pd * (1 - lr * wd * wdm)
    m1 = b1 * md + (1 - b1) * gj
    v1 = b2 * vd + (1 - b2) * gj * gj
    upd = (lr / bc1) * m1 / (torch.sqrt(v1 / bc2) + eps)
    # |update| with the |terms| of m: where b1*m and (1-b1)*g cancel, the
    # update's error is relative to the terms, not to their small sum
    S_m = (b1 * md).abs() + ((1 - b1) * gj).abs()
    S_upd = (lr / bc1) * S_m / (torch.sqrt(v1 / bc2) + eps)
    return dict(p=p1 - upd, m=m1, v=v1, upd=upd, S_m=S_m, S_v=v1.abs(),
                S_upd=S_upd, S_p=p1.abs() + S_upd,
                cond=(b2 ** t) / (1 - b2 ** t))


def bf16_rne(x):
    return x.to(torch.bfloat16)


def torch_adamw_step(p, g, m, v, mask, t, b1, b2, lr, eps, wd, gscale=None,
                     bc=None, mut=None):
    """fp32 AdamW in place; returns the bf16 copy of p.  bc=None computes
    the bias corrections from t in fp32 (the device-step form)."""
    T = lambda a: torch.tensor(a, dtype=torch.float32, device=p.device)
    lr_, b1_, b2_, eps_, wd_ = T(lr), T(b1), T(b2), T(eps), T(wd)
    tt = 1 if mut == "bc2_frozen" else t
    if bc is None:
        bc1 = 1 - torch.pow(b1_, T(float(t)))
        bc2 = 1 - torch.pow(b2_, T(float(tt)))
    else:
        bc1, bc2 = T(bc[0]), T(bc[1])
    gj = g if gscale is None else g * gscale.float()
    if mut != "decay_after":
        p.mul_(1 - lr_ * wd_ * mask)
    m.mul_(b1_).add_((1 - b1_) * gj)
    if mut != "v_frozen":
        v.mul_(b2_).add_((1 - b2_) * gj * gj)
    p.sub_((lr_ / bc1) * m / (torch.sqrt(v * (1.0 / bc2)) + eps_))
    if mut == "decay_after":
        p.mul_(1 - lr_ * wd_ * mask)
    if mut == "bf16_trunc":
        return (p.view(torch.int32) & -65536).view(torch.float32).to(
            torch.bfloat16)
    return bf16_rne(p)


def check_adamw(step, n, t, betas, device, gscale=None, p_zero=False,
                host_bc=False, has_bf16=True, unit_mask=False, seed=0):
    """step(p, g, m, v, mask, t, gscale_tensor_or_None, hp) updates in place
    and returns the bf16 copy (or None).  hp = dict(lr, b1, b2, eps, wd
    [, bc1, bc2])."""
    b1, b2 = betas
    hp = dict(HP, b1=b1, b2=b2)
    if p_zero:
        hp["wd"] = 0.0
    p, g, m, v, mask = adamw_inputs(n, device, p_zero, seed)
    if unit_mask:
        mask = torch.ones_like(mask)
    bc = None
    if host_bc:
        bc = (1.0 - b1 ** t, 1.0 - b2 ** t)
        hp.update(bc1=bc[0], bc2=bc[1])
    gs_t = None if gscale is None else torch.tensor(
        gscale, dtype=torch.float32, device=device)
    r = adamw_ref64(p, g, m, v, mask, t, b1, b2, hp["lr"], hp["eps"],
                    hp["wd"], None if gs_t is None else gs_t.double().item(),
                    bc)
    out16 = step(p, g, m, v, mask, t, gs_t, hp)
    res = {"m": f32_sum_ratio(m, r["m"], r["S_m"], F32_TINY),
           "v": f32_sum_ratio(v, r["v"], r["S_v"], F32_TINY)}
    if p_zero:
        rel = 2.0 ** -16 + 2.0 ** -21 * r["cond"]
        res["upd"] = ratio((p.double() - r["p"]).abs(),
                           rel * r["S_upd"] + F32_TINY)
    else:
        res["p"] = ratio((p.double() - r["p"]).abs(),
                         2.0 ** -20 * r["S_p"] + F32_TINY)
    if has_bf16:
        same = torch.equal(out16.view(torch.int16),
                           p.to(torch.bfloat16).view(torch.int16))
        res["bf16_bits"] = 0.0 if same else INF
    return res


def check_sqsum(sqsum, sizes, device, seed=0):
    g = _gen(seed)
    ts = [torch.randn(s, generator=g) for s in sizes]
    for t in ts:   # the large values sit at both ends: a skipped head or
        t[0], t[-1] = 1e4, -1e4   # tail (grid-stride remainder) is visible
    ts = [t.to(device) for t in ts]
    ref = sum(t.double().pow(2).sum() for t in ts)
    got = sqsum(ts)
    return {"sqsum": f32_sum_ratio(got, ref, ref)}


def check_scale(scale_, sizes, s, device, seed=0):
    """scale_(tensors, s) in place; an fp32 multiply is exactly the rounded
    fp64 product, so the result must be bit-identical."""
    g = _gen(seed)
    ts = [torch.randn(n, generator=g) for n in sizes]
    ts[0][:2] = torch.tensor([1e4, -1e4])
    ts = [t.to(device) for t in ts]
    refs = [(t.double() * s.double().to(device)).float() for t in ts]
    scale_(ts, s)
    ok = all(torch.equal(t, r) for t, r in zip(ts, refs))
    return {"scale_exact": 0.0 if ok else INF}


# --------------------------------------------------------------------------
# Attention
# --------------------------------------------------------------------------
def _expand(x, Hq, head_map="div"):
    """[B,T,Hkv,D] -> [B,Hq,T,D] through the GQA head map."""
    Hkv = x.shape[2]
    idx = torch.arange(Hq, device=x.device)
    idx = idx // (Hq // Hkv) if head_map == "div" else idx % Hkv
    return x.permute(0, 2, 1, 3)[:, idx]


def causal_mask(Tq, Tkv, off, device, shift=0):
    i = torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tkv, device=device)[None, :]
    m = j <= i + off + shift
    m[:, 0] = True  # never an empty row (only matters for the -1 mutant)
    return m


def _reduce_rep(x, Hkv):
    """[B,Hq,T,D] -> [B,T,Hkv,D] summing each GQA group."""
    B, Hq, T, D = x.shape
    return x.reshape(B, Hkv, Hq // Hkv, T, D).sum(2).permute(0, 2, 1, 3)


def attn_ref64(q, k, v, off, do=None, dlse=None):
    """dlse: optional fp32 [B,Hq,Tq] gradient of lse (d lse / d score = P)."""
    B, Tq, Hq, D = q.shape
    Tkv, Hkv = k.shape[1], k.shape[2]
    sc = 1.0 / math.sqrt(D)
    qd = q.double().permute(0, 2, 1, 3)
    kd, vd = _expand(k.double(), Hq), _expand(v.double(), Hq)
    mask = causal_mask(Tq, Tkv, off, q.device)
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


def torch_attn_fwd(q, k, v, off, mut=None, tile=64, thr=8.0):
    """fp32 tiled online-softmax attention with the kernels' defer-max rule
    (the running max only moves when a tile exceeds it by more than thr),
    P rounded to bf16 before PV, bf16 output.  `mut` selects a mutant."""
    B, Tq, Hq, D = q.shape
    Tkv, Hkv = k.shape[1], k.shape[2]
    if mut == "ignore_offset":
        off = 0
    shift = {"mask_plus1": 1, "mask_minus1": -1}.get(mut, 0)
    hm = "mod" if mut == "gqa_mod" else "div"
    qf = q.float().permute(0, 2, 1, 3)
    kf, vf = _expand(k.float(), Hq, hm), _expand(v.float(), Hq, hm)
    mask = causal_mask(Tq, Tkv, off, q.device, shift)
    if mut == "drop_last_key" and Tkv > 1:
        mask[:, Tkv - 1] = False
    if mut == "drop_tile":
        t0 = ((Tkv // tile) // 2) * tile
        if t0 > 0:
            mask[:, t0:t0 + tile] = False
    s = (qf @ kf.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    m = torch.full((B, Hq, Tq, 1), -INF, device=q.device)
    l = torch.zeros(B, Hq, Tq, 1, device=q.device)
    acc = torch.zeros(B, Hq, Tq, D, device=q.device)
    for j0 in range(0, Tkv, tile):
        mk = mask[:, j0:j0 + tile]
        st = s[..., j0:j0 + tile].masked_fill(~mk, -INF)
        tmax = st.amax(-1, keepdim=True)
        if mut == "skip_rescale":
            m_new = torch.where(torch.isinf(m), tmax, m)   # stale max
        else:
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
    lse = (torch.log(l) if mut == "lse_no_max" else m + torch.log(l))[..., 0]
    return o, lse


def torch_attn_bwd(do, q, k, v, o, lse, off, mut=None, dlse=None):
    """The fp32 emulation: P, dS rounded to bf16 before the matmuls, bf16
    outputs.  Serves as `emul` in the backward bound and as the correct
    CPU implementation; mut = mask_plus1 / mask_minus1 / drop_dlse (the
    gradient of the lse output ignored)."""
    B, Tq, Hq, D = q.shape
    Tkv, Hkv = k.shape[1], k.shape[2]
    sc = 1.0 / math.sqrt(D)
    shift = {"mask_plus1": 1, "mask_minus1": -1}.get(mut, 0)
    qf = q.float().permute(0, 2, 1, 3)
    kf, vf = _expand(k.float(), Hq), _expand(v.float(), Hq)
    dof = do.float().permute(0, 2, 1, 3)
    of = o.float().permute(0, 2, 1, 3)
    mask = causal_mask(Tq, Tkv, off, q.device, shift)
    s = ((qf @ kf.transpose(-1, -2)) * sc).masked_fill(~mask, -INF)
    P = torch.exp(s - lse.float()[..., None])
    dP = dof @ vf.transpose(-1, -2)
    delta = (dof * of).sum(-1, keepdim=True)
    if dlse is not None and mut != "drop_dlse":
        delta = delta - dlse.float()[..., None]
    dS = bf(P * (dP - delta)).float()
    dq = ((dS @ kf) * sc).permute(0, 2, 1, 3)
    dk = _reduce_rep((dS.transpose(-1, -2) @ qf) * sc, Hkv)
    dv = _reduce_rep(bf(P).float().transpose(-1, -2) @ dof, Hkv)
    return bf(dq), bf(dk), bf(dv)


def attn_random_inputs(B, Tq, Tkv, Hq, Hkv, D, device, seed=0):
    g = _gen(seed)
    mk = lambda *s: bf(torch.randn(*s, generator=g)).to(device)
    return dict(q=mk(B, Tq, Hq, D), k=mk(B, Tkv, Hkv, D),
                v=mk(B, Tkv, Hkv, D), do=mk(B, Tq, Hq, D))


def attn_ramp_inputs(Tq, Tkv, D, step, device, B=1, Hq=2, Hkv=1, seed=0):
    """Score ramp: q.k = a*j exactly, so score(i, j) is linear in j with
    slope ~ step.  All values are bf16-exact."""
    g = _gen(seed)
    a = bf(torch.tensor(step * math.sqrt(D))).float()
    j = torch.arange(Tkv)
    k = torch.zeros(B, Tkv, Hkv, D)
    k[..., 0] = (j % 256).float()[None, :, None]
    k[..., 1] = (j // 256).float()[None, :, None]
    q = torch.zeros(B, Tq, Hq, D)
    q[..., 0] = a
    q[..., 1] = 256.0 * a
    v = torch.randn(B, Tkv, Hkv, D, generator=g)
    do = torch.randn(B, Tq, Hq, D, generator=g)
    return dict(q=bf(q).to(device), k=bf(k).to(device), v=bf(v).to(device),
                do=bf(do).to(device), slope=a.double().item() / math.sqrt(D))


class AttnCase:
    """Inputs + fp64 reference + fp32/bf16 emulation, computed once."""

    def __init__(self, inp, off, backward=True, dlse=None):
        self.q, self.k, self.v, self.do = inp["q"], inp["k"], inp["v"], inp["do"]
        self.off = off
        self.dlse = dlse
        self.slope = inp.get("slope")
        self.ref = attn_ref64(self.q, self.k, self.v, off,
                              self.do if backward else None, dlse)
        self.emul_err = None
        if backward:
            ref = self.ref
            self.o_in = bf(ref["o"]).contiguous()
            self.lse_in = ref["lse"].float().contiguous()
            e = torch_attn_bwd(self.do, self.q, self.k, self.v, self.o_in,
                               self.lse_in, off, dlse=dlse)
            self.emul_err = {n: (t.double() - ref[n]).abs().max().item()
                             for n, t in zip(("dq", "dk", "dv"), e)}


def check_attn_fwd(attn, case):
    """attn(q, k, v, off) -> (o, lse).  Returns (ratios, o, lse)."""
    o, lse = attn(case.q, case.k, case.v, case.off)
    r = case.ref
    res = {"o": ratio((o.double() - r["o"]).abs(),
                      3 * BF16_ULP * r["absPV"] + F32_TINY),
           "lse": ratio((lse.double() - r["lse"]).abs(),
                        1e-4 + 2.0 ** -21 * r["smax"])}
    return res, o, lse


def check_attn_bwd(attn_bwd, case, o=None, lse=None,
                   which=("dq", "dk", "dv")):
    """attn_bwd(do, q, k, v, o, lse, off) -> (dq, dk, dv).  By default the
    backward is handed the rounded reference o and lse -- the very inputs
    the emulation got, so that the error which rounding o induces through
    delta = rowsum(dO*O) is common to both and the 2x-emulation bound
    compares like with like (at Tq = 1 that error is a single random draw,
    and two independent draws differ by more than 2x now and then).  It also
    makes the backward check independent of the forward kernel.  A case
    with dlse calls attn_bwd(do, q, k, v, o, lse, off, dlse)."""
    if o is None:
        o, lse = case.o_in, case.lse_in
    extra = () if case.dlse is None else (case.dlse,)
    got = dict(zip(("dq", "dk", "dv"),
                   attn_bwd(case.do, case.q, case.k, case.v, o, lse, case.off,
                            *extra)))
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


def check_ramp_step8(case, o, lse):
    """With slope 8 the last visible key holds all but e^-8 of the weight:
    o[i] = v[min(i+off, Tkv-1)], lse[i] = slope*j + log sum_n e^(-slope n)."""
    B, Tq, Hq, D = case.q.shape
    Tkv = case.k.shape[1]
    dev = case.q.device
    jl = torch.clamp(torch.arange(Tq, device=dev) + case.off, max=Tkv - 1)
    vexp = _expand(case.v.double(), Hq).permute(0, 2, 1, 3)[:, jl]
    vmax = case.v.double().abs().max().item()
    tol = 2 * math.exp(-8.0) * vmax + BF16_ULP * vmax
    sl = case.slope
    n = torch.arange(Tkv, device=dev).double()
    geo = torch.cumsum(torch.exp(-sl * n), 0)      # sum_{n<=j} e^(-sl n)
    lse_ref = (sl * jl.double() + torch.log(geo[jl]))[None, None, :]
    return {"o_is_v_last": ratio((o.double() - vexp).abs(), tol),
            "lse_closed_form": ratio((lse.double() - lse_ref).abs(),
                                     1e-4 + 2.0 ** -21 * sl * (Tkv - 1))}


def check_attn_counting(attn, D, Tq, Tkv, off, device, B=1, Hq=2, Hkv=1,
                        seed=0):
    """q = 0, v[j] = e_(j mod D): o[i,d]*n_i counts the visible keys with
    j mod D == d and lse[i] = log n_i.  One missing/extra key moves a count
    by 1.0; the check allows 0.5."""
    g = _gen(seed)
    q = torch.zeros(B, Tq, Hq, D, dtype=torch.bfloat16, device=device)
    k = bf(torch.randn(B, Tkv, Hkv, D, generator=g)).to(device)
    j = torch.arange(Tkv)
    v = torch.zeros(B, Tkv, Hkv, D)
    v[:, j, :, j % D] = 1.0
    v = bf(v).to(device)
    o, lse = attn(q, k, v, off)
    jl = torch.clamp(torch.arange(Tq, device=device) + off, max=Tkv - 1)
    n = (jl + 1).double()
    counts = torch.cumsum(v[0, :, 0].double(), 0)[jl]          # [Tq, D]
    err = (o.double() * n[None, :, None, None]
           - counts[None, :, None, :]).abs()
    return {"count": ratio(err, 0.5),
            "lse_log_n": ratio((lse.double() - torch.log(n)[None, None]).abs(),
                               1e-4)}
