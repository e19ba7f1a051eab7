"""fp64 oracle, checker and fp32 emulations (with deliberate mutants) for the
LayerNorm kernels, in the conventions of tests/kernel_oracles.py: the
reference is computed in fp64 from the same bf16 inputs the kernel receives,
and a checker returns ``{name: error / bound}`` with <= 1 meaning correct.

Bounds (derived from the arithmetic, none fitted to a kernel):

* mean:  fp32 sum rule, ``|got-ref| <= 2^-18 mean_j|x|``.
* rstd:  ``|got-ref| <= 2^-18 ref (1 + ref^2 mean_j(|d| (|x|+|mu|)))``,
  d = x - mu.  The first term is the fp32 sum/rsqrt rule; the second is the
  fp32 rounding of the centred values (each d carries an absolute error of
  2^-24 (|x|+|mu|), which moves the variance by 2 |d| times that, and rstd by
  ref^3 / 2 times the variance error).
* y:  single bf16 rounding of ``(x-m) r w + b`` evaluated in fp64 WITH THE
  mean / rstd THE IMPLEMENTATION RETURNED (the statistics are judged on
  their own); S = (|x|+|m|) r |w| + |b|.
* dx:  single bf16 rounding; the backward is handed the fp64 statistics
  rounded to fp32 (as check_rmsnorm does), so it is checked independently of
  the forward; S = r (|g| + mean_j|g| + xa mean_j(|g| xa)), g = dy w,
  xa = (|x|+|m|) r.
* dw, db:  fp32 sum rule over rows, S = sum|dy| xa and sum|dy|.
"""

import torch

from tests.kernel_oracles import (F32_SLACK, F32_TINY, bf, f32_sum_ratio,
                                  ratio, require, single_rounding_ratio)

__all__ = ["layernorm_inputs", "layernorm_ref64", "check_layernorm",
           "check_layernorm_op", "torch_layernorm_fwd", "torch_layernorm_bwd",
           "require"]


def layernorm_inputs(N, H, device, seed=0):
    """x, w, b, dy in bf16.  Rows of x (those that exist for N): 0 randn,
    1 x1e3, 2 x1e-3, 3 randn, 4 all zero, 5 offset (8 + 0.1 randn),
    6 constant 3.140625."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, generator=g)
    if N >= 3:
        x[1] *= 1e3
        x[2] *= 1e-3
    if N >= 5:
        x[4] = 0.0
    w = torch.randn(H, generator=g) * 0.1 + 1.0
    dy = torch.randn(N, H, generator=g)
    b = torch.randn(H, generator=g) * 0.1
    if N >= 6:
        x[5] = 8.0 + 0.1 * torch.randn(H, generator=g)
    if N >= 7:
        x[6] = 3.140625
    return tuple(bf(t).to(device) for t in (x, w, b, dy))


def layernorm_stats64(x, eps):
    """fp64 mean, rstd and the terms of their bounds, from x [N,H]."""
    xd = x.double()
    mu = xd.mean(-1)
    d = xd - mu[:, None]
    r = torch.rsqrt(d.pow(2).mean(-1) + eps)
    S_mean = xd.abs().mean(-1)
    centred = (d.abs() * (xd.abs() + mu.abs()[:, None])).mean(-1)
    rstd_bound = F32_SLACK * r * (1.0 + r * r * centred)
    return mu, r, S_mean, rstd_bound


def layernorm_ref64(x, w, b, dy, mean, rstd):
    """Everything downstream of the statistics, in fp64, from the given
    mean / rstd [N]: y, dx, dw, db and the sums of |terms| of each."""
    xd, wd = x.double(), w.double()
    m, r = mean.double()[:, None], rstd.double()[:, None]
    bd = torch.zeros_like(wd) if b is None else b.double()
    xhat = (xd - m) * r
    xa = (xd.abs() + m.abs()) * r
    out = dict(y=xhat * wd + bd, S_y=xa * wd.abs() + bd.abs())
    if dy is not None:
        dyd = dy.double()
        g = dyd * wd
        out["dx"] = r * (g - g.mean(-1, keepdim=True)
                         - xhat * (g * xhat).mean(-1, keepdim=True))
        out["S_dx"] = r * (g.abs() + g.abs().mean(-1, keepdim=True)
                           + xa * (g.abs() * xa).mean(-1, keepdim=True))
        out["dw"] = (dyd * xhat).sum(0)
        out["S_dw"] = (dyd.abs() * xa).sum(0)
        out["db"] = dyd.sum(0)
        out["S_db"] = dyd.abs().sum(0)
    return out


def check_layernorm(fwd, bwd, N, H, eps, device, bias=True, seed=0):
    """fwd(x, w, b_or_None, eps) -> (y, mean, rstd);
    bwd(dy, x, w, mean, rstd, has_bias) -> (dx, dw, db_or_anything).
    bwd=None checks the forward only."""
    x, w, b, dy = layernorm_inputs(N, H, device, seed)
    if not bias:
        b = None
    y, mean, rstd = fwd(x, w, b, eps)
    assert y.shape == x.shape and y.dtype == torch.bfloat16
    assert mean.shape == (N,) and mean.dtype == torch.float32
    assert rstd.shape == (N,) and rstd.dtype == torch.float32
    mu, r, S_mean, rstd_bound = layernorm_stats64(x, eps)
    f = layernorm_ref64(x, w, b, None, mean, rstd)
    out = {"mean": f32_sum_ratio(mean, mu, S_mean, floor=F32_TINY),
           "rstd": ratio((rstd.double() - r).abs(), rstd_bound),
           "y": single_rounding_ratio(y, f["y"], f["S_y"])}
    if bwd is not None:
        m32, r32 = mu.float(), r.float()  # the backward is checked on its own
        dx, dw, db = bwd(dy, x, w, m32, r32, bias)
        assert dx.shape == x.shape and dx.dtype == torch.bfloat16
        assert dw.shape == (H,) and dw.dtype == torch.float32
        g = layernorm_ref64(x, w, b, dy, m32, r32)
        out["dx"] = single_rounding_ratio(dx, g["dx"], g["S_dx"])
        out["dw"] = f32_sum_ratio(dw, g["dw"], g["S_dw"], floor=F32_TINY)
        if bias:
            assert db.shape == (H,) and db.dtype == torch.float32
            out["db"] = f32_sum_ratio(db, g["db"], g["S_db"], floor=F32_TINY)
    return out


def check_layernorm_op(op, x, w, b, dy, eps):
    """The autograd op: op(x, w, b_or_None, eps) -> y, x of any shape [..,H]
    and any strides.  The statistics are not visible here, so y and dx are
    held against the fp64 statistics (their fp32 error, <= 2^-22 relative, is
    inside the 2^-18 S term); dw / db come back in bf16: single rounding."""
    H = x.shape[-1]
    xl = x.detach().clone().requires_grad_(True)
    wl = w.detach().clone().requires_grad_(True)
    bl = None if b is None else b.detach().clone().requires_grad_(True)
    y = op(xl, wl, bl, eps)
    assert y.shape == x.shape and y.dtype == x.dtype
    y.backward(dy)
    x2, dy2 = x.reshape(-1, H), dy.reshape(-1, H)
    mu, r, _, _ = layernorm_stats64(x2, eps)
    g = layernorm_ref64(x2, w, b, dy2, mu, r)
    out = {"y": single_rounding_ratio(y.detach().reshape(-1, H), g["y"],
                                      g["S_y"]),
           "dx": single_rounding_ratio(xl.grad.reshape(-1, H), g["dx"],
                                       g["S_dx"]),
           "dw": single_rounding_ratio(wl.grad, g["dw"], g["S_dw"])}
    if b is not None:
        out["db"] = single_rounding_ratio(bl.grad, g["db"], g["S_db"])
    return out


# --------------------------------------------------------------------------
# fp32 torch emulations (the arithmetic a correct kernel does) and mutants
# --------------------------------------------------------------------------
def torch_layernorm_fwd(x, w, b, eps, mut=None):
    xf = x.float()
    H = x.shape[1]
    m = xf.sum(-1) / H
    if mut == "var_one_pass":      # E[x^2] - mean^2
        var = (xf * xf).sum(-1) / H - m * m
    else:
        d = xf - m[:, None]
        var = (d * d).sum(-1) / H
    r = torch.rsqrt(var + eps)
    y = (xf - m[:, None]) * r[:, None] * w.float()
    if b is not None:
        y = y + b.float()
    return bf(y), m, r


def torch_layernorm_bwd(dy, x, w, mean, rstd, has_bias, mut=None):
    xf, wf, dyf = x.float(), w.float(), dy.float()
    H = x.shape[1]
    m, r = mean[:, None], rstd[:, None]
    xhat = (xf - m) * r
    g = dyf * wf
    c1 = g.sum(-1, keepdim=True) / H
    c2 = (g * xhat).sum(-1, keepdim=True) / H
    if mut == "drop_mean_g":
        dx = r * (g - xhat * c2)
    else:
        dx = r * (g - c1 - xhat * c2)
    t = dyf * xhat
    dw = (t[:-1] if mut == "dw_last_row" else t).sum(0)
    db = (dyf[:-1] if mut == "db_last_row" else dyf).sum(0)
    return bf(dx), dw, (db if has_bias else None)
