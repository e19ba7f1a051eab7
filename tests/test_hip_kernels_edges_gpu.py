"""GPU tests: every HIP kernel against the fp64 oracles of
tests/kernel_oracles.py, at the shapes, types and edges where kernels go
wrong.  tests/test_kernel_oracles_cpu.py proves on the CPU that these
checkers reject subtly wrong implementations.

Worst measured error / bound on an MI355X (every check asserts <= 1; the
bounds are derived in tests/kernel_oracles.py, none is fitted to a kernel).
v1 and v2 give the same figures at D = 64 / 128 (same fragment maps).

  kernel / case family               worst error / bound
  ---------------------------------  ------------------------------------------
  attention fwd, random square T     o 0.52   lse 0.008
  attention fwd, offset / decode     o 0.24   lse 0.008
  attention fwd, GQA x batch         o 0.55   lse 0.008
  attention fwd, ramp step 8         o 0.33   lse 0.22  o==v[last] 0.11
                                     lse closed form 0.22
  attention fwd, ramp step 1         o 0.48   lse 0.15
  attention fwd, counting V          count 0.25 (of 0.5 key)  lse-log n 0.011
  attention fwd, V view / cache      o 0.44   lse 0.007
  attention bwd, random square T     dq 0.72  dk 0.81  dv 0.48
  attention bwd, offset / decode     dq 0.70  dk 0.70  dv 0.49
  attention bwd, GQA x batch         dq 0.78  dk 0.62  dv 0.48
  attention bwd, ramp step 8 (dv)    dv 0.48
  attention bwd, ramp step 1         dq 0.64  dk 0.66  dv 0.49
  attention bwd, V view / cache      dq 0.70  dk 0.58  dv 0.48
  attn_bwd_qkvjoint (D 64/80/128)    dq 0.48  dk 0.47  dv 0.48, sentinel intact
  fused_qkv_rope_attention (64/80)   o 0.46   dq 0.25  dk 0.20  dv 0.48
  rope_fwd / _fwd_slice / _bwd_slice y 0.99 (half a bf16 ulp is the bound)
  silu_mul, silu_mul_joint           out 0.99  dg 0.99  du 0.99, all finite
  rmsnorm                            y 0.99  invrms 0.036  dx 0.99  dw 0.041
  cross_entropy                      lse 0.014  losses 0.015  dlogits 0.99
  fused_adamw_masked_devstep         m 0.039  v 0.057  p 0.28  update 0.024
                                     bf16 copy bit-identical
  fused_adamw_masked / fused_adamw   m 0.030  v 0.042  p 0.25
  multi_tensor_sqsum / _scale        sqsum 0.11 (over runs); scale bit-exact

  backward kernel / emulation error ratio (max|kernel-ref| / max|emul-ref|):
  dv 1.0 everywhere; dq, dk 1.0 at D = 64, up to 1.8 (dk, D = 128, random
  square) and 1.7 (dq, D = 80, GQA); the bound allows 2.

  The 2x-of-PyTorch-fp32 rule for fast intrinsics replaces NO derived bound:
  __expf (SiLU, cross entropy) and exp2 (attention) stay inside the derived
  bounds.  __powf did not: with 1 - __powf(beta, t) the devstep kernel
  missed the p bound at beta2 = 0.999, t = 2 (error / bound 3.6; PyTorch
  fp32 pow: 3.7 -- the loss is in holding beta^t in fp32, not in the fast
  pow), and its update error at p0 = 0 was 0.013 of the bound.  The kernel
  now computes -expm1f(t * logf(beta)): p 0.23, update 0.0012 at that point.
"""

import functools
import math

import pytest
import torch

from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32

# (kernel generation, head_dim): v2 for all three head dims, v1 for 64/128
IMPLS = [(2, 64), (2, 80), (2, 128), (1, 64), (1, 128)]
IMPL_IDS = [f"v{i}-D{d}" for i, d in IMPLS]


def _fwd(impl):
    f = EXT.attn_fwd_v1 if impl == 1 else EXT.attn_fwd_v2
    return lambda q, k, v, off: tuple(f(q, k, v, True, off))


def _bwd(impl):
    f = EXT.attn_bwd_v1 if impl == 1 else EXT.attn_bwd_v2
    return lambda do, q, k, v, o, lse, off: tuple(
        f(do, q, k, v, o, lse, True, off))


@functools.lru_cache(maxsize=None)
def _case(kind, D, Tq, Tkv, off, B=1, Hq=2, Hkv=1):
    """Inputs + fp64 reference + emulation, shared by v1 and v2."""
    if kind == "random":
        inp = ko.attn_random_inputs(B, Tq, Tkv, Hq, Hkv, D, DEV,
                                    seed=Tq * 7 + Tkv)
    else:
        inp = ko.attn_ramp_inputs(Tq, Tkv, D, {"ramp8": 8, "ramp1": 1}[kind],
                                  DEV, B, Hq, Hkv, seed=Tq)
    return ko.AttnCase(inp, off)


def _fwd_bwd(label, impl, case, which=("dq", "dk", "dv")):
    r, o, lse = ko.check_attn_fwd(_fwd(impl), case)
    ko.require(label + "/fwd", r)
    ko.require(label + "/bwd", ko.check_attn_bwd(_bwd(impl), case,
                                                 which=which))
    return o, lse


# ------------------------------------------------------------- attention
@pytest.mark.parametrize("T", [1, 31, 33, 63, 65, 127, 129, 255, 257])
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_random_square(impl, D, T):
    _fwd_bwd(f"attn_random/v{impl}/D{D}/T{T}", impl,
             _case("random", D, T, T, 0))


OFFSET_SHAPES = [(1, 1, 0), (1, 130, 129), (1, 257, 256), (5, 200, 195),
                 (32, 96, 64), (100, 300, 100), (128, 512, 384),
                 (128, 128, 128),   # ring context-parallel, fully unmasked
                 (40, 100, 100)]    # every row sees all keys


@pytest.mark.parametrize("Tq,Tkv,off", OFFSET_SHAPES)
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_offset_and_decode(impl, D, Tq, Tkv, off):
    _fwd_bwd(f"attn_offset/v{impl}/D{D}/{Tq}x{Tkv}+{off}", impl,
             _case("random", D, Tq, Tkv, off))


RAMP_SHAPES = [(300, 300, 0), (128, 512, 384), (1, 200, 199), (257, 257, 0)]


@pytest.mark.parametrize("Tq,Tkv,off", RAMP_SHAPES)
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_score_ramp_step8(impl, D, Tq, Tkv, off):
    """Slope 8: the rescale branch runs on every tile, o[i] is the last
    visible v row, lse has a closed form; a mask off by one key moves o by
    O(1) at any offset.  Forward plus dv."""
    case = _case("ramp8", D, Tq, Tkv, off)
    label = f"attn_ramp8/v{impl}/D{D}/{Tq}x{Tkv}+{off}"
    o, lse = _fwd_bwd(label, impl, case, which=("dv",))
    ko.require(label + "/closed", ko.check_ramp_step8(case, o, lse))


@pytest.mark.parametrize("Tq,Tkv,off", RAMP_SHAPES)
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_score_ramp_step1(impl, D, Tq, Tkv, off):
    """Slope 1: P is geometric near the diagonal, so dq, dk and dv all see
    the masks of the dq and dK/dV kernels."""
    _fwd_bwd(f"attn_ramp1/v{impl}/D{D}/{Tq}x{Tkv}+{off}", impl,
             _case("ramp1", D, Tq, Tkv, off))


@pytest.mark.parametrize("Tq,Tkv,off", [(2048, 2048, 0), (128, 512, 384)])
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_counting_v(impl, D, Tq, Tkv, off):
    """Uniform attention over a one-hot V counts the visible keys: dropped
    tail tiles, a wrong n_tiles and tile-edge errors move a count by 1."""
    ko.require(f"attn_count/v{impl}/D{D}/{Tq}x{Tkv}+{off}",
               ko.check_attn_counting(_fwd(impl), D, Tq, Tkv, off, DEV))


@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (4, 2), (8, 1), (6, 3)])
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_gqa_and_batch(impl, D, Hq, Hkv):
    """Distinct random data per batch and head: a wrong stride or head map
    cannot cancel."""
    _fwd_bwd(f"attn_gqa/v{impl}/D{D}/Hq{Hq}Hkv{Hkv}", impl,
             _case("random", D, 130, 130, 0, 3, Hq, Hkv))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("D", [64, 80, 128])
def test_attn_v_view_into_joint_buffer(D, B):
    """V read in place from a joint [B, T, Cq+2Ckv] activation (v2)."""
    T, Hq, Hkv = 130, 2, 1
    Cq, Ckv = Hq * D, Hkv * D
    case = _case("random", D, T, T, 0, B, Hq, Hkv)
    joint = torch.full((B, T, Cq + 2 * Ckv), 3.0, dtype=BF16, device=DEV)
    joint[..., Cq + Ckv:] = case.v.reshape(B, T, Ckv)
    v_view = joint[..., Cq + Ckv:].view(B, T, Hkv, D)
    assert not v_view.is_contiguous() and torch.equal(v_view, case.v)
    fwd = lambda q, k, v, off: _fwd(2)(q, k, v_view, off)
    bwd = lambda do, q, k, v, o, lse, off: _bwd(2)(do, q, k, v_view, o, lse,
                                                   off)
    label = f"attn_vjoint/D{D}/B{B}"
    r, o, lse = ko.check_attn_fwd(fwd, case)
    ko.require(label + "/fwd", r)
    ko.require(label + "/bwd", ko.check_attn_bwd(bwd, case))


@pytest.mark.parametrize("D", [64, 80, 128])
def test_attn_v_slice_of_longer_cache(D):
    """B == 1: K and V as dim-1 slices of a longer cache buffer (the
    zero-copy decode path)."""
    for Tq, Tkv, off in [(1, 130, 129), (5, 200, 195)]:
        case = _case("random", D, Tq, Tkv, off)
        cache_k = torch.full((1, Tkv + 56, 1, D), 5.0, dtype=BF16, device=DEV)
        cache_v = torch.full((1, Tkv + 56, 1, D), 5.0, dtype=BF16, device=DEV)
        cache_k[:, :Tkv] = case.k
        cache_v[:, :Tkv] = case.v
        ks, vs = cache_k[:, :Tkv], cache_v[:, :Tkv]
        fwd = lambda q, k, v, off_: _fwd(2)(q, ks, vs, off_)
        bwd = lambda do, q, k, v, o, lse, off_: _bwd(2)(do, q, ks, vs, o, lse,
                                                        off_)
        label = f"attn_cache/D{D}/{Tq}x{Tkv}+{off}"
        r, o, lse = ko.check_attn_fwd(fwd, case)
        ko.require(label + "/fwd", r)
        ko.require(label + "/bwd", ko.check_attn_bwd(bwd, case))


@pytest.mark.parametrize("D", [64, 80, 128])
def test_attn_bwd_qkvjoint_writes_only_the_dv_block(D):
    """dV goes straight into its column block of a sentinel-filled joint
    gradient buffer: the block must match fp64 and EVERY other element must
    still hold the sentinel (a D=80 store spilling past column 80 of a
    head, a wrong dv_col_off or pitch)."""
    assert EXT.get_attn_impl() == 2
    B, T, Hq, Hkv = 2, 130, 4, 2
    Cq, Ckv = Hq * D, Hkv * D
    Ctot = Cq + 2 * Ckv + 16          # 16 spare columns after the dv block
    case = _case("random", D, T, T, 0, B, Hq, Hkv)
    joint = torch.zeros(B, T, Cq + 2 * Ckv, dtype=BF16, device=DEV)
    joint[..., Cq + Ckv:] = case.v.reshape(B, T, Ckv)
    v_view = joint[..., Cq + Ckv:].view(B, T, Hkv, D)
    SENT = 7.0
    dqkv = torch.full((B, T, Ctot), SENT, dtype=BF16, device=DEV)
    col = Cq + Ckv

    def bwd(do, q, k, v, o_, lse_, off):
        dq, dk = EXT.attn_bwd_qkvjoint(do, q, k, v_view, o_, lse_, True, off,
                                       dqkv, col)
        return dq, dk, dqkv[..., col:col + Ckv].reshape(B, T, Hkv, D)

    ko.require(f"attn_qkvjoint/D{D}", ko.check_attn_bwd(bwd, case))
    outside = torch.cat([dqkv[..., :col], dqkv[..., col + Ckv:]], -1)
    assert (outside == SENT).all(), "attn_bwd_qkvjoint wrote outside dv block"


@pytest.mark.parametrize("D", [64, 80])
def test_fused_qkv_rope_attention_vs_fp64(D):
    """fused_qkv_rope_attention against an fp64 split + RoPE + attention
    reference (q, k rounded to bf16 after RoPE, as the kernels hand them
    on).  Rotated gradients: a rotation scales the max-norm by at most
    sqrt(2), and the final bf16 rounding adds 2^-8 of that."""
    from modalities_amd.ops.attention import fused_qkv_rope_attention
    from modalities_amd.ops.rope import precompute_rope_cos_sin
    g = torch.Generator().manual_seed(D)
    B, T, Hq, Hkv = 2, 130, 4, 2
    C, KV = Hq * D, Hkv * D
    cos, sin = precompute_rope_cos_sin(T, D, device=DEV)
    qkv = ko.bf(torch.randn(B, T, C + 2 * KV, generator=g)).to(DEV)
    do = ko.bf(torch.randn(B, T, Hq, D, generator=g)).to(DEV)
    a = qkv.clone().requires_grad_(True)
    y = fused_qkv_rope_attention(a, cos, sin, Hq, Hkv, D)
    y.backward(do)

    qs, ks, vs = qkv.split([C, KV, KV], dim=-1)
    qb = ko.bf(ko.rope_ref64(qs.reshape(B, T, Hq, D), cos, sin, False)[0])
    kb = ko.bf(ko.rope_ref64(ks.reshape(B, T, Hkv, D), cos, sin, False)[0])
    case = ko.AttnCase(dict(q=qb, k=kb, do=do,
                            v=vs.reshape(B, T, Hkv, D).contiguous()), 0)
    r, _, _ = ko.check_attn_fwd(lambda *_: (y.detach(), case.ref["lse"]),
                                case)
    ko.require(f"fused_qkv/D{D}/fwd", {"o": r["o"]})
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
    ko.require(f"fused_qkv/D{D}/bwd", res)


# ------------------------------------------------------------------ RoPE
ROPE_SHAPES = [(4, 1), (4, 255), (4, 257), (4, 384), (64, 24), (80, 1),
               (80, 13), (128, 12)]   # Hn*D/4 in {1, 255, 257, 384, 20, 260}


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("D,Hn", ROPE_SHAPES)
def test_rope_fwd(D, Hn, neg):
    rope = lambda x, c, s, n: EXT.rope_fwd(x, c, s, n)
    ko.require(f"rope_fwd/D{D}/Hn{Hn}",
               ko.check_rope(rope, 2, 3, Hn, D, neg, DEV, table_len=7))


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("col_off", [0, 6])
@pytest.mark.parametrize("D,Hn", ROPE_SHAPES)
def test_rope_fwd_slice(D, Hn, col_off, neg):
    def rope(x, c, s, n):
        B, T = x.shape[:2]
        qkv = torch.full((B, T, col_off + Hn * D + 10), 9.0, dtype=BF16,
                         device=DEV)
        qkv[..., col_off:col_off + Hn * D] = x.reshape(B, T, Hn * D)
        return EXT.rope_fwd_slice(qkv, c, s, col_off, Hn, D, n)
    ko.require(f"rope_fwd_slice/D{D}/Hn{Hn}/off{col_off}",
               ko.check_rope(rope, 2, 3, Hn, D, neg, DEV, table_len=7))


@pytest.mark.parametrize("col_off", [0, 6])
@pytest.mark.parametrize("D,Hn", ROPE_SHAPES)
def test_rope_bwd_slice(D, Hn, col_off):
    SENT = 9.0
    seen = {}

    def rope(x, c, s, n):
        B, T = x.shape[:2]
        dqkv = torch.full((B, T, col_off + Hn * D + 10), SENT, dtype=BF16,
                          device=DEV)
        EXT.rope_bwd_slice(x, c, s, dqkv, col_off)
        seen["outside"] = torch.cat([dqkv[..., :col_off],
                                     dqkv[..., col_off + Hn * D:]], -1)
        return dqkv[..., col_off:col_off + Hn * D].reshape(x.shape)
    ko.require(f"rope_bwd_slice/D{D}/Hn{Hn}/off{col_off}",
               ko.check_rope(rope, 2, 3, Hn, D, True, DEV, table_len=7))
    assert (seen["outside"] == SENT).all(), "rope_bwd_slice wrote outside"


# ------------------------------------------------------------ SiLU * mul
@pytest.mark.parametrize("numel", [8, 8 * (524288 + 3)])
def test_silu_mul(numel):
    """The second size forces a second grid-stride trip (2048 x 256 x 8)."""
    g, u, d = ko.silu_inputs(numel, DEV)
    r = ko.check_silu(lambda g_, u_: EXT.silu_mul_fwd(g_, u_),
                      lambda d_, g_, u_: tuple(EXT.silu_mul_bwd(d_, g_, u_)),
                      g, u, d)
    ko.require(f"silu_mul/n{numel}", r)


@pytest.mark.parametrize("rows,H", [(4099, 1032), (5, 24)])
def test_silu_mul_joint(rows, H):
    g, u, d = ko.silu_inputs(rows * H, DEV)
    wv = torch.cat([g.view(rows, H), u.view(rows, H)], -1).contiguous()

    def fwd(g_, u_):
        return EXT.silu_mul_joint_fwd(wv).reshape(-1)

    def bwd(d_, g_, u_):
        dwv = EXT.silu_mul_joint_bwd(d_.view(rows, H), wv)
        return dwv[:, :H].reshape(-1), dwv[:, H:].reshape(-1)

    ko.require(f"silu_mul_joint/{rows}x{H}", ko.check_silu(fwd, bwd, g, u, d))


# --------------------------------------------------------------- RMSNorm
def _rms_fwd(x, w, eps):
    return tuple(EXT.rmsnorm_fwd(x, w, eps))


def _rms_bwd(dy, x, w, r):
    return tuple(EXT.rmsnorm_bwd(dy, x, w, r))


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("H", [8, 64, 200, 520, 1000, 1024, 2560, 4096, 4104,
                               8192])
def test_rmsnorm(H, eps):
    """Every slot instantiation <1,2,5,8,16>, partial slots (H/8 not a
    multiple of 64), an all-zero row and rows scaled by 1e3 / 1e-3."""
    for N in (1, 3, 5, 257):
        ko.require(f"rmsnorm/N{N}/H{H}/eps{eps}",
                   ko.check_rmsnorm(_rms_fwd, _rms_bwd, N, H, eps, DEV))


def test_rmsnorm_many_rows_atomic_merge():
    """N=8200: rows_per_block = 5, 1640 blocks, 26 reduce chunks."""
    ko.require("rmsnorm/N8200/H128",
               ko.check_rmsnorm(_rms_fwd, _rms_bwd, 8200, 128, 1e-6, DEV))


def test_rmsnorm_fwd_rows_not_multiple_of_8():
    """H=100: rows are only 8-byte aligned, the scalar loop covers them."""
    ko.require("rmsnorm_fwd/N5/H100",
               ko.check_rmsnorm(_rms_fwd, None, 5, 100, 1e-6, DEV))
    x, w, dy = ko.rmsnorm_inputs(5, 100, DEV)
    _, r = EXT.rmsnorm_fwd(x, w, 1e-6)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_bwd(dy, x, w, r)


# --------------------------------------------------------- cross entropy
def _ce_fwd(l, t, ig):
    return tuple(EXT.cross_entropy_fwd(l, t, ig))


def _ce_bwd(l, t, lse, sc, ig):
    return EXT.cross_entropy_bwd(l, t, lse, sc, ig)


@pytest.mark.parametrize("kind", ["random", "mixed", "big", "neginf"])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("V", [8, 1000, 1004, 257])
def test_cross_entropy(V, N, kind):
    """Scalar tails (V % 8 != 0), targets at column 0, V-1 and in the tail,
    an ignored row, +-3e4 logits, -inf columns; scale != 1.  dlogits is
    checked elementwise, so the softmax part is visible."""
    logits, targets = ko.ce_inputs(N, V, DEV, kind)
    ko.require(f"ce/{kind}/N{N}/V{V}",
               ko.check_ce(_ce_fwd, _ce_bwd, logits, targets, scale=0.37))
    if kind == "neginf":
        losses, lse = EXT.cross_entropy_fwd(logits, targets, -100)
        ref = torch.nn.functional.cross_entropy(logits.float(), targets,
                                                reduction="none")
        torch.testing.assert_close(losses, ref, rtol=1e-5, atol=1e-5)
        d = EXT.cross_entropy_bwd(logits, targets, lse, torch.tensor(
            0.37, device=DEV), -100)
        assert (d[torch.isinf(logits)] == 0).all()


def test_cross_entropy_full_vocab():
    logits, targets = ko.ce_inputs(3, 50304, DEV, "mixed")
    ko.require("ce/mixed/N3/V50304",
               ko.check_ce(_ce_fwd, _ce_bwd, logits, targets, scale=1 / 3))


@pytest.mark.parametrize("V", [257, 1000])
def test_cross_entropy_all_rows_ignored(V):
    from modalities_amd.ops import fused_cross_entropy
    logits, targets = ko.ce_inputs(3, V, DEV, "ignored")
    lg = logits.clone().requires_grad_(True)
    loss = fused_cross_entropy(lg, targets)
    loss.backward()
    assert loss.item() == 0.0
    assert (lg.grad == 0).all()


# ------------------------------------------------- AdamW, norm and scale
BIG_N = 4 * (524288 + 5)   # second grid-stride trip of the float4 kernels


def _devstep(p, g, m, v, mask, t, gs, hp):
    step = torch.tensor(t, dtype=torch.int32, device=DEV)
    out = torch.empty(p.numel(), dtype=BF16, device=DEV)
    EXT.fused_adamw_masked_devstep(p, g, m, v, mask, step, out, gs, hp["lr"],
                                   hp["b1"], hp["b2"], hp["eps"], hp["wd"])
    return out


def _masked(p, g, m, v, mask, t, gs, hp):
    assert gs is None
    EXT.fused_adamw_masked(p, g, m, v, mask, hp["lr"], hp["b1"], hp["b2"],
                           hp["eps"], hp["wd"], hp["bc1"], hp["bc2"])


@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_adamw_devstep(t, betas):
    """The production optimizer kernel against fp64 AdamW: on-device bias
    correction, gscale folding, masks 0 / 1 / fractional, grads
    0 / 1e-8 / 1e4, and the fused bf16 publish (bit-identical to
    p.to(bfloat16)).  The p0 = 0, wd = 0 runs isolate the update."""
    for n in (4, BIG_N):
        for gs in (None, 0.0371):
            for p_zero in (False, True):
                ko.require(f"adamw_devstep/n{n}/t{t}/b2={betas[1]}/gs{gs}/"
                           f"p0={p_zero}",
                           ko.check_adamw(_devstep, n, t, betas, DEV,
                                          gscale=gs, p_zero=p_zero))


@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)])
@pytest.mark.parametrize("t", [1, 10, 1000])
def test_adamw_masked_host_bias_correction(t, betas):
    for n in (4, BIG_N):
        ko.require(f"adamw_masked/n{n}/t{t}/b2={betas[1]}",
                   ko.check_adamw(_masked, n, t, betas, DEV, host_bc=True,
                                  has_bf16=False))


def test_fused_adamw_list_of_three():
    """fused_adamw (weight-decay mask of ones) on a list of 3 tensors, one
    call; m, v and p of every tensor against fp64."""
    t, (b1, b2) = 3, (0.9, 0.95)
    hp = dict(ko.HP, b1=b1, b2=b2, bc1=1 - b1 ** t, bc2=1 - b2 ** t)
    sets = [ko.adamw_inputs(n, DEV, seed=s)
            for s, n in enumerate((4, 4 * 1031, 256))]
    refs = [ko.adamw_ref64(p, g, m, v, torch.ones_like(p), t, b1, b2,
                           hp["lr"], hp["eps"], hp["wd"], None,
                           (hp["bc1"], hp["bc2"]))
            for p, g, m, v, _ in sets]
    EXT.fused_adamw([s[0] for s in sets], [s[1] for s in sets],
                    [s[2] for s in sets], [s[3] for s in sets], hp["lr"], b1,
                    b2, hp["eps"], hp["wd"], hp["bc1"], hp["bc2"])
    for i, ((p, g, m, v, _), r) in enumerate(zip(sets, refs)):
        ko.require(f"fused_adamw/tensor{i}", {
            "m": ko.f32_sum_ratio(m, r["m"], r["S_m"], ko.F32_TINY),
            "v": ko.f32_sum_ratio(v, r["v"], r["S_v"], ko.F32_TINY),
            "p": ko.ratio((p.double() - r["p"]).abs(),
                          2.0 ** -20 * r["S_p"] + ko.F32_TINY)})


def test_devstep_bf16_copy_keeps_nan():
    """An fp32 NaN whose payload lives in the low 16 bits (0x7F800001)
    must come out of the fused bf16 publish as a NaN, not as Inf."""
    n = 8
    p = torch.zeros(n, device=DEV)
    p.view(torch.int32)[3] = 0x7F800001
    assert torch.isnan(p[3])
    z = torch.zeros(n, device=DEV)
    out = _devstep(p, z.clone(), z.clone(), torch.ones(n, device=DEV),
                   z.clone(), 1, None, dict(ko.HP, b1=0.9, b2=0.95))
    assert torch.isnan(out[3].float()) and torch.isnan(p[3])
    assert torch.isfinite(out.float()[[0, 1, 2, 4, 5, 6, 7]]).all()


SQ_SIZES = [4, BIG_N, 8, 12, 256]


def test_multi_tensor_sqsum():
    sq = lambda ts: EXT.multi_tensor_sqsum(ts)
    ko.require("sqsum/single4", ko.check_sqsum(sq, [4], DEV))
    ko.require("sqsum/single_big", ko.check_sqsum(sq, [BIG_N], DEV))
    ko.require("sqsum/list5", ko.check_sqsum(sq, SQ_SIZES, DEV))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_multi_tensor_scale(dtype):
    """In-place scale must equal the rounded fp64 product bit for bit,
    including the grid-stride remainder; scale as a device scalar of either
    dtype (bf16: the value is widened, not the product narrowed)."""
    s = torch.tensor(0.0371, dtype=dtype, device=DEV)
    sc = lambda ts, s_: EXT.multi_tensor_scale(ts, s_)
    ko.require(f"scale/{dtype}", ko.check_scale(sc, SQ_SIZES, s, DEV))


# -------------------------------------------------------- negative tests
# Every call below would stay in bounds even without the check it tests:
# the offending tensor is LARGER than needed, has the same element count
# in a wider dtype, or the kernel handles the value (numel % 4, q_offset).
def _bf(*shape):
    return torch.zeros(*shape, dtype=BF16, device=DEV)


def _f(*shape):
    return torch.zeros(*shape, dtype=F32, device=DEV)


def test_multi_tensor_scale_rejects_bad_arguments():
    s = torch.tensor(0.5, device=DEV)
    for bad in (_f(6),                                   # numel % 4 != 0
                torch.zeros(4, dtype=torch.float64, device=DEV),
                _f(8)[::2]):                             # non-contiguous
        with pytest.raises(RuntimeError):
            EXT.multi_tensor_scale([_f(4), bad], s)
    t = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError):     # validated before the first launch
        EXT.multi_tensor_scale([t, _f(6)], s)
    assert (t == 1).all()


def test_silu_mul_rejects_mismatched_arguments():
    g = _bf(8)
    with pytest.raises(RuntimeError):
        EXT.silu_mul_fwd(g, _bf(16))
    with pytest.raises(RuntimeError):
        EXT.silu_mul_fwd(g, _f(8))
    with pytest.raises(RuntimeError):
        EXT.silu_mul_bwd(_bf(16), g, _bf(8))
    with pytest.raises(RuntimeError):
        EXT.silu_mul_bwd(_bf(8), g, _f(8))
    with pytest.raises(RuntimeError):
        EXT.silu_mul_joint_bwd(_bf(2, 16), _bf(2, 16))   # dout twice too big
    with pytest.raises(RuntimeError):
        EXT.silu_mul_joint_bwd(_f(2, 8), _bf(2, 16))


def test_rmsnorm_rejects_mismatched_arguments():
    N, H = 3, 16
    x, w, dy, r = _bf(N, H), _bf(H), _bf(N, H), _f(N)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_fwd(x, _bf(2 * H), 1e-6)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_fwd(x, _f(H), 1e-6)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_bwd(_bf(N + 1, H), x, w, r)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_bwd(dy, x, _bf(2 * H), r)
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_bwd(dy, x, w, _f(N + 4))
    with pytest.raises(RuntimeError):
        EXT.rmsnorm_bwd(dy, x, w, torch.zeros(N, dtype=torch.float64,
                                              device=DEV))


def test_cross_entropy_bwd_rejects_mismatched_arguments():
    N, V = 3, 16
    lg = _bf(N, V)
    tg = torch.zeros(N, dtype=torch.int64, device=DEV)
    lse, s = _f(N), torch.tensor(1.0, device=DEV)
    with pytest.raises(RuntimeError):
        EXT.cross_entropy_bwd(lg, tg, _f(N + 1), s, -100)
    with pytest.raises(RuntimeError):
        EXT.cross_entropy_bwd(lg, tg, torch.zeros(N, dtype=torch.float64,
                                                  device=DEV), s, -100)
    with pytest.raises(RuntimeError):
        EXT.cross_entropy_bwd(lg, torch.zeros(N + 1, dtype=torch.int64,
                                              device=DEV), lse, s, -100)
    with pytest.raises(RuntimeError):
        EXT.cross_entropy_bwd(_f(N, V), tg, lse, s, -100)


def test_attn_v2_rejects_mismatched_arguments():
    B, T, H, D = 1, 64, 2, 64
    q, k, v = _bf(B, T, H, D), _bf(B, T, H, D), _bf(B, T, H, D)
    with pytest.raises(RuntimeError):
        EXT.attn_fwd_v2(q, k, v, True, -1)
    with pytest.raises(RuntimeError):
        EXT.attn_fwd_v2(q, k, _bf(B, T + 8, H, D), True, 0)
    with pytest.raises(RuntimeError):
        EXT.attn_fwd_v2(q, _f(B, T, H, D), v, True, 0)
    o, lse = EXT.attn_fwd_v2(q, k, v, True, 0)
    do = _bf(B, T, H, D)
    with pytest.raises(RuntimeError):
        EXT.attn_bwd_v2(do, q, k, v, o, lse, True, -1)
    with pytest.raises(RuntimeError):
        EXT.attn_bwd_v2(_bf(B + 1, T, H, D), q, k, v, o, lse, True, 0)
    with pytest.raises(RuntimeError):
        EXT.attn_bwd_v2(do, q, k, v, _f(B, T, H, D), lse, True, 0)
    with pytest.raises(RuntimeError):
        EXT.attn_bwd_v2(do, q, k, v, o, _f(B, H, T + 4), True, 0)
    with pytest.raises(RuntimeError):
        EXT.attn_bwd_v2(do, q, _f(B, T, H, D), v, o, lse, True, 0)
