"""Mutation self-test of tests/kernel_oracles.py (CPU only).

Every checker must accept the correct pure-torch implementation and
reject each deliberate mutant: the proof, on a machine without a GPU, that
tests/test_hip_kernels_edges_gpu.py would fail for a subtly wrong kernel.
The shapes are those the GPU tests use (or smaller ones of the same family).
"""

import functools

import pytest
import torch

from tests import kernel_oracles as ko

CPU = "cpu"


# ---------------------------------------------------------------- attention
@functools.lru_cache(maxsize=None)
def _case(kind, D, Tq, Tkv, off, B=1, Hq=2, Hkv=1):
    if kind == "random":
        inp = ko.attn_random_inputs(B, Tq, Tkv, Hq, Hkv, D, CPU, seed=1)
    else:
        inp = ko.attn_ramp_inputs(Tq, Tkv, D, {"ramp8": 8, "ramp1": 1}[kind],
                                  CPU, B, Hq, Hkv, seed=2)
    return ko.AttnCase(inp, off)


def _attn(mut=None):
    return lambda q, k, v, off: ko.torch_attn_fwd(q, k, v, off, mut)


def _attn_bwd(mut=None):
    return lambda do, q, k, v, o, lse, off: ko.torch_attn_bwd(
        do, q, k, v, o, lse, off, mut)


def _run_all_attn(mut, bwd_mut=None):
    """Every attention checker family on small shapes -> {label: ratios}."""
    out = {}
    for D, Tq, Tkv, off in [(64, 65, 65, 0), (80, 32, 96, 64),
                            (128, 1, 130, 129)]:
        case = _case("random", D, Tq, Tkv, off)
        r, o, lse = ko.check_attn_fwd(_attn(mut), case)
        out[f"random{D}"] = r
        out[f"random{D}_bwd"] = ko.check_attn_bwd(_attn_bwd(bwd_mut), case)
    case = _case("random", 64, 130, 130, 0, 3, 4, 2)     # GQA + batch
    out["gqa"] = ko.check_attn_fwd(_attn(mut), case)[0]
    case = _case("ramp8", 64, 128, 512, 384)
    r, o, lse = ko.check_attn_fwd(_attn(mut), case)
    out["ramp8"] = r
    out["ramp8_closed"] = ko.check_ramp_step8(case, o, lse)
    out["ramp8_dv"] = ko.check_attn_bwd(_attn_bwd(bwd_mut), case,
                                        which=("dv",))
    case = _case("ramp1", 80, 300, 300, 0)
    r, o, lse = ko.check_attn_fwd(_attn(mut), case)
    out["ramp1"] = r
    out["ramp1_bwd"] = ko.check_attn_bwd(_attn_bwd(bwd_mut), case)
    out["count"] = ko.check_attn_counting(_attn(mut), 64, 128, 512, 384, CPU)
    return out


def test_attention_correct_impl_accepted():
    res = _run_all_attn(None)
    for label, r in res.items():
        ko.require("cpu/" + label, r)
    out = ko.check_attn_counting(_attn(), 64, 2048, 2048, 0, CPU)
    ko.require("cpu/count2048", out)


@pytest.mark.parametrize("mut", [
    "mask_plus1", "mask_minus1", "drop_last_key", "gqa_mod", "ignore_offset",
    "lse_no_max", "skip_rescale"])
def test_attention_fwd_mutant_rejected(mut):
    res = _run_all_attn(mut)
    hits = [k for k, r in res.items() if ko.rejected(r)]
    print(mut, "rejected by", hits)
    assert hits, f"mutant {mut} passed every checker"
    if mut in ("mask_plus1", "mask_minus1"):
        # structured inputs see an off-by-one mask at ANY offset
        assert ko.rejected(res["ramp8_closed"]) and ko.rejected(res["count"])
    if mut == "skip_rescale":
        assert ko.rejected(res["ramp8"])


def test_attention_dropped_tile_rejected_at_2048():
    """One 64-key tile dropped at T=2048: the counting-V check sees it."""
    out = ko.check_attn_counting(_attn("drop_tile"), 64, 2048, 2048, 0, CPU)
    assert out["count"] > 1.0 and out["lse_log_n"] > 1.0, out


@pytest.mark.parametrize("mut", ["mask_plus1", "mask_minus1"])
def test_attention_bwd_mask_mutant_rejected(mut):
    """The backward kernels carry their own mask: ramp step 1 makes dq, dk
    and dv all sensitive to it."""
    case = _case("ramp1", 80, 300, 300, 0)
    r = ko.check_attn_bwd(_attn_bwd(mut), case)
    assert r["dq"] > 1 and r["dk"] > 1 and r["dv"] > 1, r


# ------------------------------------------------------------ cross entropy
def _ce(mut_f=None, mut_b=None):
    fwd = lambda l, t, ig: ko.torch_ce_fwd(l, t, ig, mut_f)
    bwd = lambda l, t, lse, sc, ig: ko.torch_ce_bwd(l, t, lse, sc, ig, mut_b)
    return fwd, bwd


CE_CASES = [(3, 1004, "random"), (3, 257, "mixed"), (1, 8, "random"),
            (3, 1000, "neginf"), (3, 1004, "big"), (3, 257, "ignored")]


def _run_ce(mut_f=None, mut_b=None):
    out = {}
    for N, V, kind in CE_CASES:
        logits, targets = ko.ce_inputs(N, V, CPU, kind)
        out[f"{kind}{V}"] = ko.check_ce(*_ce(mut_f, mut_b), logits, targets,
                                        scale=0.37)
    return out


def test_ce_correct_impl_accepted():
    for label, r in _run_ce().items():
        ko.require("cpu/ce/" + label, r)


@pytest.mark.parametrize("mut_f,mut_b", [(None, "zero_softmax"),
                                         (None, "keep_ignored"),
                                         ("skip_tail", "skip_tail")])
def test_ce_mutant_rejected(mut_f, mut_b):
    res = _run_ce(mut_f, mut_b)
    hits = [k for k, r in res.items() if ko.rejected(r)]
    assert hits, f"CE mutant {(mut_f, mut_b)} passed every checker"


def test_ce_softmax_part_visible_at_large_vocab():
    """The gap the old atol=1e-4 left open: at V=50304 the softmax part of
    dlogits is ~1/(N*V); zeroing it must still be rejected."""
    logits, targets = ko.ce_inputs(3, 50304, CPU, "random")
    r = ko.check_ce(*_ce(None, "zero_softmax"), logits, targets, scale=1 / 3)
    assert r["dlogits"] > 1.0, r
    ko.require("cpu/ce/50304", ko.check_ce(*_ce(), logits, targets,
                                           scale=1 / 3))


# ------------------------------------------------------------------ RMSNorm
def _rms(mut_f=None, mut_b=None):
    fwd = lambda x, w, eps: ko.torch_rmsnorm_fwd(x, w, eps, mut_f)
    bwd = lambda dy, x, w, r: ko.torch_rmsnorm_bwd(dy, x, w, r, mut_b)
    return fwd, bwd


def test_rmsnorm_correct_impl_accepted():
    for N, H in [(5, 200), (257, 64), (3, 1000), (1, 8)]:
        for eps in (1e-6, 1e-5):
            ko.require(f"cpu/rms/{N}x{H}",
                       ko.check_rmsnorm(*_rms(), N, H, eps, CPU))
    fwd, _ = _rms()
    ko.require("cpu/rms/fwd_only_100", ko.check_rmsnorm(fwd, None, 5, 100,
                                                       1e-6, CPU))


def test_rmsnorm_mutants_rejected():
    r = ko.check_rmsnorm(*_rms(None, "drop_kx"), 5, 200, 1e-6, CPU)
    assert r["dx"] > 1 and r["dw"] <= 1, r
    r = ko.check_rmsnorm(*_rms(None, "dw_last_row"), 3, 200, 1e-6, CPU)
    assert r["dw"] > 1 and r["dx"] <= 1, r
    fwd, _ = _rms("mean_vec8")
    r = ko.check_rmsnorm(fwd, None, 5, 100, 1e-6, CPU)
    assert r["invrms"] > 1, r


# --------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("D,H", [(4, 1), (64, 16), (80, 3), (128, 2)])
def test_rope_correct_accepted_mutants_rejected(D, H):
    for neg in (False, True):
        rope = lambda x, c, s, n: ko.torch_rope(x, c, s, n)
        ko.require(f"cpu/rope/{D}", ko.check_rope(rope, 2, 3, H, D, neg, CPU))
        for mut in ("sin_sign", "adjacent_pairs", "row_plus1"):
            bad = lambda x, c, s, n, m=mut: ko.torch_rope(x, c, s, n, m)
            r = ko.check_rope(bad, 2, 3, H, D, neg, CPU)
            assert r["y"] > 1, (mut, D, r)


# --------------------------------------------------------------- SiLU * mul
def test_silu_correct_impl_accepted():
    g, u, d = ko.silu_inputs(8 * 64, CPU)
    r = ko.check_silu(ko.torch_silu_fwd, ko.torch_silu_bwd, g, u, d)
    ko.require("cpu/silu", r)
    wrong = lambda d_, g_, u_: ko.torch_silu_bwd(d_, g_, u_)[::-1]
    assert ko.rejected(ko.check_silu(ko.torch_silu_fwd, wrong, g, u, d))


# -------------------------------------------------------------------- AdamW
def _adamw(mut=None, devstep=True):
    def step(p, g, m, v, mask, t, gs, hp):
        bc = None if devstep else (hp["bc1"], hp["bc2"])
        return ko.torch_adamw_step(p, g, m, v, mask, t, hp["b1"], hp["b2"],
                                   hp["lr"], hp["eps"], hp["wd"], gs, bc, mut)
    return step


ADAMW_GRID = [(n, t, betas, gs) for n in (4, 4 * 37)
              for t in (1, 2, 10, 1000, 100000)
              for betas in ((0.9, 0.95), (0.9, 0.999))
              for gs in (None, 0.0371)]


def _run_adamw(mut):
    out = {}
    for n, t, betas, gs in ADAMW_GRID:
        out[(n, t, betas, gs, "p0")] = ko.check_adamw(
            _adamw(mut), n, t, betas, CPU, gs, p_zero=True)
        out[(n, t, betas, gs)] = ko.check_adamw(
            _adamw(mut, devstep=False), n, t, betas, CPU, gs, host_bc=True)
    return out


def test_adamw_correct_impl_accepted():
    for label, r in _run_adamw(None).items():
        ko.require(f"cpu/adamw/{label}", r)


@pytest.mark.parametrize("mut", ["bc2_frozen", "decay_after", "v_frozen",
                                 "bf16_trunc"])
def test_adamw_mutant_rejected(mut):
    hits = [k for k, r in _run_adamw(mut).items() if ko.rejected(r)]
    assert hits, f"AdamW mutant {mut} passed every checker"


def test_sqsum_and_scale_checkers():
    sq = lambda ts: sum(t.pow(2).sum() for t in ts)
    ko.require("cpu/sqsum", ko.check_sqsum(sq, [4, 4 * 37, 8, 12, 16], CPU))
    drop = lambda ts: sum(t[:-1].pow(2).sum() for t in ts)
    assert ko.rejected(ko.check_sqsum(drop, [4, 4 * 37], CPU))

    def scale_(ts, s):
        for t in ts:
            t.mul_(s.float())

    def scale_skip_tail(ts, s):
        for t in ts:
            t[:t.numel() // 8 * 8].mul_(s.float())

    s = torch.tensor(0.0371, dtype=torch.bfloat16)
    ko.require("cpu/scale", ko.check_scale(scale_, [4, 4 * 37], s, CPU))
    assert ko.rejected(ko.check_scale(scale_skip_tail, [4, 4 * 37], s, CPU))
