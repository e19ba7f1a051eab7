"""CPU proof for tests/composed_oracles.py: every checker accepts the
correct pure-torch implementation and rejects deliberate mutants, at the
shapes tests/test_composed_paths_gpu.py uses.  No GPU needed."""

import functools

import pytest
import torch

from tests import composed_oracles as co
from tests import kernel_oracles as ko
from tests.composed_oracles import DLSE_SHAPES, RING_CASES, RING_IDS

CPU = "cpu"

# ------------------------------------------------ A. backward with dlse
@functools.lru_cache(maxsize=None)
def _dlse_case(D, Tq, Tkv, off):
    return co.dlse_case(D, Tq, Tkv, off, CPU)


def _torch_bwd(mut=None):
    return lambda do, q, k, v, o, lse, off, dlse: ko.torch_attn_bwd(
        do, q, k, v, o, lse, off, mut=mut, dlse=dlse)


@pytest.mark.parametrize("Tq,Tkv,off", DLSE_SHAPES)
@pytest.mark.parametrize("D", [64, 80])
def test_dlse_backward_accepts_emulation_rejects_drop(D, Tq, Tkv, off):
    case = _dlse_case(D, Tq, Tkv, off)
    label = f"dlse/D{D}/{Tq}x{Tkv}+{off}"
    ko.require(label, ko.check_attn_bwd(_torch_bwd(), case))
    r = ko.check_attn_bwd(_torch_bwd("drop_dlse"), case)
    print(f"ORACLE {label}/drop_dlse: {r}")
    # (at a single key P = 1 and dP = delta: dS = dlse is all there is)
    assert r["dq"] > 1 and r["dk"] > 1
    assert r["dv"] <= 1     # dv does not depend on dlse


def test_dlse_reference_matches_autograd():
    """attn_ref64's dlse term against fp64 autograd of sum(o*do)+sum(lse*dlse)
    (the oracle itself is not taken on trust)."""
    import math
    case = _dlse_case(64, 33, 33, 0)
    q, k, v = (t.double().requires_grad_(True)
               for t in (case.q, case.k, case.v))
    B, Tq, Hq, D = q.shape
    qd = q.permute(0, 2, 1, 3)
    kd, vd = ko._expand(k, Hq), ko._expand(v, Hq)
    s = (qd @ kd.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~ko.causal_mask(Tq, Tq, 0, CPU), -ko.INF)
    lse = torch.logsumexp(s, -1)
    o = (torch.softmax(s, -1) @ vd).permute(0, 2, 1, 3)
    ((o * case.do.double()).sum() + (lse * case.dlse.double()).sum()).backward()
    for n, t in (("dq", q), ("dk", k), ("dv", v)):
        err = (t.grad - case.ref[n]).abs().max().item()
        assert err < 1e-12, (n, err)


def test_dlse_zeros_equals_none_in_emulation():
    case = _dlse_case(64, 33, 33, 0)
    a = ko.torch_attn_bwd(case.do, case.q, case.k, case.v, case.o_in,
                          case.lse_in, 0)
    b = ko.torch_attn_bwd(case.do, case.q, case.k, case.v, case.o_in,
                          case.lse_in, 0, dlse=torch.zeros_like(case.dlse))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------ B. ring rank
@functools.lru_cache(maxsize=None)
def _ring_case(cp, Tl, D, r):
    return co.RingCase(cp, Tl, D, r, CPU)


@pytest.mark.parametrize("cp,Tl,r", RING_CASES, ids=RING_IDS)
@pytest.mark.parametrize("D", [64, 80, 128])
def test_ring_accepts_correct_composition(D, cp, Tl, r):
    case = _ring_case(cp, Tl, D, r)
    label = f"ring/D{D}/cp{cp}/Tl{Tl}/r{r}"
    ko.require(label + "/torch_kernel",
               co.check_ring_rank(co.torch_flash_with_lse(), case, r, cp))
    # the production CPU path (composed fp32, differentiated by autograd)
    from modalities_amd.parallel.cp import _flash_with_lse
    ko.require(label + "/composed_fp32",
               co.check_ring_rank(_flash_with_lse, case, r, cp))


@pytest.mark.parametrize("cp,Tl,r", RING_CASES, ids=RING_IDS)
@pytest.mark.parametrize("D", [64, 80, 128])
def test_ring_rejects_dropped_dlse(D, cp, Tl, r):
    case = _ring_case(cp, Tl, D, r)
    mutant = co.torch_flash_with_lse("drop_dlse")
    if r == 0:
        # one partial, no merge: lse is unused and the mutant is the same
        got = co.run_ring_rank(mutant, case.q, case.k, case.v, case.do, r, cp)
        assert all(torch.equal(a, b) for a, b in zip(got, case.emul))
        return
    res = co.check_ring_rank(mutant, case, r, cp)
    print(f"ORACLE ring/D{D}/cp{cp}/Tl{Tl}/r{r}/drop_dlse: {res}")
    assert res["dq"] > 1 and res["dk"] > 1
    assert res["o"] <= 1 and res["dv"] <= 1


@pytest.mark.parametrize("cp,Tl,r", [c for c in RING_CASES if c[2] >= 1],
                         ids=[i for c, i in zip(RING_CASES, RING_IDS)
                              if c[2] >= 1])
def test_ring_rejects_causal_off_diagonal_and_swapped_weights(
        cp, Tl, r, monkeypatch):
    case = _ring_case(cp, Tl, 64, r)
    res = co.check_ring_rank(co.torch_flash_with_lse("causal_off_diag"),
                             case, r, cp)
    assert res["o"] > 1 and ko.rejected(res)
    from modalities_amd.parallel import cp as cp_mod
    monkeypatch.setattr(cp_mod, "_merge_partials", co.merge_swapped_weights)
    res = co.check_ring_rank(co.torch_flash_with_lse(), case, r, cp)
    assert res["o"] > 1 and ko.rejected(res)


# ------------------------------------------------ C. optimizer tail
def _stand_in(mut=None):
    model = co.TorchShardedStandIn()
    return model, co.TorchAdamWStandIn(model, mut=mut)


def test_opt_stand_in_accepted():
    model, opt = _stand_in()
    ko.require("opt/stand_in/mask", co.check_wd_mask(model))
    ko.require("opt/stand_in/sequence", co.check_opt_sequence(model, opt))
    model, opt = _stand_in()
    ko.require("opt/stand_in/warm", co.check_opt_warm_start(model, opt))
    assert int(opt._step_dev) == 8


def test_opt_rejects_stale_gscale():
    model, opt = _stand_in("stale_gscale")
    res = co.check_opt_sequence(model, opt)
    print(f"ORACLE opt/stale_gscale: {res}")
    # step 1 is right; step 2 reuses step 1's coefficient
    assert not ko.rejected({k: v for k, v in res.items()
                            if k.startswith("s1/")})
    assert res["s2/m"] > 1 and res["s2/v"] > 1


def test_opt_rejects_counter_zero_after_warm_start():
    model, opt = _stand_in("warm_counter_zero")
    res = co.check_opt_warm_start(model, opt)
    print(f"ORACLE opt/warm_counter_zero: {res}")
    assert res["p"] > 1 and res["step"] > 1
    # without a warm start the mutant is the correct optimizer
    model, opt = _stand_in("warm_counter_zero")
    ko.require("opt/warm_counter_zero/cold",
               co.check_opt_sequence(model, opt))


def test_opt_rejects_all_ones_mask():
    model, opt = _stand_in("ones_mask")
    ko.require("opt/ones_mask/declared_mask", co.check_wd_mask(model))
    res = co.check_opt_sequence(model, opt)
    print(f"ORACLE opt/ones_mask: {res}")
    assert res["s1/p"] > 1 and res["s1/m"] <= 1 and res["s1/v"] <= 1


def test_opt_rejects_wrong_declared_mask_and_publish():
    model, opt = _stand_in()
    model.units[0].wd_mask_shard[0] = 0.0      # a 2-D parameter's element
    assert co.check_wd_mask(model)["wd_mask"] > 1
    model, opt = _stand_in()
    gs = co.write_grads(model, seed=5)
    step = opt.step

    def truncating_step():
        step()
        for u in model.units:   # publish by truncation, not RNE
            u.bf16_shard = (u.master_shard.view(torch.int32) & -65536).view(
                torch.float32).to(torch.bfloat16)
    opt.step = truncating_step
    assert co.checked_step(model, opt, gs, 1, None)["publish_bits"] > 1


def test_opt_production_cpu_path_accepted():
    """The engine's own CPU branch (host bias corrections, eager clip)
    through the same checker: the oracle agrees with a second, independent
    implementation of the same tail."""
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=64, n_layer=1, n_head_q=2, n_head_kv=1,
                        n_embd=64, ffn_hidden=128, sequence_length=32)
    model = XGMIShardedModel.from_transformer(
        GPT2LLM(cfg), torch.device("cpu"), blocks_per_unit=1,
        param_dtype=torch.float32, rank=0, world_size=1)
    opt = get_adam_w(model, lr=co.OPT_HP["lr"],
                     weight_decay=co.OPT_HP["wd"])
    ko.require("opt/engine_cpu/mask", co.check_wd_mask(model))
    ko.require("opt/engine_cpu/sequence",
               co.check_opt_sequence(model, opt, host_bc=True))
