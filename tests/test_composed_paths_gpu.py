"""GPU tests for the code that composes the HIP kernels, against the fp64
oracles of tests/composed_oracles.py: the attention backward with a gradient
of its lse output, one rank of ring context parallelism (forward and
backward, through the production _flash_with_lse), and the optimizer tail
ShardedAdamW + XGMIShardedModel.clip_grad_norm_.
tests/test_composed_oracles_cpu.py proves on the CPU that these checkers
reject subtly wrong implementations.

Worst measured error / bound on an MI355X (every check asserts <= 1; the
bounds are derived in tests/composed_oracles.py and tests/kernel_oracles.py,
none is fitted):

  path / case family                   worst error / bound
  -----------------------------------  ----------------------------------------
  attn_bwd with dlse, v2 D 64/80/128   dq 0.68  dk 0.57  dv 0.49
  attn_bwd with dlse, v1 D 64/128      dq 0.68  dk 0.57  dv 0.49
  dlse = None vs dlse = zeros          dq, dk, dv bit-identical
  custom op, grads of (o, lse)         dq 0.45  dk 0.48  dv 0.48
  ring rank, forward                   o 0.38
  ring rank, backward                  dq 0.67  dk 0.94  dv 0.49
  ring rank, keys after own chunk      dk, dv exactly zero
  optimizer, bf16 working copy         m 0.042  v 0.079  p 0.29  norm 0.015
  optimizer, warm start (t = 8)        m 0.015  v 0.026  p 0.18
  optimizer, fp32 working copy         m 0.042  v 0.079  p 0.19  norm 0.051

  optimizer: published copy bit-identical, step counters exact, mask equal
  in every row above.

  ring backward, kernel / CPU-ring-emulation error ratio
  (max|kernel-ref| / max|emul-ref|): dv 1.0 everywhere; dq up to 1.38; dk
  up to 2.01 (D = 80, cp 2, Tl 130, rank 1; next 1.74 and 1.71).  The bound
  allows 2 plus the 2^-12 max|ref| term, which is what keeps that one case
  at 0.94.  The factor 2 was taken over from the single-kernel rule (at
  most 1.8 there, with the backward handed the emulation's own o and lse);
  here each side runs its own forward, so o and lse differ between them,
  and the figures above are the factor's first measurement on the composed
  path.  The kernels are deterministic, so the figures do not move between
  runs.  With dlse on a single kernel: dq 1.43, dk 1.21, dv 1.0.
"""

import functools

import pytest
import torch

from tests import composed_oracles as co
from tests import kernel_oracles as ko
from tests.composed_oracles import DLSE_SHAPES, RING_CASES, RING_IDS

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"

# (kernel generation, head_dim): v2 for all three head dims, v1 for 64/128
IMPLS = [(2, 64), (2, 80), (2, 128), (1, 64), (1, 128)]
IMPL_IDS = [f"v{i}-D{d}" for i, d in IMPLS]


# ------------------------------------------------ A. backward with dlse
@functools.lru_cache(maxsize=None)
def _dlse_case(D, Tq, Tkv, off):
    return co.dlse_case(D, Tq, Tkv, off, DEV)


def _bwd(impl):
    f = EXT.attn_bwd_v1 if impl == 1 else EXT.attn_bwd_v2
    return lambda do, q, k, v, o, lse, off, dlse=None: tuple(
        f(do, q, k, v, o, lse, True, off, dlse))


@pytest.mark.parametrize("Tq,Tkv,off", DLSE_SHAPES)
@pytest.mark.parametrize("impl,D", IMPLS, ids=IMPL_IDS)
def test_attn_bwd_dlse(impl, D, Tq, Tkv, off):
    case = _dlse_case(D, Tq, Tkv, off)
    ko.require(f"attn_bwd_dlse/v{impl}/D{D}/{Tq}x{Tkv}+{off}",
               ko.check_attn_bwd(_bwd(impl), case))
    # no lse gradient and a zero one are the same computation
    args = (case.do, case.q, case.k, case.v, case.o_in, case.lse_in, off)
    none = _bwd(impl)(*args)
    zeros = _bwd(impl)(*args, torch.zeros_like(case.dlse))
    for n, a, b in zip(("dq", "dk", "dv"), none, zeros):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), n


@pytest.mark.parametrize("impl", [1, 2])
def test_attn_bwd_dlse_is_validated(impl):
    case = _dlse_case(64, 33, 33, 0)
    args = (case.do, case.q, case.k, case.v, case.o_in, case.lse_in, 0)
    B, Hq, T = case.dlse.shape
    for bad in (case.dlse.double(), case.dlse.cpu(), case.dlse[..., :T - 1],
                case.dlse.transpose(1, 2), case.dlse.reshape(B, Hq * T),
                torch.zeros(B, Hq, T + 1, device=DEV)):
        with pytest.raises(RuntimeError):
            _bwd(impl)(*args, bad)


def test_custom_op_backward_takes_grad_lse():
    """The dispatcher-visible op returns (o, lse); a loss that uses both
    must reach dq/dk through lse as well (flash_attention drops lse, where
    the gradient arrives as None)."""
    from modalities_amd.ops.attention import _ensure_custom_op
    assert _ensure_custom_op()
    case = _dlse_case(64, 33, 33, 0)

    def bwd(do, q, k, v, o, lse, off, dlse):
        q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        o, lse = torch.ops.modalities_amd.flash_attention(q, k, v, True, off)
        torch.autograd.backward((o, lse), (do, dlse))
        return q.grad, k.grad, v.grad

    ko.require("custom_op_dlse/D64/33x33+0", ko.check_attn_bwd(bwd, case))


# ------------------------------------------------ B. ring rank
@functools.lru_cache(maxsize=None)
def _ring_case(cp, Tl, D, r):
    return co.RingCase(cp, Tl, D, r, DEV)


@pytest.mark.parametrize("cp,Tl,r", RING_CASES, ids=RING_IDS)
@pytest.mark.parametrize("D", [64, 80, 128])
def test_ring_rank_fwd_bwd(D, cp, Tl, r):
    from modalities_amd.ops.backend import use_hip
    from modalities_amd.parallel.cp import _flash_with_lse
    case = _ring_case(cp, Tl, D, r)
    assert use_hip(case.q, case.k, case.v)   # the kernels, not the fp32 path
    ko.require(f"ring/D{D}/cp{cp}/Tl{Tl}/r{r}",
               co.check_ring_rank(_flash_with_lse, case, r, cp))


# ------------------------------------------------ C. optimizer tail
def _engine(param_dtype):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=64, n_layer=1, n_head_q=2, n_head_kv=1,
                        n_embd=64, ffn_hidden=128, sequence_length=32)
    model = XGMIShardedModel.from_transformer(
        GPT2LLM(cfg), torch.device(DEV), blocks_per_unit=1,
        param_dtype=param_dtype, rank=0, world_size=1)
    opt = get_adam_w(model, lr=co.OPT_HP["lr"], weight_decay=co.OPT_HP["wd"])
    assert (opt.defaults["betas"], opt.defaults["eps"]) == \
        ((co.OPT_HP["b1"], co.OPT_HP["b2"]), co.OPT_HP["eps"])
    return model, opt


def test_opt_sequence_bf16_working_copy():
    model, opt = _engine(torch.bfloat16)
    assert len(model.units) == 2
    assert all(u.bf16_shard.dtype == torch.bfloat16 for u in model.units)
    ko.require("opt/bf16/mask", co.check_wd_mask(model))
    ko.require("opt/bf16/sequence", co.check_opt_sequence(model, opt))
    assert int(opt._step_dev) == 3
    assert model._pending_grad_scale is None


def test_opt_warm_start_seeds_device_counter():
    model, opt = _engine(torch.bfloat16)
    ko.require("opt/bf16/warm", co.check_opt_warm_start(model, opt, start=7))
    assert int(opt._step_dev) == 8
    assert all(opt.state[u.master_shard]["step"] == 8 for u in model.units)


def test_opt_sequence_fp32_working_copy():
    """The unfused branch: g.mul(gscale), host bias corrections,
    publish_master."""
    model, opt = _engine(torch.float32)
    assert all(u.bf16_shard.dtype == torch.float32 for u in model.units)
    ko.require("opt/fp32/mask", co.check_wd_mask(model))
    ko.require("opt/fp32/sequence",
               co.check_opt_sequence(model, opt, host_bc=True, steps=2))


def test_opt_mixed_grad_fresh_raises_and_changes_nothing():
    model, opt = _engine(torch.bfloat16)
    co.write_grads(model, seed=3)
    model.units[0].grad_fresh = False
    before = [u.master_shard.clone() for u in model.units]
    with pytest.raises(RuntimeError, match="mixed grad_fresh"):
        opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(u.master_shard, b)
               for u, b in zip(model.units, before))
