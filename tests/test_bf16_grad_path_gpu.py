"""GPU tests of the engine's bf16-gradient path: with one micro-batch per
step the reduced bf16 gradient stays pending, and clip_grad_norm_ and
ShardedAdamW.step read it in place (multi_tensor_sqsum_bf16,
fused_adamw_devstep_bf16g with the bit-packed decay mask).

Every case runs two engines built from the same seed, one of them with
MODALITIES_AMD_BF16_GRAD_PATH=0 (it materializes the fp32 gradient at reduce
time and takes the fp32 kernels).  bf16 -> fp32 is exact and both AdamW
entries share one update body, so the optimizer state of the two must be
BIT-IDENTICAL wherever the clip coefficient is (None or exactly 1.0): no
tolerance is involved.  Where the clip is active the coefficient comes out
of float atomics in either engine; there the returned norms are held to the
fp64 sum of squares at the bound of tests/composed_oracles.check_total_norm.

The config is the tiny one of tests/test_composed_paths_gpu.py (vocab 64,
1 layer, n_embd 64, seq 32) with a single head, so that head_dim is 64 and
the forward can run on the attention kernels: two units, both masks mixed
0/1.
"""

import pytest
import torch

from tests import composed_oracles as co
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCH = "MODALITIES_AMD_BF16_GRAD_PATH"
V, T, B = 64, 32, 2


def _engine(monkeypatch, fast):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    if fast:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")
    torch.manual_seed(0)
    # one head of 64: the smallest head_dim the attention kernels take
    cfg = GPT2LLMConfig(vocab_size=V, n_layer=1, n_head_q=1, n_head_kv=1,
                        n_embd=64, ffn_hidden=128, sequence_length=T)
    model = XGMIShardedModel.from_transformer(
        GPT2LLM(cfg), torch.device(DEV), blocks_per_unit=1,
        param_dtype=torch.bfloat16, rank=0, world_size=1)
    opt = get_adam_w(model, lr=1e-3, weight_decay=0.1)
    assert all(u.keep_bf16_grads == fast for u in model.units)
    return model, opt


def _pair(monkeypatch):
    fast, slow = _engine(monkeypatch, True), _engine(monkeypatch, False)
    assert _same(_state(*fast), _state(*slow))
    return fast, slow


def _batch(step):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randint(0, V, (B, T + 1), generator=g).to(DEV)


def _backward(model, ids, loss_scale=1.0):
    from modalities_amd.ops import fused_cross_entropy
    out = model({"input_ids": ids[:, :-1]})
    loss = fused_cross_entropy(out["logits"], ids[:, 1:]) * loss_scale
    loss.backward()
    return loss


def _step(model, opt, ids, max_norm, loss_scale=1.0):
    loss = _backward(model, ids, loss_scale)
    model.backward_epilogue()
    total = model.clip_grad_norm_(max_norm)
    opt.step()
    opt.zero_grad()
    return loss, total


def _state(model, opt):
    out = []
    for u in model.units:
        st = opt.state[u.master_shard]
        out += [u.master_shard, st["exp_avg"], st["exp_avg_sq"], u.bf16_shard]
    return out


def _same(xs, ys):
    bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16
                            else torch.int32)
    return len(xs) == len(ys) and all(
        torch.equal(bits(x), bits(y)) for x, y in zip(xs, ys))


def _fill_nan(model):
    for u in model.units:
        assert u._pending_grad is None
        u.grad_shard.fill_(float("nan"))


def _still_nan(model):
    return all(u._pending_grad is None and torch.isnan(u.grad_shard).all()
               for u in model.units)


@pytest.mark.parametrize("max_norm", [None, 1e9])
def test_single_micro_batch_matches_and_never_materializes(monkeypatch,
                                                           max_norm):
    (fm, fo), (sm, so) = _pair(monkeypatch)
    _fill_nan(fm)
    for s in range(3):
        start = [x.clone() for x in _state(fm, fo)]
        lf, tf = _step(fm, fo, _batch(s), max_norm)
        ls, ts = _step(sm, so, _batch(s), max_norm)
        assert torch.equal(lf, ls)
        assert _same(_state(fm, fo), _state(sm, so)), f"step {s}"
        assert not _same(_state(fm, fo), start)       # a step was taken
        assert torch.isfinite(tf) and tf > 0 and torch.isfinite(ts)
    assert _still_nan(fm)
    assert int(fo._step_dev) == int(so._step_dev) == 3


def test_active_clip_norms(monkeypatch):
    (fm, fo), (sm, so) = _pair(monkeypatch)
    ids = _batch(0)
    for m in (fm, sm):
        _backward(m, ids, loss_scale=65536.0)
        m.backward_epilogue()
    assert all(u._pending_grad is not None for u in fm.units)
    assert all(u._pending_grad is None for u in sm.units)
    # the materialized gradients of either engine, without materializing
    gf = [(u._pending_grad.float() * u._pending_gmul).cpu() for u in fm.units]
    gs = [u.grad_shard.clone().cpu() for u in sm.units]
    assert _same(gf, gs)
    assert co.norm64(gs) > 100.0
    tf, ts = fm.clip_grad_norm_(1.0), sm.clip_grad_norm_(1.0)
    ko.require("bf16_path/active_clip",
               {"norm_fast": co.check_total_norm(tf, gf),
                "norm_slow": co.check_total_norm(ts, gs)})
    assert fm._pending_grad_scale is not None
    assert float(fm._pending_grad_scale) < 1e-2
    for m, o in ((fm, fo), (sm, so)):
        before = [x.clone() for x in _state(m, o)]
        o.step()
        assert m._pending_grad_scale is None
        assert not _same(_state(m, o), before)
        o.zero_grad()
    assert all(u._pending_grad is None for u in fm.units)


def test_two_backwards_before_one_step(monkeypatch):
    (fm, fo), (sm, so) = _pair(monkeypatch)
    for m, o in ((fm, fo), (sm, so)):
        for s in range(2):
            _backward(m, _batch(s))
            m.backward_epilogue()
        # the second reduce accumulated in fp32: nothing is pending
        assert all(u._pending_grad is None for u in m.units)
        m.clip_grad_norm_(1e9)
        o.step()
        o.zero_grad()
    assert _same(_state(fm, fo), _state(sm, so))
    assert _same([u.grad_shard for u in fm.units],
                 [u.grad_shard for u in sm.units])


def test_reading_grad_shard_materializes(monkeypatch):
    (fm, fo), (sm, so) = _pair(monkeypatch)
    ids = _batch(0)
    for m in (fm, sm):
        _backward(m, ids)
        m.backward_epilogue()
    assert all(u._pending_grad is not None for u in fm.units)
    assert _same([u.grad_shard for u in fm.units],
                 [u.grad_shard for u in sm.units])
    assert all(u._pending_grad is None and u.grad_fresh for u in fm.units)
    for m, o in ((fm, fo), (sm, so)):
        m.clip_grad_norm_(1e9)
        o.step()
        o.zero_grad()
    assert _same(_state(fm, fo), _state(sm, so))


def test_graph_captured_step_matches_eager(monkeypatch):
    """The whole step under torch.cuda.graph, as the benchmark captures it:
    two warm-up steps on a side stream, capture, three replays with fresh
    inputs copied into the static buffer; against the eager engine without
    the bf16 path (which never sees the capture's own batch: a capture
    records, it does not run)."""
    (fm, fo), (sm, so) = _pair(monkeypatch)
    _fill_nan(fm)
    static = torch.zeros(B, T + 1, dtype=torch.long, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in range(2):
            static.copy_(_batch(s))
            _step(fm, fo, static, 1e9)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    static.copy_(_batch(2))
    with torch.cuda.graph(graph):
        static_loss, _ = _step(fm, fo, static, 1e9)
    for s in range(2):
        _step(sm, so, _batch(s), 1e9)
    assert _same(_state(fm, fo), _state(sm, so))
    for s in range(3, 6):
        static.copy_(_batch(s))
        graph.replay()
        loss, _ = _step(sm, so, _batch(s), 1e9)
        torch.cuda.synchronize()
        assert torch.equal(static_loss, loss)
        assert _same(_state(fm, fo), _state(sm, so)), f"replay {s}"
    assert _still_nan(fm)
    assert int(fo._step_dev) == int(so._step_dev) == 5
