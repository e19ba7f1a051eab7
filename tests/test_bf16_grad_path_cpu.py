"""CPU tests around the engine's bf16-gradient path: on the CPU the path is
never taken, `grad_shard` behaves as the plain fp32 attribute it used to be,
and the bit-packed decay mask has numpy.packbits' little-endian layout."""

import numpy as np
import torch

from modalities_amd.ops.adamw import pack_wd_bits


def _cpu_engine():
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    torch.manual_seed(0)
    cfg = GPT2LLMConfig(vocab_size=64, n_layer=1, n_head_q=2, n_head_kv=1,
                        n_embd=64, ffn_hidden=128, sequence_length=32)
    model = XGMIShardedModel.from_transformer(
        GPT2LLM(cfg), torch.device("cpu"), blocks_per_unit=1,
        param_dtype=torch.float32, rank=0, world_size=1)
    return model, get_adam_w(model, lr=1e-3, weight_decay=0.1)


def test_grad_shard_written_by_hand_reads_back():
    model, opt = _cpu_engine()
    assert not any(u.keep_bf16_grads for u in model.units)
    written = []
    for i, u in enumerate(model.units):
        g = torch.randn(u.grad_shard.numel(),
                        generator=torch.Generator().manual_seed(i))
        u.grad_shard.copy_(g)
        u.grad_fresh = True
        written.append(g)
    for u, g in zip(model.units, written):
        assert u._pending_grad is None
        assert torch.equal(u.grad_shard, g)
        assert u.grad_shard is u.grad_shard        # one persistent buffer
    before = [u.master_shard.clone() for u in model.units]
    opt.step()                                     # and the optimizer uses it
    assert all(not torch.equal(u.master_shard, b)
               for u, b in zip(model.units, before))
    # assigning a tensor replaces the buffer, as with a plain attribute
    u = model.units[0]
    new = torch.zeros_like(written[0])
    u.grad_shard = new
    assert u.grad_shard is new


def test_backward_then_zero_grad_leaves_nothing_pending():
    model, opt = _cpu_engine()
    ids = torch.randint(0, 64, (2, 33),
                        generator=torch.Generator().manual_seed(1))
    out = model({"input_ids": ids[:, :-1]})
    torch.nn.functional.cross_entropy(
        out["logits"].reshape(-1, 64).float(), ids[:, 1:].reshape(-1)).backward()
    model.backward_epilogue()
    # the CPU engine materializes at reduce time
    assert all(u.grad_fresh and u._pending_grad is None for u in model.units)
    assert all(u.grad_shard.abs().sum() > 0 for u in model.units)
    # a pending tensor, wherever it came from, does not survive zero_grad
    for u in model.units:
        u._pending_grad = torch.ones(u.grad_shard.numel())
    model.zero_grad_shards()
    assert all(not u.grad_fresh and u._pending_grad is None
               for u in model.units)


def test_pending_gradient_materializes_on_read():
    """The property's contract without a GPU: value = float(pending) * gmul,
    written into the persistent buffer, then dropped."""
    model, _ = _cpu_engine()
    u = model.units[0]
    buf = u.grad_shard
    g = torch.randn(buf.numel(), generator=torch.Generator().manual_seed(3)
                    ).to(torch.bfloat16)
    u._pending_grad, u._pending_gmul = g, 0.125
    got = u.grad_shard
    assert got is buf and u._pending_grad is None
    assert torch.equal(got, g.float() * 0.125)


def test_pack_wd_bits_matches_numpy_little_endian():
    g = torch.Generator().manual_seed(0)
    mask = (torch.rand(192, generator=g) < 0.5).float()
    mask[:8] = torch.tensor([1., 0, 0, 0, 0, 0, 0, 0])     # byte 0 = 1
    mask[8:16] = torch.tensor([0., 0, 0, 0, 0, 0, 0, 1])   # byte 1 = 128
    bits = pack_wd_bits(mask)
    assert bits.dtype == torch.uint8 and bits.numel() == 24
    assert bits[0] == 1 and bits[1] == 128
    ref = np.packbits(mask.numpy().astype(bool), bitorder="little")
    assert np.array_equal(bits.numpy(), ref)
    assert pack_wd_bits(torch.ones(64)).tolist() == [255] * 8
    assert pack_wd_bits(torch.zeros(64)).tolist() == [0] * 8


def test_pack_wd_bits_refuses_a_fractional_mask():
    mask = torch.ones(64)
    mask[5] = 0.37
    assert pack_wd_bits(mask) is None
    mask[5] = float("nan")
    assert pack_wd_bits(mask) is None


def test_optimizer_rebuilds_bits_when_the_mask_is_written():
    model, opt = _cpu_engine()
    u = model.units[0]
    first = opt._wd_bits_for(u)
    assert opt._wd_bits_for(u) is first                    # cached
    assert np.array_equal(
        first.numpy(), np.packbits(u.wd_mask_shard.numpy().astype(bool),
                                   bitorder="little"))
    flip = int(u.wd_mask_shard[0] == 0)
    u.wd_mask_shard[0] = float(flip)                       # in-place write
    second = opt._wd_bits_for(u)
    assert second is not first and (int(second[0]) & 1) == flip
    u.wd_mask_shard[1] = 0.5                               # no longer 0/1
    assert opt._wd_bits_for(u) is None
