"""The fused options of `skinny_linear` and the fused step on the CPU."""

import os
import subprocess
import sys

import pytest
import torch

from tests import kernel_oracles as ko
from tests.test_decode_gemv_fused_gpu import (OPTIONS, fused_case,
                                              fused_reference)


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "bf16"])
@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("K", [16, 1040, 2560])
def test_fused_cpu_route_against_fp64(fmt, opt, K):
    from modalities_amd.ops import skinny_linear
    worst = {}
    for M in (1, 3, 8):
        x, w, sc, b, g, r, glu = fused_case(M, 17, K, fmt, OPTIONS[opt],
                                            K + M, "cpu")
        x[M - 1] *= 1e-3
        for eps in (1e-6, 1e-2):
            y = skinny_linear(x, w, sc, b, norm_weight=g, norm_eps=eps,
                              residual=r, glu=glu)
            assert y.dtype == torch.bfloat16 and tuple(y.shape) == (M, 17)
            ref, S = fused_reference(x, w, sc, b, g, eps, r, glu)
            worst[f"M{M}eps{eps:g}"] = ko.single_rounding_ratio(y, ref, S)
    ko.require(f"skinny_linear fused cpu {opt} {fmt} K{K}", worst)


def test_fused_argument_errors():
    from modalities_amd.ops import skinny_linear as sl
    x, w, sc, b, g, r, _ = fused_case(2, 8, 32, "fp8_e4m3",
                                      (True, True, False), 5, "cpu")
    for err, match, kw in [
            (ValueError, "norm_weight", dict(norm_weight=g[:16])),
            (ValueError, "norm_weight", dict(norm_weight=g.repeat(2)[::2])),
            (TypeError, "norm_weight", dict(norm_weight=g.float())),
            (ValueError, "residual", dict(residual=r[:, :4])),
            (ValueError, "residual", dict(residual=r, glu=True)),  # N_out 4
            (TypeError, "residual", dict(residual=r.float())),
            (ValueError, "residual is on", dict(residual=r.to("meta")))]:
        with pytest.raises(err, match=match):
            sl(x, w, sc, b, **kw)
    with pytest.raises(ValueError, match="even N"):
        sl(x, w[:7].contiguous(), sc[:7].contiguous(), b[:7].contiguous(),
           glu=True)


def test_fused_step_switch(monkeypatch):
    from modalities_amd import ops
    monkeypatch.setattr(ops.decode_linear, "_FUSED_STEP", False)
    for on in (True, False):
        ops.set_decode_fused_step(on)
        assert ops.decode_fused_step() is on
    with pytest.raises(ValueError, match="bool"):
        ops.set_decode_fused_step(1)
    code = "from modalities_amd import ops; print(ops.decode_fused_step())"
    for val, want in (("1", "True"), ("yes", None)):
        env = {**os.environ, "MA_DECODE_FUSED_STEP": val}
        p = subprocess.run([sys.executable, "-c", code], capture_output=True,
                           text=True, env=env)
        if want is None:
            assert p.returncode != 0 and "MA_DECODE_FUSED_STEP" in p.stderr
        else:
            assert p.stdout.strip() == want, p.stderr


@pytest.mark.parametrize("variant", [
    dict(), dict(fused_qkv=False, activation_type="gelu", bias=True),
    dict(packed_swiglu=False)])
def test_cpu_model_decodes_with_the_switch_on(variant, monkeypatch):
    from modalities_amd.models.gpt2 import GPT2LLM, GPT2LLMConfig
    from modalities_amd.ops import decode_linear as dl
    torch.manual_seed(3)
    cfg = {**dict(vocab_size=128, n_layer=2, n_embd=64, ffn_hidden=128,
                  n_head_q=4, n_head_kv=2, fused_qkv=True, sequence_length=32,
                  seed=7, dropout=0.0), **variant}
    model = GPT2LLM(GPT2LLMConfig(**cfg)).to(torch.bfloat16).eval()
    model.prepare_decode_weights("bf16")
    prompt = torch.randint(0, 128, (2, 5),
                           generator=torch.Generator().manual_seed(9))
    fused = []
    real = dl.skinny_linear
    monkeypatch.setattr(dl, "skinny_linear", lambda *a, **k: fused.append(
        bool(k)) or real(*a, **k))
    logits = {}
    for on in (False, True):
        monkeypatch.setattr(dl, "_FUSED_STEP", on)
        cache = model.new_kv_cache(2, max_len=16)
        model.forward_cached({"input_ids": prompt}, cache)
        logits[on] = torch.cat([model.forward_cached(
            {"input_ids": (prompt[:, :1] + i) % 128}, cache)["logits"]
            for i in range(4)], 1)
    n = 4 * len(model._decode_linears())
    assert fused[:n] == [False] * n and fused[n:] == [True] * n
    torch.testing.assert_close(logits[True].float(), logits[False].float(),
                               rtol=2e-2, atol=2e-2)
