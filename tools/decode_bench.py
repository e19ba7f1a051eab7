"""KV-cache decode microbench: cached incremental decoding vs full-context
re-forward on the flagship 2.7B shape (GPU).

    PYTHONPATH=. python tools/decode_bench.py [--ctx 512 2048 3968]
        [--batch 1 [16 32 ...]] [--impl {flash,split,graph}]
        [--weights {off,bf16,fp8_e4m3,mxfp4} ...] [--kv-format {bf16,fp8_e4m3}]
        [--kv-logit-diff]

--impl picks the route of the cached single-token step: `flash` is the
prefill kernel on the copied cache prefix (set_decode_attention(False)),
`split` the split-KV decode kernels launched eagerly (the default of
forward_cached), `graph` the same step captured into a hipGraph and replayed
(the default of text generation).

--weights picks the decode weights of the single-token steps: `off` (the
default) leaves the linears on F.linear / hipBLASLt, `bf16` and `fp8_e4m3`
prepare them (GPT2LLM.prepare_decode_weights) for the in-tree skinny GEMMs
(the VALU kernel up to batch 8, the MFMA kernel for batch 9..32), on the bf16
weights or on weight-only FP8; `mxfp4` prepares MXFP4 weights for the MXFP4
MFMA kernel (every batch up to 32). Several values run one after the other on
the same model, one line each. --batch takes one or more batch sizes; each
runs every --ctx.

--kv-format fp8_e4m3 decodes on an e4m3 KV cache (new_kv_cache(kv_format=));
--kv-logit-diff prints the largest |logit difference| of 64 greedy steps on
that cache against the same tokens on a bf16 cache.
"""

import argparse
import importlib
import time

import torch


def build_model():
    bench = importlib.import_module("bench")
    from modalities_amd.models.gpt2 import GPT2LLM
    cfg = bench.build_model_cfg("gpt2-2.7b")
    cfg.fused_qkv = True
    with torch.device("meta"):
        m = GPT2LLM(cfg)
    m = m.to_empty(device="cuda")
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.02)
    return m.to(torch.bfloat16).eval(), cfg


def time_cached(model, ids, iters, impl, kv_format=None):
    """ms per generated token of the cached decode loop."""
    from modalities_amd.inference.text_generation import DecodeGraph
    from modalities_amd.ops import set_decode_attention
    set_decode_attention(impl != "flash")
    B, ctx = ids.shape
    try:
        cache = model.new_kv_cache(B, max_len=ctx + 2 * iters + 8,
                                   kv_format=kv_format)
        out = model.forward_cached({"input_ids": ids}, cache)["logits"]
        graph = None
        if impl == "graph":
            graph = DecodeGraph(model, cache, "input_ids", "logits")

        def step(o):
            nxt = o[:, -1:].argmax(-1)
            if graph is not None:
                return graph.step(nxt)
            return model.forward_cached({"input_ids": nxt}, cache)["logits"]

        for _ in range(4):          # warm every launch of the timed loop
            out = step(out)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(iters):
            out = step(out)
        torch.cuda.synchronize()
        return (time.time() - t0) / iters * 1000
    finally:
        set_decode_attention(True)


def logit_error(model, ids):
    """Logits of the first single-token step after a prefill of `ids`, on the
    prepared decode weights against the same step on the bf16 weights."""
    fmt = model.decode_weight_format

    def step():
        cache = model.new_kv_cache(ids.shape[0], max_len=ids.shape[1] + 8)
        out = model.forward_cached({"input_ids": ids}, cache)["logits"]
        nxt = out[:, -1:].argmax(-1)
        return model.forward_cached({"input_ids": nxt},
                                    cache)["logits"].float()

    got = step()
    model.clear_decode_weights()
    ref = step()
    model.prepare_decode_weights(fmt)
    rel = ((got - ref).norm() / ref.norm()).item()
    same = (got.argmax(-1) == ref.argmax(-1)).float().mean().item()
    return rel, (got - ref).abs().max().item(), ref.abs().max().item(), same


def kv_logit_diff(model, ids, steps=64):
    """Largest |logit difference| over `steps` greedy tokens (chosen on the
    bf16 cache) between an FP8 and a bf16 KV cache, and the share of steps
    with the same argmax."""
    B, ctx = ids.shape
    caches = [model.new_kv_cache(B, max_len=ctx + steps + 8, kv_format=f)
              for f in (None, "fp8_e4m3")]
    outs = [model.forward_cached({"input_ids": ids}, c)["logits"][:, -1:]
            for c in caches]
    worst, top, same = 0.0, 0.0, 0
    for _ in range(steps):
        nxt = outs[0].argmax(-1)
        outs = [model.forward_cached({"input_ids": nxt}, c)["logits"].float()
                for c in caches]
        worst = max(worst, (outs[0] - outs[1]).abs().max().item())
        top = max(top, outs[0].abs().max().item())
        same += (outs[0].argmax(-1) == outs[1].argmax(-1)).float().mean().item()
    return worst, top, same / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="+", default=[512, 2048, 3968])
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--impl", choices=["flash", "split", "graph"],
                    default="split")
    ap.add_argument("--weights", nargs="+", default=["off"],
                    choices=["off", "bf16", "fp8_e4m3", "mxfp4"])
    ap.add_argument("--logit-error", action="store_true",
                    help="with --weights bf16/fp8_e4m3/mxfp4: also print the "
                         "error of a step's logits against the bf16 route")
    ap.add_argument("--kv-format", choices=["bf16", "fp8_e4m3"],
                    default="bf16")
    ap.add_argument("--kv-logit-diff", action="store_true",
                    help="print the logit difference of an FP8 against a "
                         "bf16 KV cache over 64 greedy tokens")
    ap.add_argument("--no-reforward", action="store_true",
                    help="skip the full-context re-forward comparison")
    ap.add_argument("--fused", action="store_true",
                    help="turn the fused decode step on "
                         "(ops.set_decode_fused_step): norms, SwiGLU gate and "
                         "residual adds ride on the bf16 / fp8_e4m3 GEMMs")
    args = ap.parse_args()
    if args.fused:
        from modalities_amd.ops import set_decode_fused_step
        set_decode_fused_step(True)
    model, cfg = build_model()
    for weights in args.weights:
        model.clear_decode_weights()
        if weights != "off":
            model.prepare_decode_weights(weights)
        args.weights = weights
        run(model, cfg, args)


def run(model, cfg, args):
    kv_format = None if args.kv_format == "bf16" else args.kv_format
    for batch in args.batch:
        for ctx in args.ctx:
            ids = torch.randint(0, cfg.vocab_size, (batch, ctx),
                                device="cuda")
            with torch.no_grad():
                if args.logit_error and args.weights != "off":
                    rel, mx, top, same = logit_error(model, ids)
                    print(f"ctx {ctx}: logits {args.weights} vs bf16 route: "
                          f"rel l2 {rel:.3e}, max abs {mx:.3e} (max |logit| "
                          f"{top:.3f}), same argmax {same:.2f}")
                if args.kv_logit_diff:
                    worst, top, same = kv_logit_diff(model, ids)
                    print(f"ctx {ctx}: logits fp8_e4m3 vs bf16 KV cache, 64 "
                          f"greedy tokens: max abs diff {worst:.3e} (max "
                          f"|logit| {top:.3f}), same argmax {same:.3f}")
                cached_ms = time_cached(model, ids, args.iters, args.impl,
                                        kv_format)
                if args.no_reforward:
                    print(f"ctx {ctx}: cached {cached_ms:.2f} ms/tok  "
                          f"[batch {batch}, {args.impl}, "
                          f"weights {args.weights}, kv {args.kv_format}"
                          f"{', fused' if args.fused else ''}]")
                    continue

                full = ids
                out2 = model({"input_ids": full})
                torch.cuda.synchronize()
                t0 = time.time()
                n_ref = max(4, args.iters // 4)
                for _ in range(n_ref):
                    nxt = out2["logits"][:, -1:].argmax(-1)
                    full = torch.cat([full, nxt], 1)
                    out2 = model({"input_ids": full})
                torch.cuda.synchronize()
                refwd_ms = (time.time() - t0) / n_ref * 1000
            tag = "" if (batch, args.impl, args.weights) \
                == (1, "split", "off") \
                else f"  [batch {batch}, {args.impl}, weights {args.weights}]"
            print(f"ctx {ctx}: cached {cached_ms:.1f} ms/tok  "
                  f"re-forward {refwd_ms:.1f} ms/tok  "
                  f"({refwd_ms/cached_ms:.1f}x)" + tag)


if __name__ == "__main__":
    main()
