"""KV-cache decode microbench: cached incremental decoding vs full-context
re-forward on the flagship 2.7B shape (GPU).

    PYTHONPATH=. python tools/decode_bench.py [--ctx 512 2048 3968]
        [--batch 1] [--impl {flash,split,graph}]
        [--weights {off,bf16,fp8_e4m3}]

--impl picks the route of the cached single-token step: `flash` is the
prefill kernel on the copied cache prefix (set_decode_attention(False)),
`split` the split-KV decode kernels launched eagerly (the default of
forward_cached), `graph` the same step captured into a hipGraph and replayed
(the default of text generation).

--weights picks the decode weights of the single-token steps: `off` (the
default) leaves the linears on F.linear / hipBLASLt, `bf16` and `fp8_e4m3`
prepare them (GPT2LLM.prepare_decode_weights) for the in-tree skinny GEMM,
on the bf16 weights or on weight-only FP8.
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


def time_cached(model, ids, iters, impl):
    """ms per generated token of the cached decode loop."""
    from modalities_amd.inference.text_generation import DecodeGraph
    from modalities_amd.ops import set_decode_attention
    set_decode_attention(impl != "flash")
    B, ctx = ids.shape
    try:
        cache = model.new_kv_cache(B, max_len=ctx + 2 * iters + 8)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="+", default=[512, 2048, 3968])
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--impl", choices=["flash", "split", "graph"],
                    default="split")
    ap.add_argument("--weights", choices=["off", "bf16", "fp8_e4m3"],
                    default="off")
    ap.add_argument("--logit-error", action="store_true",
                    help="with --weights bf16/fp8_e4m3: also print the "
                         "error of a step's logits against the bf16 route")
    ap.add_argument("--no-reforward", action="store_true",
                    help="skip the full-context re-forward comparison")
    args = ap.parse_args()
    model, cfg = build_model()
    if args.weights != "off":
        model.prepare_decode_weights(args.weights)
    for ctx in args.ctx:
        ids = torch.randint(0, cfg.vocab_size, (args.batch, ctx),
                            device="cuda")
        with torch.no_grad():
            if args.logit_error and args.weights != "off":
                rel, mx, top, same = logit_error(model, ids)
                print(f"ctx {ctx}: logits {args.weights} vs bf16 route: "
                      f"rel l2 {rel:.3e}, max abs {mx:.3e} (max |logit| "
                      f"{top:.3f}), same argmax {same:.2f}")
            cached_ms = time_cached(model, ids, args.iters, args.impl)
            if args.no_reforward:
                print(f"ctx {ctx}: cached {cached_ms:.2f} ms/tok  "
                      f"[batch {args.batch}, {args.impl}, "
                      f"weights {args.weights}]")
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
        tag = "" if (args.batch, args.impl, args.weights) \
            == (1, "split", "off") \
            else f"  [batch {args.batch}, {args.impl}, weights {args.weights}]"
        print(f"ctx {ctx}: cached {cached_ms:.1f} ms/tok  "
              f"re-forward {refwd_ms:.1f} ms/tok  ({refwd_ms/cached_ms:.1f}x)"
              + tag)


if __name__ == "__main__":
    main()
