"""Kernel-level A/B of the batch-1..8 decode GEMMs on the 2.7B shapes (GPU):

  blaslt  F.linear on the bf16 weight (hipBLASLt), what a decode step runs
          with `decode_weight_format` unset
  bf16    ops.skinny_linear on the same bf16 weight (in-tree kernel, equal
          bytes)
  e4m3    ops.skinny_linear on the weight-only FP8 copy (half the bytes)

for QKV, c_proj, packed W|V, W_2 and lm_head at M = 1 and 8, in one process.

A decode step streams every weight of the model once per token, so each
weight arrives cold. To time that and not a cache-resident loop, every shape
gets enough copies of its weight that one format's set exceeds `--cold-mb`
(default 768 MB, three times the 256 MB Infinity Cache) and consecutive calls
take consecutive copies. The calls of one implementation are captured into a
hipGraph, as the decode step is, and the replay is timed with device events:
the figure is time per call inside a replayed graph, launch gaps included.
`--repeats` replays alternate between the three implementations; the table
gives the median and the min..max spread. GB/s counts the weight bytes only.

    PYTHONPATH=. python tools/decode_gemv_bench.py [--m 1 8] [--repeats 7]
        [--calls 64] [--cold-mb 768] [--only qkv c_proj wv w2 lm_head]
"""

import argparse
import importlib
import statistics

import torch
import torch.nn.functional as F


def shapes_2p7b():
    bench = importlib.import_module("bench")
    from modalities_amd.models.model import SwiGLU
    cfg = bench.build_model_cfg("gpt2-2.7b")
    C = cfg.n_embd
    kv = C // cfg.n_head_q * cfg.n_head_kv
    H = SwiGLU._get_hidden_dim(cfg.ffn_hidden)
    return {"qkv": (C + 2 * kv, C), "c_proj": (C, C), "wv": (2 * H, C),
            "w2": (C, H), "lm_head": (cfg.vocab_size, C)}


def capture(fn, ncalls):
    """A graph of fn(0), fn(1), ..., fn(ncalls - 1) on one stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(ncalls):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g):
        for i in range(ncalls):
            keep.append(fn(i))
    return g, keep


def replay_us(g, ncalls):
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    t0.record()
    g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / ncalls * 1e3


def main():
    from modalities_amd.ops import quantize_weight_fp8, skinny_linear
    from modalities_amd.ops.backend import require_hip
    require_hip("decode_gemv_bench")
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=64,
                    help="calls per timed graph replay (at least the number "
                         "of weight copies is used)")
    ap.add_argument("--cold-mb", type=int, default=768)
    ap.add_argument("--only", nargs="+", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    print(f"# cold set >= {args.cold_mb} MB per format; time per call inside "
          f"a replayed graph; median [min..max] of {args.repeats} replays")
    for name, (N, K) in shapes_2p7b().items():
        if args.only and name not in args.only:
            continue
        w = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
        wq, scale = quantize_weight_fp8(w)
        ncopy = max(2, -(-args.cold_mb * (1 << 20) // (N * K)))   # e4m3 bytes
        ncalls = max(args.calls, ncopy)
        wb = [w.clone() for _ in range(ncopy)]
        w8 = [wq.clone() for _ in range(ncopy)]
        for M in args.m:
            x = torch.randn(M, K, device="cuda").bfloat16()
            impls = {
                "blaslt": lambda i: F.linear(x, wb[i % ncopy]),
                "bf16": lambda i: skinny_linear(x, wb[i % ncopy]),
                "e4m3": lambda i: skinny_linear(x, w8[i % ncopy], scale),
            }
            graphs = {k: capture(fn, ncalls) for k, fn in impls.items()}
            for g, _ in graphs.values():     # warm every graph once
                replay_us(g, ncalls)
            # results must agree before a time means anything (the outputs
            # of a graph hold values only after a replay)
            ref = graphs["blaslt"][1][0].float()
            d_bf = (graphs["bf16"][1][0].float() - ref).abs().max().item()
            ref8 = F.linear(x, (wq.float() * scale[:, None]).bfloat16()).float()
            d_8 = (graphs["e4m3"][1][0].float() - ref8).abs().max().item()
            us = {k: [] for k in impls}
            for _ in range(args.repeats):    # alternate the implementations
                for k, (g, _) in graphs.items():
                    us[k].append(replay_us(g, ncalls))
            line = f"{name:8s} N{N:6d} K{K:5d} M{M}:"
            med = {}
            for k in impls:
                med[k] = statistics.median(us[k])
                nbytes = N * K * (1 if k == "e4m3" else 2)
                line += (f"  {k} {med[k]:7.2f} us [{min(us[k]):.2f}.."
                         f"{max(us[k]):.2f}] {nbytes / med[k] / 1e3:6.0f} GB/s")
            line += (f"  | blaslt/bf16 {med['blaslt'] / med['bf16']:.2f}x "
                     f"blaslt/e4m3 {med['blaslt'] / med['e4m3']:.2f}x "
                     f"| maxdiff bf16 {d_bf:.1e} e4m3 {d_8:.1e}")
            print(line, flush=True)
            del graphs
        del wb, w8
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
