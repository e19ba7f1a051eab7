"""Kernel-level A/B of the batch-1..32 decode GEMMs on the 2.7B shapes (GPU):

  blaslt  F.linear on the bf16 weight (hipBLASLt), what a decode step runs
          with `decode_weight_format` unset
  bf16    ops.skinny_linear on the same bf16 weight (in-tree kernel, equal
          bytes)
  e4m3    ops.skinny_linear on the weight-only FP8 copy (half the bytes)
  mfma-bf16 / mfma-e4m3
          ops.skinny_linear_mfma (matrix cores, M <= 32) on the same two
  mxfp4   ops.skinny_linear_mxfp4 (matrix cores, M <= 32) on the MXFP4 copy
          (0.53 bytes per weight)

for QKV, c_proj, packed W|V, W_2 and lm_head at M = 1, 8, 16 and 32, in one
process; the VALU kernel (bf16, e4m3) only where M <= 8. `--tilings` times
the MFMA kernel's RT x KSPLIT instantiations on the e4m3 weight instead (the
A/B behind the shipped MFMA_GEMV_RT / MFMA_GEMV_KSPLIT) and the MXFP4
kernel's RT = 1, 2, 4 (the A/B behind SKINNY_FP4_FILL_WGS).

`--fused` times, for M <= 8 on the bf16 and e4m3 weights, each decode GEMM
with its elementwise neighbours as separate launches against the one fused
launch (`skinny_linear`'s norm_weight / glu / residual): rms_norm + GEMM for
QKV and lm_head, rms_norm + GEMM + silu_mul_joint for W|V, GEMM + add for
c_proj and W_2.

A decode step streams every weight of the model once per token, so each
weight arrives cold. To time that and not a cache-resident loop, every shape
gets enough copies of its weight that one format's set exceeds `--cold-mb`
(default 768 MB, three times the 256 MB Infinity Cache) and consecutive calls
take consecutive copies. The calls of one implementation are captured into a
hipGraph, as the decode step is, and the replay is timed with device events:
the figure is time per call inside a replayed graph, launch gaps included.
`--repeats` replays alternate between the implementations; the table
gives the median and the min..max spread. GB/s counts the weight bytes only.

    PYTHONPATH=. python tools/decode_gemv_bench.py [--m 1 8 16 32]
        [--repeats 7] [--calls 64] [--cold-mb 768] [--tilings]
        [--only qkv c_proj wv w2 lm_head] [--fused]
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


def fused_ab(args):
    """The unfused launch sequence of each decode GEMM against the fused
    launch, same cold-weight graph timing as the main table."""
    from modalities_amd.ops import (quantize_weight_fp8, rms_norm,
                                    silu_mul_joint, skinny_linear)
    from modalities_amd.ops.decode_linear import SKINNY_MAX_M
    for name, (N, K) in shapes_2p7b().items():
        if args.only and name not in args.only:
            continue
        w = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
        wq, scale = quantize_weight_fp8(w)
        ncopy = max(2, -(-args.cold_mb * (1 << 20) // (N * K)))
        ncalls = max(args.calls, ncopy)
        sets = {"bf16": ([w.clone() for _ in range(ncopy)], None),
                "e4m3": ([wq.clone() for _ in range(ncopy)], scale)}
        g = (1 + 0.1 * torch.randn(K, device="cuda")).bfloat16()
        glu = name == "wv"
        for M in (m for m in args.m if m <= SKINNY_MAX_M):
            x = torch.randn(M, K, device="cuda").bfloat16()
            r = torch.randn(M, N, device="cuda").bfloat16()
            impls = {}
            for fmt, (ws, sc) in sets.items():
                if name in ("c_proj", "w2"):
                    impls[fmt] = lambda i, ws=ws, sc=sc: \
                        r + skinny_linear(x, ws[i % ncopy], sc)
                    impls[fmt + "-fused"] = lambda i, ws=ws, sc=sc: \
                        skinny_linear(x, ws[i % ncopy], sc, residual=r)
                elif glu:
                    impls[fmt] = lambda i, ws=ws, sc=sc: silu_mul_joint(
                        skinny_linear(rms_norm(x, g), ws[i % ncopy], sc))
                    impls[fmt + "-fused"] = lambda i, ws=ws, sc=sc: \
                        skinny_linear(x, ws[i % ncopy], sc, norm_weight=g,
                                      glu=True)
                else:
                    impls[fmt] = lambda i, ws=ws, sc=sc: skinny_linear(
                        rms_norm(x, g), ws[i % ncopy], sc)
                    impls[fmt + "-fused"] = lambda i, ws=ws, sc=sc: \
                        skinny_linear(x, ws[i % ncopy], sc, norm_weight=g)
            graphs = {k: capture(fn, ncalls) for k, fn in impls.items()}
            for gr, _ in graphs.values():
                replay_us(gr, ncalls)
            us = {k: [] for k in impls}
            for _ in range(args.repeats):
                for k, (gr, _) in graphs.items():
                    us[k].append(replay_us(gr, ncalls))
            line = f"{name:8s} N{N:6d} K{K:5d} M{M}:"
            med = {k: statistics.median(v) for k, v in us.items()}
            for k in impls:
                line += (f"  {k} {med[k]:7.2f} us [{min(us[k]):.2f}.."
                         f"{max(us[k]):.2f}]")
            line += "  |" + "".join(
                f" {f}/fused {med[f] / med[f + '-fused']:.2f}x" for f in sets)
            line += "  | maxdiff" + "".join(
                f" {f} {(graphs[f][1][0].float() - graphs[f + '-fused'][1][0].float()).abs().max().item():.1e}"
                for f in sets)
            print(line, flush=True)
            del graphs
        del sets
        torch.cuda.empty_cache()


def main():
    from modalities_amd.ops import (dequantize_weight_mxfp4,
                                    quantize_weight_fp8, quantize_weight_mxfp4,
                                    skinny_linear, skinny_linear_mfma,
                                    skinny_linear_mxfp4)
    from modalities_amd.ops.backend import hip_ext, require_hip
    from modalities_amd.ops.decode_linear import (SKINNY_MAX_M,
                                                  pack_mxfp4_scales)
    require_hip("decode_gemv_bench")
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 8, 16, 32])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=64,
                    help="calls per timed graph replay (at least the number "
                         "of weight copies is used)")
    ap.add_argument("--cold-mb", type=int, default=768)
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--tilings", action="store_true",
                    help="time skinny_linear_mfma's RT x KSPLIT variants on "
                         "the e4m3 weight instead of the implementations")
    ap.add_argument("--fused", action="store_true",
                    help="time each GEMM plus its norm / gate / add launches "
                         "against the fused launch (M <= 8, bf16 and e4m3)")
    args = ap.parse_args()
    torch.manual_seed(0)
    print(f"# cold set >= {args.cold_mb} MB per format; time per call inside "
          f"a replayed graph; median [min..max] of {args.repeats} replays")
    if args.fused:
        return fused_ab(args)
    for name, (N, K) in shapes_2p7b().items():
        if args.only and name not in args.only:
            continue
        w = (torch.randn(N, K, device="cuda") * 0.02).bfloat16()
        wq, scale = quantize_weight_fp8(w)
        w4, s4 = quantize_weight_mxfp4(w)
        s4 = pack_mxfp4_scales(s4)
        ncopy = max(2, -(-args.cold_mb * (1 << 20) // (N * K)))   # e4m3 bytes
        ncalls = max(args.calls, ncopy)
        wb = [w.clone() for _ in range(ncopy)]
        w8 = [wq.clone() for _ in range(ncopy)]
        # twice the copies: the MXFP4 set is as cold as the e4m3 one
        w4 = [(w4.clone(), s4.clone()) for _ in range(2 * ncopy)]
        ref4_w = dequantize_weight_mxfp4(*w4[0])
        for M in args.m:
            x = torch.randn(M, K, device="cuda").bfloat16()
            impls = {"blaslt": lambda i: F.linear(x, wb[i % ncopy])}
            if args.tilings:
                for rt in (1, 2):
                    for ks in (4, 8):
                        impls[f"rt{rt}ks{ks}"] = \
                            lambda i, rt=rt, ks=ks: hip_ext().skinny_linear_mfma(
                                x, w8[i % ncopy], scale, None, rt, ks)
                for rt in (1, 2, 4):
                    impls[f"mxfp4-rt{rt}"] = \
                        lambda i, rt=rt: hip_ext().skinny_linear_mxfp4(
                            x, *w4[i % (2 * ncopy)], None, rt)
            else:
                if M <= SKINNY_MAX_M:
                    impls["bf16"] = lambda i: skinny_linear(x, wb[i % ncopy])
                    impls["e4m3"] = lambda i: skinny_linear(x, w8[i % ncopy],
                                                            scale)
                impls["mfma-bf16"] = lambda i: skinny_linear_mfma(
                    x, wb[i % ncopy])
                impls["mfma-e4m3"] = lambda i: skinny_linear_mfma(
                    x, w8[i % ncopy], scale)
                impls["mxfp4"] = lambda i: skinny_linear_mxfp4(
                    x, *w4[i % (2 * ncopy)])
            graphs = {k: capture(fn, ncalls) for k, fn in impls.items()}
            for g, _ in graphs.values():     # warm every graph once
                replay_us(g, ncalls)
            # results must agree before a time means anything (the outputs
            # of a graph hold values only after a replay)
            ref = graphs["blaslt"][1][0].float()
            ref8 = F.linear(x, (wq.float() * scale[:, None]).bfloat16()).float()
            ref4 = F.linear(x, ref4_w).float()
            diff = {k: (graphs[k][1][0].float()
                        - (ref if k.endswith("bf16") else
                           ref4 if k.startswith("mxfp4") else ref8)).abs().max()
                    .item() for k in impls if k != "blaslt"}
            us = {k: [] for k in impls}
            for _ in range(args.repeats):    # alternate the implementations
                for k, (g, _) in graphs.items():
                    us[k].append(replay_us(g, ncalls))
            line = f"{name:8s} N{N:6d} K{K:5d} M{M}:"
            med = {}
            for k in impls:
                med[k] = statistics.median(us[k])
                nbytes = N * K * (2 if k in ("blaslt", "bf16", "mfma-bf16")
                                  else 17 / 32 if k.startswith("mxfp4") else 1)
                line += (f"  {k} {med[k]:7.2f} us [{min(us[k]):.2f}.."
                         f"{max(us[k]):.2f}] {nbytes / med[k] / 1e3:6.0f} GB/s")
            line += "  |" + "".join(
                f" blaslt/{k} {med['blaslt'] / med[k]:.2f}x"
                for k in impls if k != "blaslt")
            line += "  | maxdiff" + "".join(f" {k} {d:.1e}"
                                            for k, d in diff.items())
            print(line, flush=True)
            del graphs
        del wb, w8, w4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
