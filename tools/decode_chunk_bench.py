"""Call-level A/B of multi-token attention over a KV cache (GPU): T new
tokens per row, already stored, against a cache of `ctx` rows in all.

  chunk  decode_attn_chunk_fwd / decode_attn_chunk_fp8_fwd, cache read in
         place (ops.decode_attention with T >= 2, few query rows)
  wide   decode_attn_wide_fwd / decode_attn_wide_fp8_fwd, the same call
         with one workgroup per 64 query rows (ops.decode_attention from
         _DECODE_WIDE_MIN_ROWS rows per kv head up)
  flash  what forward_cached does with the switch off, for the same call:
         bf16  attn_fwd on cache[:, :ctx].contiguous(), both prefix copies
               included, q_offset = ctx - T
         fp8   dequantize_kv_fp8 of the ctx - T prefix rows, torch.cat of
               the T fresh bf16 rows, then the bf16 chain

The routes alternate inside one process (`--rounds` rounds of `--iters`
calls each, device events around each batch of calls); the figure is the
median round. The cache rate is the bytes the call must move, 2 * B * ctx *
Hkv * D * 2 (bf16) or 2 * B * ctx * Hkv * (D + 4) (fp8), over the CALL time
(two launches and the workspace included), so it understates the kernel.
For kernel times run it under `rocprofv3 --kernel-trace --stats` with
`--rounds 1 --iters 20 --no-flash`.

    PYTHONPATH=. python tools/decode_chunk_bench.py [--ctx 2048 16384]
        [--batch 1 8] [--shape 32:32:80 32:8:128] [--tokens 2 4 8 16 32 64]
        [--kv-format bf16 fp8_e4m3] [--kv-chunk 0] [--wide-chunk 0]
"""

import argparse
import statistics

import torch


def timed(fn, iters):
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3      # us per call


def alternate(fns, rounds, iters):
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            us[i].append(timed(fn, iters))
    return [statistics.median(u) for u in us]


def main():
    from modalities_amd.ops import dequantize_kv_fp8, quantize_kv_fp8
    from modalities_amd.ops.backend import require_hip
    ext = require_hip("decode_chunk_bench")
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--shape", nargs="+", default=["32:32:80", "32:8:128"],
                    help="Hq:Hkv:D")
    ap.add_argument("--tokens", type=int, nargs="+",
                    default=[2, 4, 8, 16, 32, 64])
    ap.add_argument("--kv-format", nargs="+", default=["bf16", "fp8_e4m3"],
                    choices=["bf16", "fp8_e4m3"])
    ap.add_argument("--kv-chunk", type=int, default=0,
                    help="0 = the compiled default")
    ap.add_argument("--wide-chunk", type=int, default=0,
                    help="kv_chunk of the wide entries, 0 = their default")
    ap.add_argument("--no-flash", action="store_true",
                    help="skip the baseline route")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ch, wch = args.kv_chunk, args.wide_chunk
    print(f"default kv_chunk {ext.decode_attn_chunk_kv_chunk()}, wide "
          f"{ext.decode_attn_wide_kv_chunk()}")
    for shape in args.shape:
        Hq, Hkv, D = (int(x) for x in shape.split(":"))
        for B in args.batch:
            lmax = max(args.ctx)
            kc = torch.randn(B, lmax, Hkv, D, device="cuda").bfloat16()
            vc = torch.randn(B, lmax, Hkv, D, device="cuda").bfloat16()
            (kq, ks), (vq, vs) = quantize_kv_fp8(kc), quantize_kv_fp8(vc)
            for fmt in args.kv_format:
                for n in args.ctx:
                    lens = torch.full((B,), n, dtype=torch.int32,
                                      device="cuda")
                    for T in args.tokens:
                        q = torch.randn(B, T, Hq, D, device="cuda").bfloat16()
                        if fmt == "bf16":
                            nbytes = 2 * B * n * Hkv * D * 2

                            def chunk():
                                return ext.decode_attn_chunk_fwd(
                                    q, kc, vc, lens, ch)[0]

                            def wide():
                                return ext.decode_attn_wide_fwd(
                                    q, kc, vc, lens, wch)[0]

                            def flash():
                                return ext.attn_fwd(
                                    q, kc[:, :n].contiguous(),
                                    vc[:, :n].contiguous(), True, n - T)[0]
                        else:
                            nbytes = 2 * B * n * Hkv * (D + 4)
                            kf, vf = kc[:, n - T:n], vc[:, n - T:n]

                            def chunk():
                                return ext.decode_attn_chunk_fp8_fwd(
                                    q, kq, ks, vq, vs, lens, ch)[0]

                            def wide():
                                return ext.decode_attn_wide_fp8_fwd(
                                    q, kq, ks, vq, vs, lens, wch)[0]

                            def flash():
                                p = n - T
                                k = torch.cat([dequantize_kv_fp8(
                                    kq[:, :p], ks[:, :p]), kf], 1)
                                v = torch.cat([dequantize_kv_fp8(
                                    vq[:, :p], vs[:, :p]), vf], 1)
                                return ext.attn_fwd(q, k.contiguous(),
                                                    v.contiguous(), True, p)[0]
                        line = f"{fmt} Hq{Hq} Hkv{Hkv} D{D} B{B} ctx{n} T{T}:"
                        if args.no_flash:
                            us_c, us_w = alternate([chunk, wide], args.rounds,
                                                   args.iters)
                        else:
                            us_c, us_w, us_f = alternate(
                                [chunk, wide, flash], args.rounds, args.iters)
                            err = (chunk().float() - flash().float()
                                   ).abs().max().item()
                            line += (f" flash {us_f:8.1f} us | speed-up "
                                     f"{us_f / us_c:5.2f}x maxdiff {err:.1e} |")
                        werr = (chunk().float() - wide().float()
                                ).abs().max().item()
                        line += (f" chunk {us_c:7.1f} us "
                                 f"{nbytes / us_c / 1e6:6.3f} TB/s | wide "
                                 f"{us_w:7.1f} us {nbytes / us_w / 1e6:6.3f} "
                                 f"TB/s vs chunk {werr:.1e}")
                        print(line, flush=True)


if __name__ == "__main__":
    main()
