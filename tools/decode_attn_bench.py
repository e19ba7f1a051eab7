"""Kernel-level A/B of single-token attention over a KV cache (GPU):

  split  decode_attn_fwd (partial + combine launches), cache read in place
  flash  what forward_cached did before: the cache prefix copied
         (.contiguous() of cache[:, :n]; a no-op view at batch 1) and sent
         through attn_fwd with Tq = 1, q_offset = n - 1

at the same shapes. Times come from device events around `--iters` calls
after a warm-up; the K/V rate is the bytes the algorithm needs
(2 * B * n * Hkv * D * 2) over that time.

    PYTHONPATH=. python tools/decode_attn_bench.py [--ctx 512 2048 3968]
        [--batch 1 8] [--shape 32:32:80 32:8:128] [--kv-chunk 0 128 512]
"""

import argparse

import torch


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3      # us per call


def main():
    from modalities_amd.ops.backend import require_hip
    ext = require_hip("decode_attn_bench")
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, nargs="+", default=[512, 2048, 3968])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--shape", nargs="+", default=["32:32:80", "32:8:128"],
                    help="Hq:Hkv:D")
    ap.add_argument("--kv-chunk", type=int, nargs="+", default=[0],
                    help="0 = the compiled default")
    ap.add_argument("--lmax", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    print(f"default kv_chunk {ext.decode_attn_kv_chunk()}")
    for shape in args.shape:
        Hq, Hkv, D = (int(x) for x in shape.split(":"))
        for B in args.batch:
            q = torch.randn(B, 1, Hq, D, device="cuda").bfloat16()
            kc = torch.randn(B, args.lmax, Hkv, D, device="cuda").bfloat16()
            vc = torch.randn(B, args.lmax, Hkv, D, device="cuda").bfloat16()
            for n in args.ctx:
                lens = torch.full((B,), n, dtype=torch.int32, device="cuda")
                kv_bytes = 2 * B * n * Hkv * D * 2

                def flash():
                    return ext.attn_fwd(q, kc[:, :n].contiguous(),
                                        vc[:, :n].contiguous(), True, n - 1)

                us_f = timed(flash, args.iters)
                line = (f"Hq{Hq} Hkv{Hkv} D{D} B{B} ctx{n}: flash "
                        f"{us_f:7.1f} us {kv_bytes / us_f / 1e6:7.3f} TB/s |")
                o_f = flash()[0]
                for ch in args.kv_chunk:
                    us_s = timed(lambda: ext.decode_attn_fwd(q, kc, vc, lens,
                                                             ch), args.iters)
                    o_s = ext.decode_attn_fwd(q, kc, vc, lens, ch)[0]
                    err = (o_s.float() - o_f.float()).abs().max().item()
                    line += (f" split[{ch}] {us_s:6.1f} us "
                             f"{kv_bytes / us_s / 1e6:6.3f} TB/s "
                             f"({us_f / us_s:4.1f}x, maxdiff {err:.1e}) |")
                print(line, flush=True)


if __name__ == "__main__":
    main()
