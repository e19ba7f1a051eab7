"""LayerNorm micro-benchmark: the HIP op (modalities_amd.ops.layer_norm)
against torch.nn.functional.layer_norm on the same device in the same run.

bf16, forward and forward+backward (torch.autograd.grad, so no gradient
accumulation kernels are timed).  The two implementations alternate inside
every round; the inputs (x, dy) rotate over more than 1 GiB of buffer sets,
so no pass finds its input rows in the 256 MiB Infinity Cache.  The outputs
come from the caching allocator and may be written to recently used memory,
for both implementations alike.  GB/s is the bytes a pass must
move (fwd: read x, write y = 4NH; fwd+bwd: fwd + read dy, x, write dx =
10NH; plus the fp32 statistics) over the measured time -- an achieved rate,
not a share of any peak.

Usage: python tools/layernorm_bench.py [--out FILE.md]
"""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch
import torch.nn.functional as F

from modalities_amd.ops import layer_norm

SHAPES = [(8192, 2560), (8192, 4096), (65536, 80)]
ROUNDS = 5
WINDOW_MS = 1000.0


def bytes_moved(N, H, bwd):
    fwd = 4 * N * H + 8 * N + 4 * H
    return fwd + (6 * N * H + 8 * N + 2 * H + 8 * H if bwd else 0)


def hip_op(x, w, b):
    return layer_norm(x, w, b, 1e-5)


def torch_op(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def make_sets(N, H):
    per_set = 4 * N * H            # x, dy in bf16 (the rotating inputs)
    nset = max(2, -(-(1 << 30) // per_set))
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda *s: torch.randn(*s, device="cuda", generator=g).bfloat16()
    return [(mk(N, H).requires_grad_(True), mk(N, H)) for _ in range(nset)]


def timed(fn, sets, w, b, bwd, iters):
    def one(i):
        x, dy = sets[i % len(sets)]
        if bwd:
            torch.autograd.grad(fn(x, w, b), (x, w, b), dy)
        else:
            with torch.no_grad():
                fn(x, w, b)
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for i in range(iters):
        one(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters       # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "layernorm_bench needs a GPU"
    rows = []
    for N, H in SHAPES:
        sets = make_sets(N, H)
        w = (torch.randn(H, device="cuda") * 0.1 + 1).bfloat16().requires_grad_(True)
        b = (torch.randn(H, device="cuda") * 0.1).bfloat16().requires_grad_(True)
        for bwd in (False, True):
            # warm-up each implementation, then size the timed window
            iters = {}
            for name, fn in (("hip", hip_op), ("torch", torch_op)):
                timed(fn, sets, w, b, bwd, 3)
                ms = timed(fn, sets, w, b, bwd, 10)
                iters[name] = max(10, int(WINDOW_MS / ms))
            t = {"hip": [], "torch": []}
            for _ in range(ROUNDS):        # alternate the two in each round
                for name, fn in (("hip", hip_op), ("torch", torch_op)):
                    t[name].append(timed(fn, sets, w, b, bwd, iters[name]))
            nbytes = bytes_moved(N, H, bwd)
            med = {k: statistics.median(v) for k, v in t.items()}
            rows.append((N, H, "fwd+bwd" if bwd else "fwd", nbytes, med,
                         {k: (min(v), max(v)) for k, v in t.items()}))
    lines = ["| shape | pass | MB moved | HIP us (min-max) | HIP GB/s | "
             "torch us (min-max) | torch GB/s | HIP / torch time |",
             "|---|---|---|---|---|---|---|---|"]
    for N, H, p, nb, med, rng in rows:
        gb = {k: nb / 1e9 / (v / 1e3) for k, v in med.items()}
        lines.append(
            f"| [{N}, {H}] | {p} | {nb / 1e6:.1f} | "
            f"{med['hip'] * 1e3:.1f} ({rng['hip'][0] * 1e3:.1f}-{rng['hip'][1] * 1e3:.1f}) | "
            f"{gb['hip']:.0f} | "
            f"{med['torch'] * 1e3:.1f} ({rng['torch'][0] * 1e3:.1f}-{rng['torch'][1] * 1e3:.1f}) | "
            f"{gb['torch']:.0f} | {med['hip'] / med['torch']:.2f} |")
    table = "\n".join(lines)
    print(table)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(table + "\n")


if __name__ == "__main__":
    main()
