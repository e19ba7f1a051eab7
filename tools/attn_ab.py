"""A/B micro-benchmark: K1 attention v1 vs v2 on the bench shapes, and the
document-masked v2 kernels against the causal ones.

Usage (on a GPU box):  python tools/attn_ab.py [--iters 50]
Prints per-kernel times and effective TFLOP/s (causal-adjusted) for
fwd and bwd at the 2.7B bench shape (hd=128/20 heads) and the exact
reference 2.7B shape (hd=80/32 heads, v2 only).

Document layouts:  python tools/attn_ab.py --doc-layout one \\
                       --doc-layout uniform:512 --doc-layout mixed --rounds 5
times, at the reference 2.7B shape (B=2, T=4096, 32 heads, D=80), the causal
v2 kernels and the document-masked kernels alternately for --rounds rounds
and prints every round, the median, the spread (max - min) and the ratio of
visited 32x64 tiles (the least work a tile-skipping kernel can do).
Layouts: `causal` (the causal kernels alone), `one` (a single document: the cost of the mask itself),
`uniform:L` (documents of L tokens), `mixed` (a fixed uneven list, different
per batch row) or explicit starts `0,100,900`.  --ext loads another build of
the extension (A/B across commits).
"""

import argparse
import importlib.util
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))  # repo root


def flops_attn(B, T, H, D, causal=True, n_matmul=2):
    f = 2.0 * B * H * T * T * D * n_matmul
    return f / 2 if causal else f


def timeit(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


MIXED_LENGTHS = ([37, 1500, 300, 64, 900, 2, 700],
                 [1024, 5, 5, 2000, 129, 257])


def doc_layout_starts(spec, B, T):
    """-> one sorted list of document starts per batch row."""
    if spec == "one":
        return [[0]] * B
    if spec.startswith("uniform:"):
        L = int(spec.split(":")[1])
        return [list(range(0, T, L))] * B
    if spec == "mixed":
        rows = []
        for b in range(B):
            s, out = 0, []
            for n in MIXED_LENGTHS[b % len(MIXED_LENGTHS)]:
                if s >= T:
                    break
                out.append(s)
                s += n
            if s < T:
                out.append(s)
            rows.append(out)
        return rows
    starts = sorted(set(int(x) for x in spec.split(",")))
    if not starts or starts[0] != 0 or starts[-1] >= T:
        raise ValueError(f"bad --doc-layout {spec!r}")
    return [starts] * B


def starts_to_doc_start(rows, T, device):
    out = torch.zeros(len(rows), T, dtype=torch.int32)
    for b, starts in enumerate(rows):
        for s in starts:
            out[b, s:] = s
    return out.to(device).contiguous()


def tile_ratio(doc_start, qblk=32, kvblk=64):
    """(visited 32x64 tiles with the mask) / (visited under plain causal),
    and the same ratio of exact areas."""
    ds = doc_start.cpu()
    B, T = ds.shape
    doc = causal = 0
    for b in range(B):
        for q0 in range(0, T, qblk):
            q1 = min(q0 + qblk, T) - 1
            causal += q1 // kvblk + 1
            doc += q1 // kvblk - int(ds[b, q0]) // kvblk + 1
    i = torch.arange(T)[None]
    area = (i - ds + 1).sum().item() / (i + 1).expand(B, T).sum().item()
    return doc / causal, area


def load_ext(path):
    if path is None:
        from modalities_amd.ops.backend import hip_ext
        return hip_ext()
    spec = importlib.util.spec_from_file_location("_hip_ops", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_doc_layouts(ext, args, dev):
    from modalities_amd.ops.attention import document_ends
    B, T, Hq, Hkv, D = 2, 4096, 32, 32, 80
    torch.manual_seed(0)
    q = torch.randn(B, T, Hq, D, device=dev).bfloat16()
    k = torch.randn(B, T, Hkv, D, device=dev).bfloat16()
    v = torch.randn(B, T, Hkv, D, device=dev).bfloat16()
    do = torch.randn(B, T, Hq, D, device=dev).bfloat16()
    print(f"== doc layouts: B{B} T{T} Hq{Hq} Hkv{Hkv} D{D}, "
          f"{args.rounds} rounds x {args.iters} iters, alternating")
    variants = [("causal", None, None)]
    for spec in args.doc_layout:
        if spec == "causal":      # the causal kernels alone (e.g. with --ext)
            continue
        ds = starts_to_doc_start(doc_layout_starts(spec, B, T), T, dev)
        variants.append((spec, ds, document_ends(ds)))
        tr, ar = tile_ratio(ds)
        print(f"  layout {spec}: tile ratio {tr:.4f} (ideal speedup "
              f"{1 / tr:.2f}x), exact area ratio {ar:.4f}")
    times = {n: ([], []) for n, _, _ in variants}
    saved = {}
    for _ in range(args.rounds):
        for name, ds, de in variants:
            if ds is None:
                fwd = lambda: ext.attn_fwd_v2(q, k, v, True, 0)
                o, lse = fwd()
                bwd = lambda: ext.attn_bwd_v2(do, q, k, v, o, lse, True, 0)
            else:
                fwd = lambda: ext.attn_fwd_doc_v2(q, k, v, True, 0, ds)
                o, lse = fwd()
                bwd = lambda: ext.attn_bwd_doc_v2(do, q, k, v, o, lse, True,
                                                  0, ds, de)
            saved.setdefault(name, (o, *bwd()))
            times[name][0].append(timeit(fwd, args.iters))
            times[name][1].append(timeit(bwd, args.iters))
    base = None
    for name, _, _ in variants:
        tf, tb = times[name]
        mf, mb = statistics.median(tf), statistics.median(tb)
        if base is None:
            base = (mf, mb)
        print(f"  {name:>14}: fwd {mf:7.3f} ms (spread {max(tf) - min(tf):.3f})"
              f"  bwd {mb:7.3f} ms (spread {max(tb) - min(tb):.3f})"
              f"  fwd+bwd {mf + mb:7.3f} ms"
              f"  vs causal: fwd {base[0] / mf:5.2f}x  bwd {base[1] / mb:5.2f}x"
              f"  fwd+bwd {(base[0] + base[1]) / (mf + mb):5.2f}x")
        print("    rounds fwd: " + " ".join(f"{t:.3f}" for t in tf)
              + " | bwd: " + " ".join(f"{t:.3f}" for t in tb))
    if "one" in saved:
        for i, tag in enumerate(("o", "dq", "dk", "dv")):
            same = torch.equal(saved["one"][i], saved["causal"][i])
            print(f"  one-document {tag} bit-identical to causal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--doc-layout", action="append", default=[],
                    help="one | uniform:L | mixed | s0,s1,... (repeatable)")
    ap.add_argument("--rounds", type=int, default=5,
                    help="alternating measurement rounds per layout")
    ap.add_argument("--ext", default=None,
                    help="path to another build of the op extension")
    args = ap.parse_args()

    ext = load_ext(args.ext)
    dev = "cuda"
    if args.doc_layout:
        run_doc_layouts(ext, args, dev)
        print("done")
        return 0

    shapes = [
        ("bench-2.7B (hd128)", 2, 4096, 20, 20, 128, (1, 2)),
        ("ref-2.7B (hd80)", 2, 4096, 32, 32, 80, (2,)),
        ("8B-class (hd128 gqa)", 1, 8192, 32, 8, 128, (1, 2)),
    ]
    for name, B, T, Hq, Hkv, D, impls in shapes:
        torch.manual_seed(0)
        q = torch.randn(B, T, Hq, D, device=dev).bfloat16()
        k = torch.randn(B, T, Hkv, D, device=dev).bfloat16()
        v = torch.randn(B, T, Hkv, D, device=dev).bfloat16()
        do = torch.randn(B, T, Hq, D, device=dev).bfloat16()
        print(f"== {name}: B{B} T{T} Hq{Hq} Hkv{Hkv} D{D}")
        outs = {}
        for impl in impls:
            fwd = ext.attn_fwd_v1 if impl == 1 else ext.attn_fwd_v2
            bwd = ext.attn_bwd_v1 if impl == 1 else ext.attn_bwd_v2
            o, lse = fwd(q, k, v, True, 0)
            dq, dk, dv = bwd(do, q, k, v, o, lse, True, 0)
            outs[impl] = (o, dq, dk, dv)
            tf = timeit(lambda: fwd(q, k, v, True, 0), args.iters)
            tb = timeit(lambda: bwd(do, q, k, v, o, lse, True, 0), args.iters)
            ffw = flops_attn(B, T, Hq, D, n_matmul=2) / (tf * 1e-3) / 1e12
            fbw = flops_attn(B, T, Hq, D, n_matmul=5) / (tb * 1e-3) / 1e12
            print(f"  v{impl}: fwd {tf:7.3f} ms ({ffw:6.1f} TF/s eff)   "
                  f"bwd {tb:7.3f} ms ({fbw:6.1f} TF/s eff)")
        if len(outs) == 2:
            for i, tag in enumerate(("o", "dq", "dk", "dv")):
                a, b = outs[1][i].float(), outs[2][i].float()
                md = (a - b).abs().max().item()
                print(f"  v1-v2 max|d{tag}| = {md:.4e}")
    print("done")


if __name__ == "__main__":
    sys.exit(main())
