"""Sampler microbench on the flagship 2.7B shape (GPU): time per generated
token of TextInferenceComponent.generate_tokens with device_sampling off and
on, and the sample_logits kernel on its own.

    PYTHONPATH=. python tools/sampling_bench.py [--tokens 256] [--repeats 3]
        [--weights {off,bf16,fp8_e4m3}] [--kernel-only]

`--kernel-only` launches ops.sample_logits per shape (V 50304 / 50257, bf16 /
fp32, batch 1 / 32; greedy, temperature only, server defaults) and prints
device-event times; run it under `rocprofv3 --kernel-trace --stats` for the
kernel's own time.
"""

import argparse
import time

import torch

SERVER = dict(temperature=0.8, top_k=50, top_p=0.95)
GREEDY = dict(temperature=0.0, top_k=None, top_p=None)


class ByteTokenizer:
    """Ids are bytes; no eod, so a run always generates its full length."""

    def tokenize(self, text):
        return list(text.encode())

    def decode(self, ids):
        return " ".join(map(str, ids))

    def get_token_id(self, token):
        raise KeyError(token)


def time_generate(component_cls, model, tokens, sampling, **kw):
    """ms per generated token, prompt of 16 tokens, decode graph on."""
    comp = component_cls(model, ByteTokenizer(), "{text}",
                         sequence_length=16 + tokens,
                         device=torch.device("cuda"), **sampling, **kw)
    comp.generate_tokens("x" * 16)            # warm-up: every launch, capture
    torch.cuda.synchronize()
    t0 = time.time()
    comp.generate_tokens("x" * 16)
    torch.cuda.synchronize()
    return (time.time() - t0) / tokens * 1000


def time_kernel(iters=200):
    from modalities_amd import ops
    for V in (50304, 50257):
        for dtype in (torch.bfloat16, torch.float32):
            for B in (1, 32):
                x = (torch.randn(B, V, device="cuda") * 1.5).to(dtype)
                u = torch.rand(B, device="cuda")
                out = torch.empty(B, 1, dtype=torch.long, device="cuda")
                for name, args in (("greedy", (0.0, 0, 0.0)),
                                   ("temperature", (1.0, 0, 0.0)),
                                   ("server", (0.8, 50, 0.95)),
                                   ("top_p", (1.0, 0, 0.95))):
                    for _ in range(3):
                        ops.sample_logits(x, u, out, *args)
                    beg, end = (torch.cuda.Event(enable_timing=True)
                                for _ in range(2))
                    beg.record()
                    for _ in range(iters):
                        ops.sample_logits(x, u, out, *args)
                    end.record()
                    torch.cuda.synchronize()
                    print(f"sample_logits V {V} {str(dtype)[6:]} B {B} "
                          f"{name}: {beg.elapsed_time(end) / iters * 1000:.1f}"
                          f" us per launch (back to back)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--weights", choices=["off", "bf16", "fp8_e4m3"],
                    default="fp8_e4m3")
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if args.kernel_only:
        time_kernel()
        return
    from modalities_amd.inference.text_generation import \
        TextInferenceComponent
    from tools.decode_bench import build_model
    model, _ = build_model()
    fmt = None if args.weights == "off" else args.weights
    for r in range(args.repeats):             # alternate the variants
        for name, sampling in (("server", SERVER), ("greedy", GREEDY)):
            for on in (False, True):
                ms = time_generate(TextInferenceComponent, model, args.tokens,
                                   sampling, decode_weight_format=fmt,
                                   device_sampling=on)
                print(f"repeat {r}: {name} device_sampling={on}: {ms:.3f} "
                      f"ms/token [batch 1, weights {args.weights}]",
                      flush=True)


if __name__ == "__main__":
    main()
