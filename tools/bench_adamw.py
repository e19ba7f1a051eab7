"""AdamW devstep kernel micro-benchmark: the fp32-gradient / fp32-mask entry
(34 B/elem) next to the bf16-gradient / bit-packed-mask entry (28.125
B/elem), at 320M elements."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from modalities_amd.ops.adamw import pack_wd_bits
from modalities_amd.ops.backend import hip_ext

n = 320_000_000
p0 = torch.randn(n, device="cuda")
g0 = torch.randn(n, device="cuda")
m0 = torch.zeros(n, device="cuda")
v0 = torch.zeros(n, device="cuda")
mask = torch.ones(n, device="cuda")
step = torch.tensor(3, dtype=torch.int32, device="cuda")
out = torch.empty(n, device="cuda", dtype=torch.bfloat16)
g16 = g0.to(torch.bfloat16)
bits = pack_wd_bits(mask)


def call_f32():
    hip_ext().fused_adamw_masked_devstep(p0, g0, m0, v0, mask, step, out,
                                         None, 3e-4, .9, .95, 1e-8, .1)


def call_bf16g():
    hip_ext().fused_adamw_devstep_bf16g(p0, g16, 1.0, m0, v0, bits, step, out,
                                        None, 3e-4, .9, .95, 1e-8, .1)


def time_ms(call, iters=20):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


for name, call, bpe in (("fp32 grad, fp32 mask", call_f32, 34.0),
                        ("bf16 grad, packed mask", call_bf16g, 28.125)):
    ms = time_ms(call)
    print(f"{name}: {ms:.3f} ms  {bpe} B/elem  "
          f"({n * bpe / 1e9 / (ms / 1e3):.0f} GB/s)")
