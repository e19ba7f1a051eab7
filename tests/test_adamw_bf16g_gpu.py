"""GPU tests of the bf16-gradient / bit-packed-mask AdamW entry
(fused_adamw_devstep_bf16g) and the bf16 sum of squares
(multi_tensor_sqsum_bf16).

The AdamW entry is held to the fp32 entry fused_adamw_masked_devstep, which
has its fp64 oracle in tests/test_hip_kernels_edges_gpu.py: given
g.float() * gmul and the fp32 form of the mask, p, m, v and the bf16 copy
must be BIT-IDENTICAL (bf16 -> fp32 is exact, a 0/1 mask makes the decay
factor's product exact, and both entries instantiate one update body).  No
tolerance is involved.

The sum of squares is held to the fp64 sum of (g.float() * gmul)^2 at the
bound of test_multi_tensor_sqsum (2^-18 of the sum).  It is not compared to
the fp32 kernel bit for bit: both add block partials with float atomics.

n = 64 and 192 are single-block sizes (the smallest engine shard, and one
whose float4 count is not a power of two); 64 * (32768 + 5) is the first
multiple of 64 past one full grid of 2048 blocks x 256 threads x 4 elements,
so the grid-stride loop takes a second trip.
"""

import numpy as np
import pytest
import torch

from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SIZES = [64, 192, 64 * (32768 + 5)]
BETAS = (0.9, 0.95)
HP = dict(ko.HP, b1=BETAS[0], b2=BETAS[1])


def _mask(kind, n):
    if kind == "ones":
        return torch.ones(n)
    if kind == "zeros":
        return torch.zeros(n)
    # runs of three: the 0/1 boundaries at 3, 6, 9, ... fall inside a
    # float4 (3, 6, 9) and inside a byte (3, 6, 9, 12, 15 but not 24)
    return ((torch.arange(n) // 3) % 2 == 0).float()


def _bits(mask):
    return torch.from_numpy(np.packbits(mask.numpy().astype(bool),
                                        bitorder="little")).to(DEV)


def _bf16g(p, g16, gmul, m, v, bits, t, gs, out=None):
    step = torch.tensor(t, dtype=torch.int32, device=DEV)
    out = torch.empty(p.numel(), dtype=BF16, device=DEV) if out is None \
        else out
    EXT.fused_adamw_devstep_bf16g(p, g16, gmul, m, v, bits, step, out, gs,
                                  HP["lr"], HP["b1"], HP["b2"], HP["eps"],
                                  HP["wd"])
    return out


def _f32(p, g, m, v, mask, t, gs):
    step = torch.tensor(t, dtype=torch.int32, device=DEV)
    out = torch.empty(p.numel(), dtype=BF16, device=DEV)
    EXT.fused_adamw_masked_devstep(p, g, m, v, mask, step, out, gs, HP["lr"],
                                   HP["b1"], HP["b2"], HP["eps"], HP["wd"])
    return out


@pytest.mark.parametrize("kind", ["ones", "zeros", "runs3"])
@pytest.mark.parametrize("n", SIZES)
def test_bf16g_bit_identical_to_fp32_entry(n, kind):
    p0, g, m0, v0, _ = ko.adamw_inputs(n, DEV, seed=n % 97)
    g16 = g.to(BF16)            # g[:3] = 0, 1e-8, 1e4, rounded to bf16
    assert g16[0] == 0 and g16[1] > 0 and g16[2] > 9e3
    mask = _mask(kind, n)
    bits, mask = _bits(mask), mask.to(DEV)
    assert bits.numel() * 8 == n
    for gscale in (None, 0.0371):
        gs = None if gscale is None else torch.tensor(gscale, device=DEV)
        for gmul in (1.0, 0.125):
            for t in (1, 1000):
                ref = [x.clone() for x in (p0, m0, v0)]
                ref.append(_f32(ref[0], g16.float() * gmul, ref[1], ref[2],
                                mask, t, gs))
                got = [x.clone() for x in (p0, m0, v0)]
                got.append(_bf16g(got[0], g16, gmul, got[1], got[2], bits, t,
                                  gs))
                for name, a, b in zip(("p", "m", "v", "bf16_out"), got, ref):
                    bits_t = torch.int16 if a.dtype == BF16 else torch.int32
                    assert torch.equal(a.view(bits_t), b.view(bits_t)), \
                        f"{name} differs: n={n} mask={kind} gscale={gscale} " \
                        f"gmul={gmul} t={t}"
                assert not torch.equal(got[0], p0)


def _sq_inputs(sizes, seed=0):
    g = ko._gen(seed)
    ts = [torch.randn(s, generator=g) for s in sizes]
    for t in ts:        # as ko.check_sqsum: a skipped head or tail shows
        t[0], t[-1] = 1e4, -1e4
    return [t.to(DEV).to(BF16) for t in ts]


@pytest.mark.parametrize("gmul", [1.0, 0.125])
def test_sqsum_bf16(gmul):
    for label, sizes in (("single64", SIZES[:1]), ("single_big", SIZES[2:]),
                         ("list3", SIZES)):
        ts = _sq_inputs(sizes)
        ref = sum(((t.float() * gmul).double() ** 2).sum() for t in ts)
        got = EXT.multi_tensor_sqsum_bf16(ts, gmul)
        assert got.dtype == F32 and got.dim() == 0
        ko.require(f"sqsum_bf16/{label}/gmul{gmul}",
                   {"sqsum": ko.f32_sum_ratio(got, ref, ref)})


# -------------------------------------------------------- negative tests
# Every call below would stay in bounds even without the check it tests:
# the offending tensor is no smaller than the kernel would read.
def _args(n):
    f = lambda: torch.zeros(n, dtype=F32, device=DEV)
    return dict(p=f(), g=torch.zeros(n, dtype=BF16, device=DEV), m=f(), v=f(),
                bits=torch.zeros(n // 8, dtype=torch.uint8, device=DEV),
                out=torch.zeros(n, dtype=BF16, device=DEV))


def _call(a):
    return _bf16g(a["p"], a["g"], 1.0, a["m"], a["v"], a["bits"], 1, None,
                  out=a["out"])


def test_bf16g_rejects_bad_arguments():
    n = 64
    _call(_args(n))                                   # the base call is fine
    bad = _args(12)                                   # numel % 8 != 0
    bad["bits"] = torch.zeros(2, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        _call(bad)
    for key, tensor in (
            ("g", torch.zeros(2 * n, dtype=BF16, device=DEV)[::2]),
            ("g", torch.zeros(n, dtype=F32, device=DEV)),
            ("bits", torch.zeros(n // 8 + 1, dtype=torch.uint8, device=DEV)),
            ("bits", torch.zeros(n // 8, dtype=torch.int32, device=DEV))):
        bad = _args(n)
        bad[key] = tensor
        before = bad["p"].clone()
        with pytest.raises(RuntimeError):
            _call(bad)
        assert torch.equal(bad["p"], before)


def test_sqsum_bf16_rejects_bad_arguments():
    ok = torch.zeros(64, dtype=BF16, device=DEV)
    for bad in (torch.zeros(12, dtype=BF16, device=DEV),       # numel % 8
                torch.zeros(128, dtype=BF16, device=DEV)[::2],  # strided
                torch.zeros(64, dtype=F32, device=DEV)):        # fp32
        with pytest.raises(RuntimeError):
            EXT.multi_tensor_sqsum_bf16([ok, bad], 1.0)
