"""GPU tests: the workgroup order of the v2 attention kernels.

The kernels run on a 1-D grid of n_blk*H*B workgroups, id = rank*(H*B) +
b*H + h (globally heavy-first); MA_ATTN_GRID=legacy restores the
dim3(n_blk, H, B) grid. The remap is a bijection on workgroups and every
workgroup owns its output rows (no atomics), so o, lse, dq, dk and dv must be
bit-identical between the two grids. A wrong decode (h and b swapped, a block
counted from the wrong end, n_blk of the other backward kernel) computes some
row from another head's or block's data, or leaves it unwritten.

Each case first asserts that the legacy grid reproduces itself bit for bit;
an output that does not is instead held, under the default grid, to the fp64
oracle of tests/kernel_oracles.py / tests/docmask_oracles.py with that file's
own bounds.

Shapes: the smallest at which the decode can go wrong (H*B no multiple of 8,
GQA with the split dV/dK kernels, a ragged last block, a dkdv block count
that differs from the dq block count, document bounds off the 32/256
multiples, the joint-QKV backward, a single block)."""

import os

import pytest
import torch

from tests import docmask_oracles as dm
from tests import kernel_oracles as ko

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from modalities_amd.ops.backend import hip_ext
    EXT = hip_ext()
else:
    EXT = None

DEV = "cuda:0"
BF16 = torch.bfloat16
ENV = "MA_ATTN_GRID"


def _with_grid(mode, fn):
    """Run fn() with MA_ATTN_GRID = mode (None: unset, the default grid)."""
    old = os.environ.pop(ENV, None)
    if mode is not None:
        os.environ[ENV] = mode
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def _check(label, fwd, bwd, inp, make_case, check_fwd, check_bwd):
    """fwd(q, k, v) -> (o, lse); bwd(do, q, k, v, o, lse) -> (dq, dk, dv).
    make_case() builds the fp64 oracle case (only if an output of the legacy
    grid does not reproduce itself)."""
    assert EXT.get_attn_impl() == 2
    q, k, v, do = inp["q"], inp["k"], inp["v"], inp["do"]

    def run():
        o, lse = fwd(q, k, v)
        dq, dk, dv = bwd(do, q, k, v, o, lse)
        return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)

    leg_a = _with_grid("legacy", run)
    leg_b = _with_grid("legacy", run)
    new = _with_grid(None, run)
    unstable = [n for n in leg_a if not torch.equal(leg_a[n], leg_b[n])]
    print(f"GRID {label}: legacy-vs-legacy differs in {unstable or 'nothing'}")
    for n in leg_a:
        assert not torch.isnan(new[n].float()).any(), f"{label}: NaN in {n}"
        if n not in unstable:
            assert torch.equal(new[n], leg_a[n]), \
                f"{label}: {n} differs between the legacy and the linear grid"
    if unstable:
        case = make_case()
        if "o" in unstable or "lse" in unstable:
            r, _, _ = _with_grid(None, lambda: check_fwd(case))
            ko.require(label + "/fwd", r)
        which = tuple(n for n in ("dq", "dk", "dv") if n in unstable)
        if which:
            ko.require(label + "/bwd",
                       _with_grid(None, lambda: check_bwd(case, which)))


def _causal(label, B, Tq, Tkv, off, Hq, Hkv, D, fwd_fn, bwd_fn):
    inp = ko.attn_random_inputs(B, Tq, Tkv, Hq, Hkv, D, DEV, seed=Tq + D)
    fwd = lambda q, k, v: tuple(fwd_fn(q, k, v, True, off))
    bwd = lambda do, q, k, v, o, lse: tuple(
        bwd_fn(do, q, k, v, o, lse, True, off))
    _check(label, fwd, bwd, inp,
           lambda: ko.AttnCase(inp, off),
           lambda c: ko.check_attn_fwd(lambda q, k, v, _o: fwd(q, k, v), c),
           lambda c, which: ko.check_attn_bwd(
               lambda do, q, k, v, o, lse, _o: bwd(do, q, k, v, o, lse), c,
               which=which))


def test_grid_hb_not_multiple_of_8():
    # H*B = 3; 4 blocks per head
    _causal("B1_H3_T1024_D80", 1, 1024, 1024, 0, 3, 3, 80,
            EXT.attn_fwd, EXT.attn_bwd)


def test_grid_gqa_ragged_split_dkdv():
    # GQA (dkdv decodes over Hkv = 2, fwd/dq over Hq = 8), ragged last block,
    # D = 128 runs the split dV / dK kernels (128 kv rows per workgroup)
    _causal("B2_H8_2_T777_D128", 2, 777, 777, 0, 8, 2, 128,
            EXT.attn_fwd_v2, EXT.attn_bwd_v2)


def test_grid_odd_batch_and_heads():
    _causal("B3_H5_T513_D64", 3, 513, 513, 0, 5, 5, 64,
            EXT.attn_fwd, EXT.attn_bwd)


def test_grid_offset_causal():
    # 1 dq block, 3 dkdv blocks
    _causal("Tq256_Tkv768_off512_D80", 1, 256, 768, 512, 2, 2, 80,
            EXT.attn_fwd_v2, EXT.attn_bwd_v2)


def test_grid_one_block():
    _causal("B2_H3_T200_D80", 2, 200, 200, 0, 3, 3, 80,
            EXT.attn_fwd, EXT.attn_bwd)


@pytest.mark.parametrize("D", [80, 128])
def test_grid_document_masked(D):
    B, H, T = 2, 4, 1024
    start = dm.layouts_to_start([[0, 333, 777], [0, 101, 515, 900]], T, DEV)
    end = dm.start_to_end(start)
    inp = ko.attn_random_inputs(B, T, T, H, H, D, DEV, seed=T + D)
    fwd = lambda q, k, v: tuple(EXT.attn_fwd_doc(q, k, v, True, 0, start))
    bwd = lambda do, q, k, v, o, lse: tuple(
        EXT.attn_bwd_doc(do, q, k, v, o, lse, True, 0, start, end, None))
    _check(f"doc_B2_H4_T1024_D{D}", fwd, bwd, inp,
           lambda: dm.DocCase(inp, start),
           lambda c: dm.check_doc_fwd(lambda q, k, v, _s: fwd(q, k, v), c),
           lambda c, which: dm.check_doc_bwd(
               lambda do, q, k, v, o, lse, _s, _e: bwd(do, q, k, v, o, lse),
               c, which=which))


def test_grid_qkvjoint_backward():
    """attn_bwd_qkvjoint at the first shape: V read in place from the joint
    activation, dV stored into its column block of the joint gradient."""
    B, T, H, D = 1, 1024, 3, 80
    C = H * D
    inp = ko.attn_random_inputs(B, T, T, H, H, D, DEV, seed=T + D + 1)
    joint = torch.zeros(B, T, 3 * C, dtype=BF16, device=DEV)
    joint[..., 2 * C:] = inp["v"].reshape(B, T, C)
    v_view = joint[..., 2 * C:].view(B, T, H, D)
    fwd = lambda q, k, v: tuple(EXT.attn_fwd(q, k, v_view, True, 0))

    def bwd(do, q, k, v, o, lse):
        dqkv = torch.full((B, T, 3 * C), 7.0, dtype=BF16, device=DEV)
        dq, dk = EXT.attn_bwd_qkvjoint(do, q, k, v_view, o, lse, True, 0,
                                       dqkv, 2 * C)
        assert (dqkv[..., :2 * C] == 7.0).all(), "wrote outside the dv block"
        return dq, dk, dqkv[..., 2 * C:].reshape(B, T, H, D).clone()

    _check("qkvjoint_B1_H3_T1024_D80", fwd, bwd, inp,
           lambda: ko.AttnCase(inp, 0),
           lambda c: ko.check_attn_fwd(lambda q, k, v, _o: fwd(q, k, v), c),
           lambda c, which: ko.check_attn_bwd(
               lambda do, q, k, v, o, lse, _o: bwd(do, q, k, v, o, lse), c,
               which=which))
