"""ops.sample_logits on the CPU: the semantics of ops/sampling.py on hand
cases, through the public op (fp32) and through its reference in fp64."""

import math

import pytest
import torch

from modalities_amd import ops
from modalities_amd.ops.sampling import _sample_logits_ref

LAST_U = 1.0 - 2.0 ** -24
LN = math.log

# name: (logits, temperature, top_k, top_p, {u: expected id})
CASES = {
    # k = 3 lands inside the pair of 1s: z >= 1 keeps ids 1..4 (e2, e, e2, e);
    # id 0 is filtered out, so u = 0 must skip it
    "topk_border_ties_all_kept": (
        [0.0, 2.0, 1.0, 2.0, 1.0, -1.0], 1.0, 3, None,
        {0.0: 1, 0.3: 1, 0.45: 2, 0.6: 3, 0.9: 4, LAST_U: 4}),
    # masses .1 .2 .4 .1 .2: G = 0 for .4, .4 for the .2 class (kept whole,
    # where a cut in sorted order drops its second member), .8 for .1
    "topp_border_class_kept_whole": (
        [LN(.1), LN(.2), LN(.4), LN(.1), LN(.2)], 1.0, None, 0.5,
        {0.0: 1, 0.2: 1, 0.3: 2, 0.7: 2, 0.8: 4, LAST_U: 4}),
    # top-k keeps .4 .2 .2 (renormalised .5 .25 .25): G(.2) = .5 > .45
    "topp_over_topk_survivors": (
        [LN(.1), LN(.2), LN(.4), LN(.1), LN(.2)], 1.0, 3, 0.45,
        {0.0: 2, 0.5: 2, LAST_U: 2}),
    "greedy_lowest_index_of_maxima": (
        [1.0, 3.0, 3.0, 2.0], 0.0, 2, 0.5, {0.0: 1, 0.7: 1, LAST_U: 1}),
    "topk_at_least_v_is_off": (
        [0.0, 0.0, 0.0, 0.0], 1.0, 4, None,
        {0.0: 0, 0.3: 1, 0.6: 2, LAST_U: 3}),
    "topk_one_keeps_tied_maxima": (
        [1.0, 3.0, 3.0, 2.0], 1.0, 1, None, {0.0: 1, 0.4: 1, 0.6: 2,
                                             LAST_U: 2}),
    "v_one": ([5.0], 1.0, 50, 0.95, {0.0: 0, LAST_U: 0}),
    "v_one_greedy": ([5.0], 0.0, None, None, {0.5: 0}),
    # z = (0, 2 ln 2): masses .2 .8
    "temperature_divides": (
        [0.0, LN(2.0)], 0.5, None, None, {0.1: 0, 0.3: 1, LAST_U: 1}),
    "minus_inf_is_never_drawn": (
        [float("-inf"), 0.0, float("-inf")], 1.0, None, None,
        {0.0: 1, LAST_U: 1}),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(name):
    logits, temperature, top_k, top_p, expected = CASES[name]
    us = sorted(expected)
    x = torch.tensor([logits] * len(us), dtype=torch.float32)
    u = torch.tensor(us, dtype=torch.float32)
    out = torch.full((len(us), 1), -1, dtype=torch.long)
    assert ops.sample_logits(x, u, out, temperature, top_k, top_p) is out
    want = [expected[v] for v in us]
    assert out[:, 0].tolist() == want
    ref = _sample_logits_ref(x, u, temperature, top_k or 0, top_p or 0.0,
                             dtype=torch.float64)
    assert ref.tolist() == want


def test_strided_rows_and_flat_out_ids():
    """The [:, -1, :] view of a [B, T, V] tensor, ids into a [B] tensor."""
    x = torch.full((2, 3, 4), 9.0)
    x[:, -1] = torch.tensor([[0.0, 1.0, 5.0, 1.0], [7.0, 1.0, 5.0, 1.0]])
    out = torch.empty(2, dtype=torch.long)
    ops.sample_logits(x[:, -1, :], torch.zeros(2), out, 0.0)
    assert out.tolist() == [2, 0]


@pytest.mark.parametrize("bad", ["logits_dtype", "u_shape", "out_dtype",
                                 "logits_stride"])
def test_argument_checks(bad):
    x = torch.zeros(2, 4)
    u = torch.zeros(2)
    out = torch.zeros(2, 1, dtype=torch.long)
    if bad == "logits_dtype":
        x = x.double()
    elif bad == "u_shape":
        u = torch.zeros(3)
    elif bad == "out_dtype":
        out = out.int()
    else:
        x = torch.zeros(2, 8)[:, ::2]
    with pytest.raises((TypeError, ValueError), match="sample_logits"):
        ops.sample_logits(x, u, out, 1.0, 0, 0.0)
