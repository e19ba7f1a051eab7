"""ops.sample_logits on the GPU (csrc/sample_logits.hip) against an fp64
reference written here in plain torch, and device_sampling through the
decode graph of the tiny model.

Acceptance per row (token t drawn with u), tol = 2^-16 of the survivors'
mass: t survives the exact top-k threshold; G(t) <= top_p + tol, G the mass
strictly above t's value; and with c the reference's normalised inclusive
prefix sum over its own kept set, c[t-1] - s <= u <= c[t] + s, where
s = (tol + 2 m_amb) / c_last and m_amb is the mass of the value classes with
|G - top_p| <= tol (asserted <= 1e-3). Greedy, u = 0 and the largest u must
match the reference's token exactly whenever m_amb = 0.

tol: exp2(z log2e - m) in fp32 carries an argument error of about 2^-24
relative; mass-weighted it sums to at most about log2(V) 2^-23 ~ 2e-6, and
fixed-order summation adds a few ulps; 2^-16 leaves about 8x over that."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 2.0 ** -16
B = 32
LAST_U = 1.0 - 2.0 ** -24
VOCABS = (1, 7, 1000, 1025, 50257, 50304)
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
PARAMS = {"greedy": (0.0, 0, 0.0), "plain": (1.0, 0, 0.0),
          "server": (1.0, 50, 0.95), "t07_p09": (0.7, 0, 0.9),
          "p095": (1.0, 0, 0.95)}


@functools.lru_cache(maxsize=None)
def _logits(V, dtype):
    g = torch.Generator().manual_seed(1000 + V)
    x = torch.randn(V, generator=g) * 1.5
    n = min(40, V)
    where = torch.randperm(V, generator=g)[:n]
    x[where] += 8 + torch.randn(n, generator=g)
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def _u():
    g = torch.Generator().manual_seed(77)
    return torch.cat([torch.tensor([0.0, LAST_U]),
                      torch.rand(B - 2, generator=g)]).float()


class Reference:
    """fp64 semantics of one row of stored logits x (any float dtype)."""

    def __init__(self, x, temperature, top_k, top_p):
        x = x.detach().double().cpu()
        V = x.numel()
        self.greedy = temperature <= 0
        self.argmax = int((x == x.max()).nonzero()[0])
        if self.greedy:
            return
        z = x / temperature
        self.survives = torch.ones(V, dtype=torch.bool)
        if 0 < top_k < V:
            self.survives = z >= torch.topk(z, top_k).values[-1]
        pr = torch.softmax(z.masked_fill(~self.survives, float("-inf")), 0)
        self.top_p = top_p if 0.0 < top_p < 1.0 else None
        self.m_amb = 0.0
        keep = self.survives
        if self.top_p is not None:
            vals, inv = torch.unique(z, return_inverse=True)   # ascending
            mass = torch.zeros(vals.numel(), dtype=torch.float64)
            mass.scatter_add_(0, inv, pr)
            above = mass.flip(0).cumsum(0).flip(0) - mass
            self.G = above[inv]
            self.m_amb = float(mass[(above - top_p).abs() <= TOL].sum())
            keep = keep & (self.G <= top_p)
        self.w = pr * keep
        c = self.w.cumsum(0)
        self.c_last = float(c[-1])
        self.c = c / c[-1]

    def token(self, u):
        if self.greedy:
            return self.argmax
        hit = ((self.c > u) & (self.w > 0)).nonzero()
        return int(hit[0]) if hit.numel() else int((self.w > 0).nonzero()[-1])

    def check(self, t, u):
        if self.greedy:
            assert t == self.argmax
            return
        assert 0 <= t < self.w.numel()
        assert self.survives[t], f"token {t} is below the top-k threshold"
        if self.top_p is not None:
            assert float(self.G[t]) <= self.top_p + TOL, \
                f"token {t}: G = {float(self.G[t])} > top_p"
        s = (TOL + 2 * self.m_amb) / self.c_last
        lo = float(self.c[t - 1]) if t > 0 else 0.0
        hi = float(self.c[t])
        assert lo - s <= u <= hi + s, \
            f"token {t} covers [{lo}, {hi}], u = {u}, slack {s}"
        if self.m_amb == 0 and u in (0.0, LAST_U):
            assert t == self.token(u), f"u = {u}: {t} != {self.token(u)}"


@pytest.mark.parametrize("params", sorted(PARAMS))
@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("V", VOCABS)
def test_kernel_against_fp64_reference(V, dtype, params):
    from modalities_amd import ops
    temperature, top_k, top_p = PARAMS[params]
    x = _logits(V, DTYPES[dtype])
    ref = Reference(x, temperature, top_k, top_p)
    if not ref.greedy:
        assert ref.m_amb <= 1e-3, "the case's own ambiguity is too large"
    u = _u()
    flat = x.to(DEV).repeat(B, 1).contiguous()
    wide = torch.full((B, 3, V), 100.0, dtype=x.dtype, device=DEV)
    wide[:, -1] = flat
    got = []
    for rows in (flat, wide[:, -1, :]):
        out = torch.full((B, 1), -1, dtype=torch.long, device=DEV)
        assert ops.sample_logits(rows, u.to(DEV), out, temperature, top_k,
                                 top_p) is out
        got.append(out[:, 0].tolist())
    assert got[0] == got[1], "the row layout changed a token"
    worst = 0.0
    for t, ur in zip(got[0], u.double().tolist()):
        ref.check(t, ur)
        if not ref.greedy:
            lo = float(ref.c[t - 1]) if t > 0 else 0.0
            worst = max(worst, lo - ur, ur - float(ref.c[t]))
    print(f"V={V} {dtype} {params}: m_amb={getattr(ref, 'm_amb', 0.0):.3g} "
          f"largest excursion of u beyond its token={worst:.3g}")


def test_same_row_same_token_at_every_batch_position():
    """Top-p sums are order-fixed: 32 copies of a row with one u agree, on
    an odd V whose contiguous rows start at every 2-byte alignment."""
    from modalities_amd import ops
    x = _logits(50257, torch.bfloat16).to(DEV).repeat(B, 1)
    for u in (0.0, 0.25, 0.949, LAST_U):
        out = torch.empty(B, dtype=torch.long, device=DEV)
        ops.sample_logits(x, torch.full((B,), u, device=DEV), out, 1.0, 0,
                          0.95)
        assert out.unique().numel() == 1, out.tolist()


def _generate(model, prompt, sampler, graph, steps=8):
    """Prefill, then `steps` tokens with ops.sample_logits: eagerly, or from
    a DecodeGraph that samples inside the capture. Returns per step the
    logits row, u and the id sampled from them."""
    from modalities_amd import ops
    from modalities_amd.inference.text_generation import DecodeGraph
    from tests.test_decode_model_gpu import _chunk
    B_ = prompt.shape[0]
    trace = []
    with torch.no_grad():
        cache = model.new_kv_cache(B_, max_len=_chunk() + 16)
        out = model.forward_cached({"input_ids": prompt}, cache)["logits"]
        u = torch.rand(B_, device=DEV)
        ids = torch.empty(B_, 1, dtype=torch.long, device=DEV)
        ops.sample_logits(out[:, -1, :], u, ids, *sampler)
        trace.append((out[:, -1].clone(), u.clone(), ids.clone()))
        g = DecodeGraph(model, cache, "input_ids", "logits", sampler) \
            if graph else None
        for i in range(steps - 1):
            if g is not None:
                out = g.step(ids if i == 0 else None)
                u, ids = g.u, g.ids
            else:
                out = model.forward_cached({"input_ids": ids}, cache)["logits"]
                u = torch.rand(B_, device=DEV)
                ids = torch.empty(B_, 1, dtype=torch.long, device=DEV)
                ops.sample_logits(out[:, -1, :], u, ids, *sampler)
            trace.append((out[:, -1].clone(), u.clone(), ids.clone()))
    return trace


def test_device_sampling_in_the_decode_graph():
    from modalities_amd import ops
    from tests.test_decode_model_gpu import _chunk, _model, _prompt
    was = ops.decode_attention_enabled()
    ops.set_decode_attention(True)
    try:
        model = _model(fused_qkv=True, n_head_q=4, n_head_kv=2)
        prompt = _prompt(2, _chunk() - 3)
        # temperature 0: eager and replayed sampling give today's greedy ids
        with torch.no_grad():
            cache = model.new_kv_cache(2, max_len=_chunk() + 16)
            out = model.forward_cached({"input_ids": prompt}, cache)["logits"]
            today = []
            for _ in range(8):
                today.append(out[:, -1, :].float().argmax(-1, keepdim=True))
                out = model.forward_cached({"input_ids": today[-1]},
                                           cache)["logits"]
        for graph in (False, True):
            trace = _generate(model, prompt, (0.0, 0, 0.0), graph)
            assert [t[2].tolist() for t in trace] \
                == [t.tolist() for t in today], f"graph={graph}"
        # temperature 1, top-k 50: every replayed token against its logits
        torch.manual_seed(11)
        trace = _generate(model, prompt, (1.0, 50, 0.0), graph=True)
        us = torch.stack([t[1] for t in trace[1:]])
        assert us.unique().numel() == us.numel(), "a replay reused its u"
        for logits, u, ids in trace:
            for b in range(2):
                Reference(logits[b], 1.0, 50, 0.0).check(
                    int(ids[b]), float(u[b].double()))
    finally:
        ops.set_decode_attention(was)


def test_generate_tokens_with_device_sampling(monkeypatch):
    """The public switch: greedy text is the same with it off, on, and on
    without the graph; with it on the graph samples its own input."""
    from modalities_amd import ops
    from modalities_amd.inference import text_generation as tg
    from modalities_amd.tokenization.tokenizer_wrapper import CharTokenizer
    from tests.test_decode_model_gpu import _model
    was = ops.decode_attention_enabled()
    ops.set_decode_attention(True)
    try:
        model = _model(vocab=260, fused_qkv=True, n_head_q=4, n_head_kv=2)
        kw = dict(prompt_template="{text}", sequence_length=24,
                  temperature=0.0, device=torch.device(DEV))
        off = tg.TextInferenceComponent(model, CharTokenizer(), **kw)
        on = tg.TextInferenceComponent(model, CharTokenizer(),
                                       device_sampling=True, **kw)
        eager = tg.TextInferenceComponent(model, CharTokenizer(),
                                          device_sampling=True,
                                          use_decode_graph=False, **kw)
        text = off.generate_tokens("hello world")
        assert eager.generate_tokens("hello world") == text
        fed = []
        step = tg.DecodeGraph.step
        monkeypatch.setattr(
            tg.DecodeGraph, "step",
            lambda g, ids=None: fed.append(ids is not None) or step(g, ids))
        assert on.generate_tokens("hello world") == text
        assert fed[0] and len(fed) > 1 and not any(fed[1:]), fed
    finally:
        ops.set_decode_attention(was)
