"""fp64 oracles and checkers for the code that COMPOSES the HIP kernels (no
GPU needed): the attention backward with a gradient of its lse output, one
rank's ring context-parallel attention, and the ShardedAdamW +
clip_grad_norm_ optimizer tail.

Same conventions as tests/kernel_oracles.py: a checker returns
``{name: error / bound}``, a correct implementation has every ratio <= 1,
keys starting with ``~`` are informational, ``ko.require`` prints and
asserts.  tests/test_composed_oracles_cpu.py proves that the checkers accept
correct pure-torch implementations and reject mutants;
tests/test_composed_paths_gpu.py runs them on the production paths.

Bounds (derived, never tuned):

* ring forward, ``|o - ref| <= 4 * 2^-8 * (P|V|) + 2^-126``.  Each partial
  o_s carries the single-kernel error 3 * 2^-8 * P_s|V| (kernel_oracles);
  the merge weights w_s = exp(lse_s - lse) are exact up to the lse error
  (1e-4, far below 2^-9) and sum_s w_s P_s|V| = P|V|; the merge itself is
  fp32; the final cast to bf16 adds 2^-9 |o| <= 2^-9 P|V|.  3 + 1/2 < 4.
* ring backward, per tensor, the rule of ko.check_attn_bwd:
  ``max|got - ref| <= 2 max|emul - ref| + 2^-12 max|ref| + 2^-18 C``, where
  ref is fp64 FULL attention over all cp_size chunks with the rank's offset
  and emul is the CPU ring emulation: the production ring helper and
  ``_merge_partials`` under autograd with ko.torch_attn_fwd /
  ko.torch_attn_bwd (with dlse) as the partial kernel, from the same
  inputs.  The per-chunk bf16 rounding of dq and its bf16 accumulation by
  autograd are therefore common to both sides.
* optimizer tail: the bounds of ko.check_adamw, unchanged (m, v:
  2^-18 S + 2^-126; p: 2^-20 S_p + 2^-126; published copy bit-identical),
  against ko.adamw_ref64 evaluated per step from clones of the state taken
  just before the step.  The clip coefficient and the weight-decay mask of
  the reference are computed here, independently of the engine.  The total
  norm is checked SQUARED against the fp64 sum of squares with
  ko.check_sqsum's bound 2^-18 * ref: squaring a correctly rounded fp32
  sqrt adds at most 2^-23 of relative error, 1/32 of the bound.
"""

import torch

from tests import kernel_oracles as ko

INF = ko.INF
HEADS = dict(B=2, Hq=4, Hkv=2)

# the cases of the CPU proof and of the GPU tests
# (Tq, Tkv, off): one key; odd; two q tiles; decode-like; fully unmasked
DLSE_SHAPES = [(1, 1, 0), (33, 33, 0), (130, 130, 0), (5, 200, 195),
               (40, 40, 40)]
RING_SHAPES = [(2, 33), (3, 40), (4, 16), (2, 130)]      # (cp_size, Tl)
RING_CASES = [(cp, Tl, r) for cp, Tl in RING_SHAPES for r in range(cp)]
RING_IDS = [f"cp{cp}-Tl{Tl}-r{r}" for cp, Tl, r in RING_CASES]


# --------------------------------------------------------------------------
# A. attention backward with dlse
# --------------------------------------------------------------------------
def dlse_case(D, Tq, Tkv, off, device, seed=None):
    """ko.AttnCase with dlse ~ N(0,1) fp32 [B,Hq,Tq] (the ring's real dlse is
    w * dO . (o_s - o), which is O(1))."""
    seed = Tq * 7 + Tkv + D if seed is None else seed
    inp = ko.attn_random_inputs(HEADS["B"], Tq, Tkv, HEADS["Hq"],
                                HEADS["Hkv"], D, device, seed=seed)
    dlse = torch.randn(HEADS["B"], HEADS["Hq"], Tq,
                       generator=ko._gen(seed + 1)).to(device)
    return ko.AttnCase(inp, off, dlse=dlse)


# --------------------------------------------------------------------------
# B. one rank of ring context parallelism
# --------------------------------------------------------------------------
class _TorchFlashWithLse(torch.autograd.Function):
    """The partial kernel of the CPU ring emulation: ko.torch_attn_fwd /
    ko.torch_attn_bwd, differentiable in o AND lse.  mut = drop_dlse."""

    @staticmethod
    def forward(ctx, q, k, v, off, mut):
        o, lse = ko.torch_attn_fwd(q, k, v, off)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.off, ctx.mut = off, mut
        ctx.set_materialize_grads(False)
        return o, lse

    @staticmethod
    def backward(ctx, do, dlse):
        q, k, v, o, lse = ctx.saved_tensors
        if do is None:
            do = torch.zeros_like(o)
        dq, dk, dv = ko.torch_attn_bwd(do, q, k, v, o, lse, ctx.off,
                                       mut=ctx.mut, dlse=dlse)
        return dq, dk, dv, None, None


def torch_flash_with_lse(mut=None):
    """flash_with_lse(q, k, v, off) -> (o, lse) from the torch emulation.
    mut: drop_dlse (backward ignores the lse gradient) or causal_off_diag
    (off = 0 also for the unmasked off-diagonal chunks)."""
    def f(q, k, v, off):
        if mut == "causal_off_diag":
            off = 0
        return _TorchFlashWithLse.apply(
            q.contiguous(), k.contiguous(), v.contiguous(), off,
            mut if mut == "drop_dlse" else None)
    return f


def merge_swapped_weights(o_a, lse_a, o_b, lse_b):
    """_merge_partials mutant: each partial weighted with the OTHER's lse."""
    lse_new = torch.logaddexp(lse_a, lse_b)
    w_a = torch.exp(lse_b - lse_new).permute(0, 2, 1).unsqueeze(-1)
    w_b = torch.exp(lse_a - lse_new).permute(0, 2, 1).unsqueeze(-1)
    return o_a.float() * w_a + o_b.float() * w_b, lse_new


def run_ring_rank(flash_with_lse, q, k_full, v_full, do, cp_rank, cp_size):
    """The production ring helper on one device: step s is handed chunk
    (cp_rank - s) % cp_size as a differentiable slice of the full k, v, so
    autograd sums the per-chunk dk/dv back into the full tensors.  Returns
    detached (o, dq, dk, dv)."""
    from modalities_amd.parallel.cp import _ring_local_attention
    Tl = q.shape[1]
    q = q.detach().clone().requires_grad_(True)
    k = k_full.detach().clone().requires_grad_(True)
    v = v_full.detach().clone().requires_grad_(True)

    def kv_at_step(s):
        c = (cp_rank - s) % cp_size
        sl = slice(c * Tl, (c + 1) * Tl)
        return torch.stack((k[:, sl], v[:, sl]))

    o = _ring_local_attention(q, kv_at_step, cp_rank, cp_size,
                              flash_with_lse)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


class RingCase:
    """Inputs of one (cp_size, Tl, D, cp_rank), the fp64 full-attention
    reference and the CPU ring emulation, computed once."""

    def __init__(self, cp_size, Tl, D, cp_rank, device, seed=None):
        seed = 1000 * cp_size + 10 * Tl + D + cp_rank if seed is None else seed
        inp = ko.attn_random_inputs(HEADS["B"], Tl, cp_size * Tl, HEADS["Hq"],
                                    HEADS["Hkv"], D, device, seed=seed)
        self.cp_size, self.cp_rank, self.Tl = cp_size, cp_rank, Tl
        self.q, self.k, self.v, self.do = (inp[n] for n in "q k v do".split())
        self.full = ko.AttnCase(inp, cp_rank * Tl)
        self.ref = self.full.ref
        self.emul = run_ring_rank(torch_flash_with_lse(), self.q, self.k,
                                  self.v, self.do, cp_rank, cp_size)
        self.emul_err = {
            n: (t.double() - self.ref[n]).abs().max().item()
            for n, t in zip(("dq", "dk", "dv"), self.emul[1:])}


def check_ring_rank(flash_with_lse, case, cp_rank, cp_size):
    """flash_with_lse(q, k, v, off) -> (o, lse), differentiable in both.
    Runs the production ring helper with it, backpropagates case.do and
    compares o, dq, dk, dv with fp64 full attention at Tq = Tl,
    Tkv = cp_size * Tl, off = cp_rank * Tl."""
    assert (cp_rank, cp_size) == (case.cp_rank, case.cp_size)
    o, dq, dk, dv = run_ring_rank(flash_with_lse, case.q, case.k, case.v,
                                  case.do, cp_rank, cp_size)
    r = case.ref
    assert o.dtype == case.q.dtype and o.shape == case.q.shape
    res = {"o": ko.ratio((o.double() - r["o"]).abs(),
                         4 * ko.BF16_ULP * r["absPV"] + ko.F32_TINY)}
    for n, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        err = (got.double() - r[n]).abs().max().item()
        if err != err:
            err = INF
        e = case.emul_err[n]
        bound = 2 * e + ko.BF16_ULP * r[n].abs().max().item() * 2.0 ** -4 \
            + ko.F32_SLACK * r["C_" + n] + ko.F32_TINY
        res[n] = err / bound
        res["~" + n + "/emul"] = err / e if e > 0 else 0.0
    # keys of the chunks after the rank's own are never attended to
    end = (cp_rank + 1) * case.Tl
    zero = all(not t[:, end:].any().item() for t in (dk, dv))
    res["later_chunks_zero"] = 0.0 if zero else INF
    return res


# --------------------------------------------------------------------------
# C. optimizer tail: ShardedAdamW + clip_grad_norm_
#
# The checkers drive anything shaped like the production pair:
#   model.units[i].{master_shard, grad_shard, grad_fresh, wd_mask_shard,
#                   bf16_shard, param_infos, shapes, offsets, numels}
#   model.clip_grad_norm_(max_norm) -> total norm
#   opt.state[u.master_shard]{"step", "exp_avg", "exp_avg_sq"}, opt.step(),
#   opt._step_dev (shared counter; None where the engine keeps none)
# --------------------------------------------------------------------------
OPT_HP = dict(lr=1e-3, wd=0.1, b1=0.9, b2=0.95, eps=1e-8)


def expected_wd_mask(u):
    """[shard_numel] fp32 built from the unit's parameter list: 0 where
    the parameter has fewer than 2 dimensions, 1 elsewhere (the padding
    tail holds p = g = 0, where the mask has no effect; 1 there).  The
    parameter's rank is read from u.shapes: the engine releases p.data
    while a unit is not gathered, so p.ndim is not the parameter's."""
    mask = torch.ones(u.master_shard.numel())
    assert len(u.shapes) == len(u.param_infos)
    for shape, off, n in zip(u.shapes, u.offsets, u.numels):
        if len(shape) < 2:
            mask[off:off + n] = 0.0
    return mask


def check_wd_mask(model):
    ok, seen = True, set()
    for u in model.units:
        n = sum(u.numels)
        exp = expected_wd_mask(u)[:n]
        ok &= torch.equal(u.wd_mask_shard[:n].cpu(), exp)
        seen |= set(exp.unique().tolist())
    return {"wd_mask": 0.0 if ok else INF,
            "wd_mask_both_values": 0.0 if seen == {0.0, 1.0} else INF}


def write_grads(model, seed, target_norm=None):
    """Writes known grads straight into every unit's grad_shard (drawn as in
    ko.adamw_inputs: N(0,1) with 0, 1e-8 and 1e4 entries; zeros in the
    padding tail) and marks them fresh.  target_norm rescales them to about
    that global norm.  Returns the fp32 values written, on the CPU."""
    gs = []
    for i, u in enumerate(model.units):
        n = sum(u.numels)
        g = torch.zeros(u.grad_shard.numel())
        g[:n] = ko.adamw_inputs(n, "cpu", seed=seed + i)[1]
        gs.append(g)
    if target_norm is not None:
        norm = sum(g.double().pow(2).sum() for g in gs).sqrt().item()
        gs = [(g.double() * (target_norm / norm)).float() for g in gs]
    for u, g in zip(model.units, gs):
        u.grad_shard.copy_(g)
        u.grad_fresh = True
    return gs


def norm64(gs):
    return sum(g.double().pow(2).sum() for g in gs).sqrt().item()


def clip_ref64(gs, max_norm):
    """min(1, max_norm / (norm64 + 1e-6)) from the grads that were written."""
    return min(1.0, max_norm / (norm64(gs) + 1e-6))


def check_total_norm(total, gs):
    ref = torch.tensor(norm64(gs), dtype=torch.float64) ** 2
    got = total.double().cpu() ** 2
    return ko.f32_sum_ratio(got, ref, ref)


def checked_step(model, opt, gs, t, gscale, hp=OPT_HP, host_bc=False):
    """opt.step() against ko.adamw_ref64 computed from clones of the state
    taken just before the step (errors do not compound across steps).
    gs: the grads written; gscale: the reference clip coefficient or None;
    host_bc: the engine evaluates the bias corrections on the host in fp64
    (the unfused fp32-working-copy branch)."""
    before = []
    for u in model.units:
        st = opt.state[u.master_shard]
        before.append([x.detach().clone().cpu() for x in
                       (u.master_shard, st["exp_avg"], st["exp_avg_sq"])])
    opt.step()
    res = {"m": 0.0, "v": 0.0, "p": 0.0, "publish_bits": 0.0, "step": 0.0}
    bc = (1.0 - hp["b1"] ** t, 1.0 - hp["b2"] ** t) if host_bc else None
    for u, g, (p0, m0, v0) in zip(model.units, gs, before):
        st = opt.state[u.master_shard]
        r = ko.adamw_ref64(p0, g, m0, v0, expected_wd_mask(u), t, hp["b1"],
                           hp["b2"], hp["lr"], hp["eps"], hp["wd"], gscale,
                           bc)
        p, m, v = (x.detach().cpu() for x in
                   (u.master_shard, st["exp_avg"], st["exp_avg_sq"]))
        res["m"] = max(res["m"], ko.f32_sum_ratio(m, r["m"], r["S_m"],
                                                  ko.F32_TINY))
        res["v"] = max(res["v"], ko.f32_sum_ratio(v, r["v"], r["S_v"],
                                                  ko.F32_TINY))
        res["p"] = max(res["p"], ko.ratio((p.double() - r["p"]).abs(),
                                          2.0 ** -20 * r["S_p"] + ko.F32_TINY))
        pub = u.bf16_shard.detach().cpu()
        bits = torch.int16 if pub.dtype == torch.bfloat16 else torch.int32
        if not torch.equal(pub.view(bits), p.to(pub.dtype).view(bits)):
            res["publish_bits"] = INF
        if st["step"] != t:
            res["step"] = INF
    sd = getattr(opt, "_step_dev", None)
    if sd is not None and int(sd) != t:
        res["step"] = INF
    return res


def check_opt_sequence(model, opt, hp=OPT_HP, host_bc=False, steps=3):
    """step 1: clip at 1.0 with a grad norm far above 1 (gscale < 1);
    step 2: no clip call (gscale None: a stale coefficient shows);
    step 3: clip at 1.0 with the norm at 0.5 (gscale exactly 1.0).
    Returns {"s<k>/<name>": ratio}."""
    res = {}

    def put(k, d):
        res.update({f"s{k}/{n}": x for n, x in d.items()})

    gs = write_grads(model, seed=11)
    total = model.clip_grad_norm_(1.0)
    gscale = clip_ref64(gs, 1.0)
    assert gscale < 1e-2
    put(1, {"norm": check_total_norm(total, gs)})
    put(1, checked_step(model, opt, gs, 1, gscale, hp, host_bc))
    if steps >= 2:
        gs = write_grads(model, seed=23)
        put(2, checked_step(model, opt, gs, 2, None, hp, host_bc))
    if steps >= 3:
        gs = write_grads(model, seed=37, target_norm=0.5)
        total = model.clip_grad_norm_(1.0)
        gscale = clip_ref64(gs, 1.0)
        assert gscale == 1.0
        put(3, {"norm": check_total_norm(total, gs)})
        put(3, checked_step(model, opt, gs, 3, gscale, hp, host_bc))
    return res


def check_opt_warm_start(model, opt, hp=OPT_HP, host_bc=False, start=7):
    """A fresh optimizer whose per-unit step is `start` (a loaded
    checkpoint) must take its first step with t = start + 1."""
    for u in model.units:
        opt.state[u.master_shard]["step"] = start
    gs = write_grads(model, seed=41)
    return checked_step(model, opt, gs, start + 1, None, hp, host_bc)


# -- pure-torch stand-in for the engine (CPU proof of the checkers) ---------
class _StandInUnit:
    def __init__(self, shapes, seed):
        g = ko._gen(seed)
        self.param_infos = [(None, f"p{i}", torch.nn.Parameter(
            torch.randn(*s, generator=g))) for i, s in enumerate(shapes)]
        self.shapes = [p.shape for _, _, p in self.param_infos]
        self.numels = [p.numel() for _, _, p in self.param_infos]
        self.offsets = [sum(self.numels[:i]) for i in range(len(shapes))]
        total = -(-sum(self.numels) // 64) * 64
        self.master_shard = torch.zeros(total)
        self.wd_mask_shard = torch.ones(total)
        for (_, _, p), off, n in zip(self.param_infos, self.offsets,
                                     self.numels):
            self.master_shard[off:off + n] = p.detach().reshape(-1)
            if p.ndim < 2:
                self.wd_mask_shard[off:off + n] = 0.0
        self.grad_shard = torch.empty(total)
        self.grad_fresh = False
        self.bf16_shard = self.master_shard.to(torch.bfloat16)


class TorchShardedStandIn:
    """Two units with decayed (2-D) and undecayed (1-D) parameters and a
    padding tail each; clip_grad_norm_ defers the coefficient."""

    def __init__(self):
        self.units = [_StandInUnit([(8, 12), (12,), (12, 8)], 1),
                      _StandInUnit([(16,), (16, 8)], 2)]
        self._pending_grad_scale = None

    def clip_grad_norm_(self, max_norm):
        total = sum(u.grad_shard.pow(2).sum() for u in self.units).sqrt()
        self._pending_grad_scale = (max_norm / (total + 1e-6)).clamp(max=1.0)
        return total


class TorchAdamWStandIn:
    """ko.torch_adamw_step driven like ShardedAdamW.step.  mut:
    stale_gscale (the coefficient is not cleared after use),
    warm_counter_zero (the shared counter ignores a loaded step count),
    ones_mask (every element decays)."""

    def __init__(self, model, hp=OPT_HP, mut=None):
        self.model, self.hp, self.mut = model, hp, mut
        self.state = {u.master_shard: dict(
            step=0, exp_avg=torch.zeros_like(u.master_shard),
            exp_avg_sq=torch.zeros_like(u.master_shard)) for u in model.units}
        self._step_dev = None

    @torch.no_grad()
    def step(self):
        hp = self.hp
        if self._step_dev is None:
            start = 0 if self.mut == "warm_counter_zero" else max(
                st["step"] for st in self.state.values())
            self._step_dev = torch.tensor(start, dtype=torch.int32)
        self._step_dev += 1
        gscale = self.model._pending_grad_scale
        if self.mut != "stale_gscale":
            self.model._pending_grad_scale = None
        for u in self.model.units:
            st = self.state[u.master_shard]
            st["step"] += 1
            mask = torch.ones_like(u.wd_mask_shard) \
                if self.mut == "ones_mask" else u.wd_mask_shard
            u.bf16_shard = ko.torch_adamw_step(
                u.master_shard, u.grad_shard, st["exp_avg"],
                st["exp_avg_sq"], mask, int(self._step_dev), hp["b1"],
                hp["b2"], hp["lr"], hp["eps"], hp["wd"], gscale)
