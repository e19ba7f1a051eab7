#!/usr/bin/env python3
"""Flagship training benchmark for modalities_amd on MI355X.

Measures the BASELINE.json metric: whole-node training tokens/s (+MFU) for
the reference's EXACT 2.7B GPT shape (h=2560, L=32, 32 heads x head_dim 80,
seq 4096, bf16, FSDP full-shard equivalent, micro-batch 2 per GPU — the
reference's headline scaling config, /root/reference/README.md:321:
18.63 samples/s on 8xA100 = 76.3k tok/s). The K1 v2 kernels run head_dim
80 natively (r1 ran an hd=128/20-head equivalent; kept as
gpt2-2.7b-hd128 for A/B). Weak scaling: per-GPU batch fixed as N grows.

Usage:
  python bench.py --gpus 1 --steps 20 --warmup 5          # single GPU
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
      # + DIR/loss.npy, DIR/master_weights_sample.npy from the last step

A plain run sets up, warms up, times the steps and prints the result line;
--full is where any secondary measurement belongs (none exist today).

Synthetic data (random tokens, fixed seed per step), random-init weights.
Rank 0 prints ONE JSON line with the whole-job aggregate.
"""

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def build_model_cfg(model_name: str):
    from modalities_amd.models.gpt2 import GPT2LLMConfig
    if model_name == "gpt2-2.7b":  # the exact reference shape (32 x hd80)
        return GPT2LLMConfig(
            vocab_size=50304, n_layer=32, n_head_q=32, n_head_kv=32,
            n_embd=2560, ffn_hidden=10240, sequence_length=4096,
            activation_type="swiglu", use_weight_tying=False)
    if model_name == "gpt2-2.7b-hd128":  # MFMA-square-tile variant (r1 cfg)
        return GPT2LLMConfig(
            vocab_size=50304, n_layer=32, n_head_q=20, n_head_kv=20,
            n_embd=2560, ffn_hidden=10240, sequence_length=4096,
            activation_type="swiglu", use_weight_tying=False)
    if model_name == "gpt2-8b":  # Llama-8B-like (BASELINE.json config 3)
        return GPT2LLMConfig(
            vocab_size=50304, n_layer=32, n_head_q=32, n_head_kv=8,
            n_embd=4096, ffn_hidden=21504, sequence_length=8192,
            activation_type="swiglu", use_weight_tying=False)
    if model_name == "gpt2-70b":  # 288GB-HBM sizing config (BASELINE.json 5)
        return GPT2LLMConfig(
            vocab_size=50304, n_layer=80, n_head_q=64, n_head_kv=8,
            n_embd=8192, ffn_hidden=43008, sequence_length=4096,
            activation_type="swiglu", use_weight_tying=False)
    if model_name == "gpt2-tiny":  # smoke/debug
        return GPT2LLMConfig(
            vocab_size=50304, n_layer=4, n_head_q=4, n_head_kv=4,
            n_embd=512, ffn_hidden=2048, sequence_length=1024)
    raise ValueError(model_name)


DUMP_SAMPLE_PER_UNIT = 1 << 18  # fp32 elements sampled per shard unit (1 MiB)
DUMP_SAMPLE_MAX_TOTAL = 1 << 23  # whole dump stays under 32 MiB


@torch.no_grad()
def dump_outputs(out_dir: str, loss: torch.Tensor, sharded) -> None:
    """Write what the last timed step handed back: its loss, and the state
    it left behind — this rank's fp32 master weights, one fixed seeded
    sample of DUMP_SAMPLE_PER_UNIT elements per shard unit (the full 2.7B
    state is ~11 GB). Same arguments => same inputs => comparable files."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().reshape(1).cpu().numpy())
    g = torch.Generator().manual_seed(4321)
    per_unit = min(DUMP_SAMPLE_PER_UNIT,
                   DUMP_SAMPLE_MAX_TOTAL // max(len(sharded.units), 1))
    samples = []
    for u in sharded.units:
        shard = u.master_shard
        if shard.numel() > per_unit:
            idx = torch.randint(0, shard.numel(), (per_unit,), generator=g)
            shard = shard[idx.to(shard.device)]
        samples.append(shard.float().cpu())
    np.save(os.path.join(out_dir, "master_weights_sample.npy"),
            torch.cat(samples).numpy())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--micro-batch", type=int, default=2)
    p.add_argument("--seq-len", type=int, default=None,
                   help="default: the model config's native length")
    p.add_argument("--model", type=str, default="gpt2-2.7b")
    p.add_argument("--blocks-per-unit", type=int, default=4)
    p.add_argument("--reshard", action="store_true")
    p.add_argument("--ac", action="store_true",
                   help="full activation checkpointing")
    p.add_argument("--ac-variant", type=str, default="full",
                   choices=["full", "selective_layer", "selective_op"],
                   help="checkpointing variant when --ac is set")
    p.add_argument("--tp", type=int, default=1, help="tensor-parallel degree")
    p.add_argument("--no-graph", action="store_true",
                   help="disable hipGraph step capture")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write what the last timed "
                        "step computed (loss + a seeded sample of the "
                        "updated fp32 master weights) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements "
                        "(none today: a plain run already does only what "
                        "the headline figure needs)")
    args = p.parse_args()
    assert args.steps >= 1, "--steps must be >= 1"

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    assert world == args.gpus or world == 1, \
        f"WORLD_SIZE={world} but --gpus={args.gpus}"

    on_gpu = torch.cuda.is_available()
    # Load pre-tuned hipBLASLt GEMM algorithm choices (TunableOp) for the
    # benchmark shapes; tuned offline on MI355X (assets/tunableop_gfx950.csv).
    tuned_file = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                              "assets", "tunableop_gfx950.csv")
    # Re-tune mode: PYTORCH_TUNABLEOP_{ENABLED,TUNING,FILENAME} env vars
    # drive tuning (set by tools/ retune invocation); bench only LOADS the
    # committed results otherwise.
    tuning_mode = os.environ.get("PYTORCH_TUNABLEOP_TUNING") == "1"
    if on_gpu and os.path.exists(tuned_file) and not tuning_mode:
        try:
            torch.cuda.tunable.enable(True)
            torch.cuda.tunable.tuning_enable(False)
            torch.cuda.tunable.set_filename(tuned_file, insert_device_ordinal=False)
            torch.cuda.tunable.read_file(tuned_file)
        except Exception as e:
            import sys
            print(f"# TunableOp load skipped: {e}", file=sys.stderr)
    if world > 1:
        dist.init_process_group("nccl" if on_gpu else "gloo")
    if on_gpu:
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    from modalities_amd.models.gpt2 import GPT2LLM
    from modalities_amd.optimizers.optimizer_factory import get_adam_w
    from modalities_amd.ops import fused_cross_entropy
    from modalities_amd.parallel.fsdp import XGMIShardedModel
    from modalities_amd.utils.mfu import GPT2MFUCalculator, detect_device_peak_flops

    cfg = build_model_cfg(args.model)
    if args.seq_len is None:
        args.seq_len = cfg.sequence_length
    cfg.sequence_length = args.seq_len
    cfg.fused_qkv = True  # one [h, h+2kv] GEMM per block (MI355X-first;
    # TP shards the joint weight per head group since r2)
    torch.manual_seed(1234)  # identical init on all ranks
    model = GPT2LLM(cfg)
    num_params = sum(p_.numel() for p_ in model.parameters())

    mesh = None
    dp_world, dp_rank = world, rank
    if args.tp > 1:
        from modalities_amd.parallel.mesh import (ParallelismDegrees,
                                                  get_device_mesh)
        from modalities_amd.parallel.tp import \
            get_gpt2_tensor_parallelized_model
        mesh = get_device_mesh(world, rank, tensor_parallel_degree=args.tp)
        model = get_gpt2_tensor_parallelized_model(model, device_mesh=mesh)
        dp_world = mesh.dp_degree
        dp_rank = mesh.dp_rank
    if args.ac:
        from modalities_amd.training.activation_checkpointing import (
            ActivationCheckpointingVariant, apply_activation_checkpointing_)
        variant = {
            "full": ActivationCheckpointingVariant.FULL_ACTIVATION_CHECKPOINTING,
            "selective_layer":
                ActivationCheckpointingVariant.SELECTIVE_LAYER_ACTIVATION_CHECKPOINTING,
            "selective_op":
                ActivationCheckpointingVariant.SELECTIVE_OP_ACTIVATION_CHECKPOINTING,
        }[args.ac_variant]
        # selective_layer means every-2nd layer (k=1 would equal FULL)
        k = 2 if args.ac_variant == "selective_layer" else 1
        apply_activation_checkpointing_(model, variant, every_k_layers=k)

    if mesh is not None:
        from modalities_amd.models.model_factory import ModelFactory
        sharded = ModelFactory.get_sharded_model(
            model, device_mesh=mesh, blocks_per_unit=args.blocks_per_unit,
            reshard_after_forward=args.reshard,
            param_dtype="bf16" if on_gpu else "fp32", device=device)
    else:
        sharded = XGMIShardedModel.from_transformer(
            model, device, blocks_per_unit=args.blocks_per_unit,
            param_dtype=torch.bfloat16 if on_gpu else torch.float32,
            reshard_after_forward=args.reshard)
    opt = get_adam_w(sharded, lr=3e-4, weight_decay=0.1)

    B, T, V = args.micro_batch, args.seq_len, cfg.vocab_size

    def make_batch(step: int):
        # TP ranks in one dp group must see the SAME data
        g = torch.Generator().manual_seed(10_000 + step * dp_world + dp_rank)
        ids = torch.randint(0, V, (B, T + 1), generator=g)
        return ids[:, :-1].to(device, non_blocking=True), \
            ids[:, 1:].to(device, non_blocking=True)

    def run_step(x, y):
        out = sharded({"input_ids": x})
        loss = fused_cross_entropy(out["logits"], y)
        loss.backward()
        sharded.backward_epilogue()
        sharded.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad()
        return loss

    def eager_step(step: int):
        x, y = make_batch(step)
        return run_step(x, y)

    one_step = eager_step
    graph_mode = False
    # Graph capture only at world 1: RCCL-collective capture support is not
    # risked in the multi-GPU scaling run (a capture hang there would cost
    # the whole run; the measured replay gain is ~1%). Comm/compute overlap
    # at N>1 comes from the engine's dedicated HIP streams either way.
    if on_gpu and world == 1 and not args.no_graph:
        # hipGraph-capture the whole training step (launch-bound gaps were
        # ~10% of step time): static input buffers, device-side Adam step
        # counter so replays advance bias correction. Fresh random data is
        # copied into the static buffers before every replay (full compute
        # runs every step). Falls back to eager on any capture failure.
        try:
            static_x = torch.zeros(B, T, dtype=torch.long, device=device)
            static_y = torch.zeros(B, T, dtype=torch.long, device=device)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for s in range(2):  # graph warmup on a side stream
                    x, y = make_batch(s)
                    static_x.copy_(x)
                    static_y.copy_(y)
                    run_step(static_x, static_y)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            x, y = make_batch(2)
            static_x.copy_(x)
            static_y.copy_(y)
            with torch.cuda.graph(graph):
                static_loss = run_step(static_x, static_y)

            def graph_step(step: int):
                x, y = make_batch(step)
                static_x.copy_(x)
                static_y.copy_(y)
                graph.replay()
                return static_loss

            one_step = graph_step
            graph_mode = True
        except Exception as e:
            import sys
            print(f"# hipGraph capture unavailable ({type(e).__name__}: {e}); "
                  f"running eager", file=sys.stderr, flush=True)
            one_step = eager_step

    for s in range(args.warmup):
        one_step(s)

    if on_gpu:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for s in range(args.steps):
        last_loss = one_step(args.warmup + s)
    if on_gpu:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # max over ranks = slowest rank's wall time
    t = torch.tensor([elapsed], device=device if on_gpu else "cpu")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_loss, sharded)

    ms_per_step = elapsed / args.steps * 1000
    tokens_per_step_global = B * T * dp_world
    tokens_per_s = tokens_per_step_global * args.steps / elapsed

    # Reference baseline: 2.7B 8xA100 FULL_SHARD mbs=2 -> 18.63 samples/s
    #  = 76,308 tok/s on 8 GPUs => 9538.6 tok/s per GPU.
    baseline_per_gpu = 18.63 * 4096 / 8
    vs_baseline = tokens_per_s / (baseline_per_gpu * world) \
        if args.model == "gpt2-2.7b" else None

    mfu = None
    if on_gpu:
        calc = GPT2MFUCalculator(cfg.n_layer, T, cfg.n_embd, world, num_params,
                                 detect_device_peak_flops())
        m = calc.compute(torch.tensor(tokens_per_s / T))
        mfu = round(m.item(), 4) if m.item() > 0 else None

    if rank == 0:
        print(json.dumps({
            "metric": "train_tokens_per_s",
            "value": round(tokens_per_s, 1),
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(vs_baseline, 3) if vs_baseline else None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": "synthetic",
            "mfu": mfu,
            "config": {"model": args.model, "global_batch": B * dp_world,
                       "micro_batch": B, "seq_len": T,
                       "parallelism": (f"dp{dp_world}_tp{args.tp}" if args.tp > 1
                                       else f"dp{world}_fullshard")
                       + ("_ac" if args.ac else "")
                       + ("_hipgraph" if graph_mode else ""),
                       "num_params": num_params},
        }), flush=True)

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()  # in PYTORCH_TUNABLEOP_TUNING=1 runs, torch writes the results
            # csv on process exit (env-configured filename)
