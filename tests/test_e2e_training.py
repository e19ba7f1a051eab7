"""End-to-end config-driven training on CPU: the full Main path (config ->
ComponentFactory -> Gym/Trainer), checkpointing to disk, results JSONL.
Mirrors the reference's getting-started e2e run (reference:
tests/end2end_tests/, config_files/training/)."""

import json
from pathlib import Path

import numpy as np
import pytest

from modalities_amd.dataloader.packed_data import write_pbin
from modalities_amd.main import Main


@pytest.fixture
def e2e_config(tmp_path) -> Path:
    rng = np.random.default_rng(7)
    # enough tokens for 8 steps x 2 samples x 32 tokens: need >= 16*32+1
    docs = [rng.integers(0, 256, size=200, dtype=np.uint8) for _ in range(8)]
    pbin = tmp_path / "data.pbin"
    write_pbin(pbin, docs, token_size_in_bytes=1)

    template = Path(__file__).parent / "configs" / "config_tiny_e2e.yaml"
    text = template.read_text()
    text = text.replace("DATASET_PATH_PLACEHOLDER", str(pbin))
    text = text.replace("CHECKPOINT_DIR_PLACEHOLDER", str(tmp_path / "checkpoints"))
    text = text.replace("RESULTS_PATH_PLACEHOLDER",
                        str(tmp_path / "evaluation_results.jsonl"))
    cfg = tmp_path / "config.yaml"
    cfg.write_text(text)
    return cfg


def test_e2e_training_run(e2e_config, tmp_path):
    main_obj = Main(e2e_config, experiment_id="test_e2e")
    components = main_obj.build_components()
    main_obj.run(components)

    # trained the target number of steps
    progress = components.app_state  # AppState
    assert progress is not None

    # checkpoints written with the reference folder-name schema
    ckpt_root = tmp_path / "checkpoints" / "test_e2e"
    folders = sorted(p.name for p in ckpt_root.iterdir() if p.is_dir())
    assert any("seen_steps_8" in f for f in folders), folders
    # keep-2-most-recent strategy
    assert len(folders) == 2, folders
    assert (ckpt_root / "last_checkpoint_info.json").exists()
    with open(ckpt_root / "last_checkpoint_info.json") as f:
        info = json.load(f)
    assert "seen_steps_8" in info["checkpoint_folder_path"]

    # results JSONL written with losses
    results_file = tmp_path / "evaluation_results.jsonl"
    assert results_file.exists()
    records = [json.loads(ln) for ln in results_file.read_text().splitlines()]
    train_records = [r for r in records if r.get("dataloader_tag") == "train"]
    assert train_records, records
    assert "CLMCrossEntropyLoss average" in train_records[-1]["losses"]
    # the evaluator ran on the eval dataloader at the configured interval
    val_records = [r for r in records if r.get("dataloader_tag") == "val"]
    assert val_records and "CLMCrossEntropyLoss" in val_records[-1]["losses"]

    # resolved config copied into the experiment folder
    assert (ckpt_root / "config.yaml.resolved").exists()


def test_e2e_losses_decrease(e2e_config):
    main_obj = Main(e2e_config, experiment_id="test_e2e_2")
    components = main_obj.build_components()
    main_obj.run(components)
    # model state is finite after training
    import torch
    for u in components.wrapped_model.units:
        assert torch.isfinite(u.master_shard).all()


def test_bench_contract_multirank_cpu(tmp_path):
    """The driver launches bench.py via torch.distributed.run at round end;
    validate that exact path on CPU/gloo world 2: both ranks run, rank 0
    prints exactly one JSON line with the contract fields, value aggregates
    over the whole job."""
    import json
    import os
    import subprocess
    import sys

    from tests.conftest import find_free_port
    env = dict(os.environ)
    # CPU/gloo on every host: hide any GPU from the two ranks
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(find_free_port()),
         os.path.join(repo, "bench.py"), "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--model", "gpt2-tiny", "--micro-batch", "1",
         "--seq-len", "64"],
        capture_output=True, text=True, timeout=600, env=env, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    json_lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(json_lines) == 1, r.stdout
    d = json.loads(json_lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2
    assert d["metric"] == "train_tokens_per_s"
    assert d["config"]["global_batch"] == 2  # micro_batch 1 x dp 2
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["scaling"] == "weak"
    assert d["dtype"] == "fp32"  # CPU fallback dtype (bf16 on GPU)
    # the full driver contract: every documented field present
    for field in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                  "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                  "dtype", "data", "config"):
        assert field in d, field
    assert d["higher_is_better"] is True and d["data"] == "synthetic"
    for field in ("model", "global_batch", "micro_batch", "seq_len",
                  "parallelism", "num_params"):
        assert field in d["config"], field


def test_bench_dump_outputs_reproducible_cpu(tmp_path):
    """--dump-outputs writes the last timed step's loss and a seeded sample
    of the updated master weights as float32 .npy files; the same arguments
    give the same files (same inputs), and --full is accepted."""
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    # a CPU run wherever the suite runs: bit-identical across processes
    env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""

    def run(out_dir, *extra):
        r = subprocess.run(
            [sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1",
             "--steps", "2", "--warmup", "1", "--model", "gpt2-tiny",
             "--micro-batch", "1", "--seq-len", "64", "--no-graph",
             "--dump-outputs", str(out_dir), *extra],
            capture_output=True, text=True, timeout=600, env=env, cwd=repo)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        return {f.name: np.load(f) for f in sorted(Path(out_dir).iterdir())}

    a = run(tmp_path / "a")
    b = run(tmp_path / "b", "--full")
    assert sorted(a) == ["loss.npy", "master_weights_sample.npy"]
    assert sorted(b) == sorted(a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    for name in a:
        assert a[name].dtype == np.float32 and np.isfinite(a[name]).all()
        np.testing.assert_array_equal(a[name], b[name])
    assert a["loss.npy"].shape == (1,) and a["loss.npy"][0] > 0
