"""MI355X-native addition (no reference analog): Build the HIP op extension IN-TREE (modalities_amd/ops/_hip_ops.so).

Drives hipcc directly (native HIP source, no hipify) with torch's include/
lib paths; gfx950 only. The .so lands next to this file so repo snapshots
carry it to GPU boxes. Usage: python -m modalities_amd.ops.build
"""

import os
import subprocess
import sys
import sysconfig
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import torch
from torch.utils import cpp_extension

OPS_DIR = Path(__file__).parent
CSRC = OPS_DIR / "csrc"
OUT = OPS_DIR / "_hip_ops.so"

SOURCES = [
    "rms_norm.hip",
    "layer_norm.hip",
    "elementwise.hip",
    "cross_entropy.hip",
    "adamw.hip",
    "attention_fwd.hip",
    "attention_bwd.hip",
    "attention_v2.hip",
    "attention_decode.hip",
    "attention_decode_chunk.hip",
    "attention_decode_wide.hip",
    "decode_gemv.hip",
    "decode_gemv_fused.hip",
    "decode_gemv_mfma.hip",
    "decode_gemv_fp4.hip",
    "sample_logits.hip",
    "bindings.cpp",
]

# Compiled with packed fp32 arithmetic (v_pk_fma_f32 and kin) switched off
# and linked into the same library; SOURCES keep the flags they were tuned
# and validated with.
NO_PACKED_FP32_SOURCES = [
    "attention_decode_fp8.hip",
]
NO_PACKED_FP32_FLAGS = ["-Xclang", "-target-feature", "-Xclang",
                        "-packed-fp32-ops"]

HEADERS = ["common.h", "attn_common.h", "attention_decode_common.h"]

COMPILE_JOBS = 8   # hipcc processes at a time


def build_extension(verbose: bool = True, arch: str = "gfx950") -> Path:
    torch_lib = Path(torch.__file__).parent / "lib"
    includes = cpp_extension.include_paths() + [sysconfig.get_paths()["include"]]
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)

    newest_src = max((CSRC / s).stat().st_mtime
                     for s in SOURCES + NO_PACKED_FP32_SOURCES + HEADERS)
    if OUT.exists() and OUT.stat().st_mtime > newest_src:
        if verbose:
            print(f"[build] {OUT} up to date")
        return OUT

    common = (
        ["hipcc", f"--offload-arch={arch}", "-O3", "-std=c++17", "-fPIC",
         "-DTORCH_EXTENSION_NAME=_hip_ops",
         f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
         "-DUSE_ROCM=1", "-D__HIP_PLATFORM_AMD__=1",
         "-Wno-unused-result", "-fno-gpu-rdc"]
        + [f"-I{p}" for p in includes]
    )
    # One object per source, a few at a time: most of a source's compile
    # time is the host pass over the torch headers, which a single hipcc
    # call over all sources repeats one after the other.
    with tempfile.TemporaryDirectory(prefix="hip_ops_") as tmp:
        jobs = [(s, []) for s in SOURCES] \
            + [(s, NO_PACKED_FP32_FLAGS) for s in NO_PACKED_FP32_SOURCES]
        objs = [str(Path(tmp) / (Path(s).stem + ".o")) for s, _ in jobs]
        with ThreadPoolExecutor(min(COMPILE_JOBS, os.cpu_count() or 1)) as ex:
            list(ex.map(
                lambda job, obj: _run(
                    common + job[1]
                    + ["-c", "-x", "hip", str(CSRC / job[0]), "-o", obj],
                    verbose),
                jobs, objs))
        _run(common + ["-shared"] + objs
             + [f"-L{torch_lib}", "-ltorch", "-ltorch_cpu", "-ltorch_hip",
                "-lc10", "-lc10_hip", "-ltorch_python", "-lamdhip64",
                f"-Wl,-rpath,{torch_lib}", "-o", str(OUT)], verbose)
    return OUT


def _run(cmd, verbose: bool) -> None:
    if verbose:
        print("[build]", " ".join(cmd))
    result = subprocess.run(cmd, capture_output=True, text=True)
    if result.returncode != 0:
        sys.stderr.write(result.stdout[-4000:] if result.stdout else "")
        sys.stderr.write(result.stderr[-8000:] if result.stderr else "")
        raise RuntimeError(f"hipcc failed with code {result.returncode}")
    if verbose and result.stderr:
        print(result.stderr[-2000:])


if __name__ == "__main__":
    build_extension()
    print(f"built {OUT}")
