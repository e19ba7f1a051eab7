"""MI355X-native op library: HIP/CDNA4 kernels with torch reference fallbacks.

Replaces the dependency-provided kernels the reference framework leans on
(reference: SURVEY.md §2.4 K1-K11 — flash-attn wheel, cuBLAS epilogues,
torch SDPA/LayerNorm/CE/AdamW) with hand-written gfx950 HIP kernels:

- K1  flash_attention   : MFMA/LDS-tiled causal attention fwd+bwd, GQA-aware,
                          optional per-document mask for packed sequences;
                          split-KV single-token decode over a KV cache with
                          a fused RoPE + cache append; the same over an
                          e4m3 KV cache with per-(token, kv head) power-of-two
                          scales (quantize_kv_fp8, kv_quantize_store, and
                          k_scale / v_scale on the two decode ops): D + 4
                          bytes per cached row instead of 2 D; MFMA split-KV
                          attention of a few new tokens per row over either
                          cache format (decode_attention with T >= 2), and
                          from 128 query rows per kv head a variant that
                          stages the keys through LDS once per 64 rows
                          (long chunks: chunked prefill, multi-turn chat)
- K3  skinny_linear     : M <= 8 decode GEMM streaming bf16 or weight-only
                          e4m3 weights straight to registers; optionally with
                          an RMSNorm prologue, a SwiGLU gate and a residual
                          add fused in (norm_weight / glu / residual;
                          set_decode_fused_step turns them on for the model)
- K3  skinny_linear_mfma: the same for M <= 32 on the matrix cores (MFMA),
                          e4m3 widened to bf16 in registers
- K3  skinny_linear_mxfp4: M <= 32 decode GEMM on MXFP4 weights (e2m1 codes,
                          one e8m0 scale per 32 k; 0.53 bytes per weight):
                          v_cvt_scalef32_pk_bf16_fp4 widens a byte to two
                          scaled bf16 values that feed the MFMA directly
                          (quantize_weight_mxfp4 / dequantize_weight_mxfp4)
- K3  sample_logits     : temperature / top-k / top-p token sampler on the
                          logits row, radix selects instead of a sort; one
                          launch, capturable into the decode graph
- K4  rope              : fused rotate-half RoPE on q,k
- K5  rms_norm          : wave-level reduction norm fwd+bwd
- K5  layer_norm        : register-resident row LayerNorm fwd+bwd (bf16)
- K6  silu_mul          : SwiGLU gate epilogue
- K8  cross_entropy     : fused log-softmax + NLL over the vocab
- K9  fused_adamw       : multi-tensor AdamW update
- K10 grad norm/clip    : multi-tensor L2 norm + scale

Dispatch policy: on ROCm devices the HIP extension is REQUIRED — a CUDA
(ROCm) tensor reaching an op without the extension raises, so GPU runs can
never silently fall back to eager PyTorch. On CPU the ops run a plain
PyTorch implementation (used for tests and as the numerics reference).
"""

from modalities_amd.ops.backend import (  # noqa: F401
    hip_available,
    hip_ext,
    require_hip,
)
from modalities_amd.ops.rms_norm import rms_norm  # noqa: F401
from modalities_amd.ops.layer_norm import LayerNorm, layer_norm  # noqa: F401
from modalities_amd.ops.rope import precompute_rope_cos_sin, rope_apply  # noqa: F401
from modalities_amd.ops.swiglu import silu_mul, silu_mul_joint  # noqa: F401
from modalities_amd.ops.cross_entropy import fused_cross_entropy  # noqa: F401
from modalities_amd.ops.attention import document_starts, flash_attention  # noqa: F401
from modalities_amd.ops.attention import (  # noqa: F401
    decode_attention,
    decode_attention_enabled,
    decode_chunk_tokens,
    decode_rope_append,
    dequantize_kv_fp8,
    kv_quantize_store,
    quantize_kv_fp8,
    set_decode_attention,
    set_decode_chunk_tokens,
)
from modalities_amd.ops.adamw import fused_adamw_step  # noqa: F401
from modalities_amd.ops.decode_linear import (  # noqa: F401
    decode_fused_step,
    dequantize_weight_mxfp4,
    set_decode_fused_step,
    quantize_weight_fp8,
    quantize_weight_mxfp4,
    set_decode_mfma_min_rows,
    skinny_linear,
    skinny_linear_mfma,
    skinny_linear_mxfp4,
)
from modalities_amd.ops.sampling import sample_logits  # noqa: F401
