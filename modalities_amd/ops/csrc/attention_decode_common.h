// What the bf16 decode kernels (attention_decode.hip) and the FP8-cache ones
// (attention_decode_fp8.hip) share: the launch constants, the combine
// kernel over the fp32 (m, l, acc) partials, and the argument checks.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_WAVES = DEC_THREADS / WAVE_SIZE;
constexpr int DEC_UNROLL = 4;
constexpr int DEC_KV_CHUNK = 256;      // default keys per workgroup
constexpr int DEC_KV_CHUNK_MIN = 16;   // smallest override (and its multiple)

__device__ __forceinline__ float dec_weight(float m, float m_new) {
  // exp2(m - m_new) with the empty state (m = -inf) weighing nothing, also
  // when m_new is -inf as well
  return m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - m_new);
}

template <int D>
__global__ __launch_bounds__(128)
void decode_combine_kernel(const float* __restrict__ ws_ml,
                           const float* __restrict__ ws_acc,
                           const int* __restrict__ kv_lens,
                           unsigned short* __restrict__ o,
                           float* __restrict__ lse,
                           int Lmax, int Hq, int chunk, int NC) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int len = kv_lens[b];
  len = min(max(len, 0), Lmax);
  const int ncl = (len + chunk - 1) / chunk;   // chunks that hold keys, <= NC
  const long base = ((long)b * Hq + h) * NC;
  float mx = -INFINITY;
  for (int s = 0; s < ncl; ++s) mx = fmaxf(mx, ws_ml[(base + s) * 2]);
  float lsum = 0.f, a = 0.f;
  for (int s = 0; s < ncl; ++s) {
    const float wt = dec_weight(ws_ml[(base + s) * 2], mx);
    lsum += ws_ml[(base + s) * 2 + 1] * wt;
    if (d < D) a += ws_acc[(base + s) * D + d] * wt;
  }
  if (d < D)
    o[((long)b * Hq + h) * D + d] = f32_to_bf16(ncl > 0 ? a / lsum : 0.f);
  if (d == 0)
    lse[(long)b * Hq + h] =
        ncl > 0 ? (mx + log2f(lsum)) * 0.69314718056f : -INFINITY;
}

// x: bf16 [B, 1, H, D] whose heads are contiguous; rows may be strided
// (a view into a fused-QKV projection output)
[[maybe_unused]] bool token_ok(const torch::Tensor& x, long B, long H,
                               long D) {
  return x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 4
      && x.size(0) == B && x.size(1) == 1 && x.size(2) == H && x.size(3) == D
      && x.stride(3) == 1 && (H == 1 || x.stride(2) == D);
}

// every offset of the first ndims dimensions a multiple of `elems` elements,
// base aligned accordingly
[[maybe_unused]] bool strides_aligned(const torch::Tensor& x, int ndims,
                                      long elems) {
  if (reinterpret_cast<uintptr_t>(x.data_ptr())
      % (x.element_size() * elems) != 0)
    return false;
  for (int i = 0; i < ndims; ++i)
    if (x.size(i) > 1 && x.stride(i) % elems != 0) return false;
  return true;
}

// t is a contiguous device fp32 [>= T, D/2] cos or sin table
[[maybe_unused]] bool table_ok(const torch::Tensor& t, long T, long D) {
  return t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 2
      && t.is_contiguous() && t.size(0) >= T && t.size(1) == D / 2;
}

[[maybe_unused]] bool index_ok(const torch::Tensor& t,
                               const torch::Tensor& ref, long B) {
  return t.is_cuda() && t.device() == ref.device()
      && t.dtype() == torch::kInt32 && t.dim() == 1 && t.size(0) == B
      && t.is_contiguous();
}

}  // namespace
