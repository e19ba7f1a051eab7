// K9 fused AdamW on flat fp32 shards (+ per-element weight-decay mask for
// the flat-shard equivalent of weight-decay groups) and K10 multi-tensor
// L2-norm / scale. Replaces torch.optim.AdamW(fused=True)
// (reference: optimizers/optimizer_factory.py:38-50) and
// clip_grads_with_norm_ (fsdp_gradient_clipper.py:144-229).
//
// The device-step AdamW and the sum of squares each have ONE body,
// instantiated for two input forms:
//   <float grad, fp32 mask>    what any caller may hand in (fractional
//                              masks, grads accumulated in fp32): 34 B/elem
//   <bf16 grad, packed mask>   the engine's single-micro-batch fast path:
//                              the reduced bf16 gradient is read where the
//                              backward left it (no fp32 copy) and the
//                              decay mask is one bit per element:
//                              28.125 B/elem
// bf16 -> fp32 is exact and the per-element expressions are shared, so the
// two forms give bit-identical p, m, v and bf16 copy from equal values.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

// p, g, m, v, wd_mask: flat fp32; vectorized f32x4.
__global__ void adamw_masked_kernel(float* __restrict__ p,
                                    const float* __restrict__ g,
                                    float* __restrict__ m,
                                    float* __restrict__ v,
                                    const float* __restrict__ wd_mask,
                                    long n4, float lr, float beta1, float beta2,
                                    float eps, float wd, float bc1, float bc2) {
  const float step_size = lr / bc1;
  const float inv_bc2 = 1.0f / bc2;
  floatx4* p4 = reinterpret_cast<floatx4*>(p);
  const floatx4* g4 = reinterpret_cast<const floatx4*>(g);
  floatx4* m4 = reinterpret_cast<floatx4*>(m);
  floatx4* v4 = reinterpret_cast<floatx4*>(v);
  const floatx4* w4 = reinterpret_cast<const floatx4*>(wd_mask);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    floatx4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i], ww = w4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pp[j] *= (1.0f - lr * wd * ww[j]);
      mm[j] = beta1 * mm[j] + (1.0f - beta1) * gg[j];
      vv[j] = beta2 * vv[j] + (1.0f - beta2) * gg[j] * gg[j];
      pp[j] -= step_size * mm[j] / (sqrtf(vv[j] * inv_bc2) + eps);
    }
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
  }
}

// 1 - beta^t to a few fp32 ulps. 1.0f - __powf(beta, t) loses it twice: the
// fast pow is only accurate to ~1e-6 near 1, and beta^t itself cannot be
// held in fp32 to better than 2^-25 absolute, which is a relative error of
// 2^-25 * beta^t / (1 - beta^t) in the result (1.5e-5 at beta2 = 0.999,
// t = 2). -expm1(t * log(beta)) never forms beta^t. Once per thread.
__device__ __forceinline__ float bias_correction(float beta, float t) {
  return -expm1f(t * logf(beta));
}

// Elements 4i..4i+3 of a gradient, as the fp32 values the update consumes.
// fp32: as stored. bf16: 8 bytes per lane, widened (exact) and multiplied
// by gmul, the 1/world factor the fp32 copy used to carry.
__device__ __forceinline__ floatx4 load_grad4(const float* g, long i, float) {
  return reinterpret_cast<const floatx4*>(g)[i];
}

__device__ __forceinline__ floatx4 load_grad4(const unsigned short* g, long i,
                                              float gmul) {
  const shortx4 h = reinterpret_cast<const shortx4*>(g)[i];
  floatx4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = bf16_to_f32((unsigned short)h[j]) * gmul;
  return r;
}

// Decay mask of elements 4i..4i+3. fp32: as stored (any value). Packed:
// bit j of byte k is element 8k + j, so float4 i is the low or the high
// nibble of byte i / 2; two neighbouring lanes read the same byte.
__device__ __forceinline__ floatx4 load_mask4(const float* w, long i) {
  return reinterpret_cast<const floatx4*>(w)[i];
}

__device__ __forceinline__ floatx4 load_mask4(const unsigned char* bits,
                                              long i) {
  const unsigned b = (unsigned)bits[i >> 1] >> ((unsigned)(i & 1) * 4u);
  floatx4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = ((b >> j) & 1u) ? 1.0f : 0.0f;
  return r;
}

// Graph-safe variant: the Adam step count lives in DEVICE memory so a
// hipGraph replay of the training step sees the advancing bias correction
// (a host-side bc baked into kernel args would be frozen at capture).
// Also writes the bf16 working copy (bf16_out) in the same pass — fusing
// the publish cast saves a full fp32 re-read + bf16 write of the params.
// G: float or unsigned short (bf16 bits); W: float mask or packed bits.
// The 1x float4 grid-stride shape measured best (320M elems: 5.6 TB/s,
// against 5.1 and 3.9 for 2 and 4 float4 per thread).
template <typename G, typename W>
__global__ void adamw_devstep_kernel(float* __restrict__ p,
                                     const G* __restrict__ g, float gmul,
                                     float* __restrict__ m,
                                     float* __restrict__ v,
                                     const W* __restrict__ wd_mask,
                                     const int* __restrict__ step,
                                     unsigned short* __restrict__ bf16_out,
                                     const float* __restrict__ gscale,
                                     long n4, float lr, float beta1,
                                     float beta2, float eps, float wd) {
  // gscale (device scalar, e.g. the grad-clip coefficient) is folded into
  // the grad read here — saves the separate full read+write scale pass
  // over every grad shard that multi_tensor_scale_ would cost.
  const float gs = gscale ? *gscale : 1.0f;
  const float t = (float)*step;
  const float bc1 = bias_correction(beta1, t);
  const float bc2 = bias_correction(beta2, t);
  const float step_size = lr / bc1;
  const float inv_bc2 = 1.0f / bc2;
  floatx4* p4 = reinterpret_cast<floatx4*>(p);
  floatx4* m4 = reinterpret_cast<floatx4*>(m);
  floatx4* v4 = reinterpret_cast<floatx4*>(v);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    floatx4 pp = p4[i], mm = m4[i], vv = v4[i];
    const floatx4 gg = load_grad4(g, i, gmul);
    const floatx4 ww = load_mask4(wd_mask, i);
    shortx4 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = gg[j] * gs;
      pp[j] *= (1.0f - lr * wd * ww[j]);
      mm[j] = beta1 * mm[j] + (1.0f - beta1) * gj;
      vv[j] = beta2 * vv[j] + (1.0f - beta2) * gj * gj;
      pp[j] -= step_size * mm[j] / (sqrtf(vv[j] * inv_bc2) + eps);
      h[j] = (short)f32_to_bf16(pp[j]);
    }
    p4[i] = pp; m4[i] = mm; v4[i] = vv;
    reinterpret_cast<shortx4*>(bf16_out)[i] = h;
  }
}

template <typename G>
__global__ void sqsum_kernel(const G* __restrict__ x, float gmul, long n4,
                             float* __restrict__ out) {
  __shared__ float scratch[256 / WAVE_SIZE];
  float acc = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    floatx4 v = load_grad4(x, i, gmul);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += v[j] * v[j];
  }
  acc = block_reduce_sum(acc, scratch);
  if (threadIdx.x == 0) atomicAdd(out, acc);
}

__global__ void scale_kernel(float* __restrict__ x, long n4,
                             const float* __restrict__ scale) {
  const float s = *scale;
  floatx4* x4 = reinterpret_cast<floatx4*>(x);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    floatx4 v = x4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] *= s;
    x4[i] = v;
  }
}

int grid_for(long work, int block) {
  long g = (work + block - 1) / block;
  return (int)min(g, (long)(256 * 8));
}

// t is a contiguous device fp32 tensor with as many elements as ref
bool f32_like(const torch::Tensor& t, const torch::Tensor& ref) {
  return t.is_cuda() && t.dtype() == torch::kFloat32 && t.is_contiguous()
      && t.numel() == ref.numel() && t.device() == ref.device();
}

const float* gscale_ptr(const c10::optional<torch::Tensor>& gscale) {
  if (!gscale.has_value()) return nullptr;
  TORCH_CHECK(gscale->is_cuda() && gscale->dtype() == torch::kFloat32
              && gscale->numel() == 1, "gscale must be a cuda fp32 scalar");
  return gscale->data_ptr<float>();
}

}  // namespace

void fused_adamw_masked(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                        torch::Tensor v, torch::Tensor wd_mask, double lr,
                        double beta1, double beta2, double eps, double wd,
                        double bc1, double bc2) {
  TORCH_CHECK(p.is_cuda() && p.dtype() == torch::kFloat32 && p.is_contiguous());
  TORCH_CHECK(p.numel() % 4 == 0, "flat shard must be divisible by 4");
  TORCH_CHECK(f32_like(g, p) && f32_like(m, p) && f32_like(v, p)
              && f32_like(wd_mask, p),
              "g, m, v, wd_mask must match p (device fp32, contiguous)");
  long n4 = p.numel() / 4;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(adamw_masked_kernel, dim3(grid_for(n4, 256)), dim3(256), 0,
                     stream, p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     wd_mask.data_ptr<float>(), n4, (float)lr, (float)beta1,
                     (float)beta2, (float)eps, (float)wd, (float)bc1, (float)bc2);
  HIP_CHECK_KERNEL();
}

void fused_adamw_masked_devstep(torch::Tensor p, torch::Tensor g,
                                torch::Tensor m, torch::Tensor v,
                                torch::Tensor wd_mask, torch::Tensor step,
                                torch::Tensor bf16_out,
                                c10::optional<torch::Tensor> gscale, double lr,
                                double beta1, double beta2, double eps,
                                double wd) {
  const float* gs_ptr = gscale_ptr(gscale);
  TORCH_CHECK(p.is_cuda() && p.dtype() == torch::kFloat32 && p.is_contiguous());
  TORCH_CHECK(p.numel() % 4 == 0, "flat shard must be divisible by 4");
  TORCH_CHECK(f32_like(g, p) && f32_like(m, p) && f32_like(v, p)
              && f32_like(wd_mask, p),
              "g, m, v, wd_mask must match p (device fp32, contiguous)");
  TORCH_CHECK(step.is_cuda() && step.dtype() == torch::kInt32
              && step.numel() == 1);
  TORCH_CHECK(bf16_out.is_cuda() && bf16_out.dtype() == torch::kBFloat16
              && bf16_out.is_contiguous() && bf16_out.numel() == p.numel());
  long n4 = p.numel() / 4;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((adamw_devstep_kernel<float, float>),
                     dim3(grid_for(n4, 256)), dim3(256), 0, stream,
                     p.data_ptr<float>(), g.data_ptr<float>(), 1.0f,
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     wd_mask.data_ptr<float>(), step.data_ptr<int>(),
                     (unsigned short*)bf16_out.data_ptr(), gs_ptr, n4,
                     (float)lr, (float)beta1, (float)beta2, (float)eps,
                     (float)wd);
  HIP_CHECK_KERNEL();
}

// The fast path of the sharded engine: g is the reduced bf16 gradient as the
// backward left it, used as float(g) * gmul (then * gscale); wd_bits holds
// the 0/1 decay mask, bit j of byte i for element 8i + j.
void fused_adamw_devstep_bf16g(torch::Tensor p, torch::Tensor g, double gmul,
                               torch::Tensor m, torch::Tensor v,
                               torch::Tensor wd_bits, torch::Tensor step,
                               torch::Tensor bf16_out,
                               c10::optional<torch::Tensor> gscale, double lr,
                               double beta1, double beta2, double eps,
                               double wd) {
  const float* gs_ptr = gscale_ptr(gscale);
  TORCH_CHECK(p.is_cuda() && p.dtype() == torch::kFloat32 && p.is_contiguous());
  TORCH_CHECK(p.numel() % 8 == 0,
              "flat shard must be divisible by 8 (one mask byte per 8)");
  TORCH_CHECK(f32_like(m, p) && f32_like(v, p),
              "m, v must match p (device fp32, contiguous)");
  TORCH_CHECK(g.is_cuda() && g.dtype() == torch::kBFloat16 && g.is_contiguous()
              && g.numel() == p.numel() && g.device() == p.device(),
              "g must be a contiguous device bf16 tensor of p's size");
  TORCH_CHECK(wd_bits.is_cuda() && wd_bits.dtype() == torch::kUInt8
              && wd_bits.is_contiguous() && wd_bits.numel() * 8 == p.numel()
              && wd_bits.device() == p.device(),
              "wd_bits must be a contiguous device uint8 tensor of "
              "p.numel() / 8 bytes");
  TORCH_CHECK(step.is_cuda() && step.dtype() == torch::kInt32
              && step.numel() == 1);
  TORCH_CHECK(bf16_out.is_cuda() && bf16_out.dtype() == torch::kBFloat16
              && bf16_out.is_contiguous() && bf16_out.numel() == p.numel());
  long n4 = p.numel() / 4;
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL((adamw_devstep_kernel<unsigned short, unsigned char>),
                     dim3(grid_for(n4, 256)), dim3(256), 0, stream,
                     p.data_ptr<float>(),
                     (const unsigned short*)g.data_ptr(), (float)gmul,
                     m.data_ptr<float>(), v.data_ptr<float>(),
                     wd_bits.data_ptr<unsigned char>(), step.data_ptr<int>(),
                     (unsigned short*)bf16_out.data_ptr(), gs_ptr, n4,
                     (float)lr, (float)beta1, (float)beta2, (float)eps,
                     (float)wd);
  HIP_CHECK_KERNEL();
}

void fused_adamw(std::vector<torch::Tensor> ps, std::vector<torch::Tensor> gs,
                 std::vector<torch::Tensor> ms, std::vector<torch::Tensor> vs,
                 double lr, double beta1, double beta2, double eps, double wd,
                 double bc1, double bc2) {
  TORCH_CHECK(gs.size() == ps.size() && ms.size() == ps.size()
              && vs.size() == ps.size(), "fused_adamw: list lengths differ");
  for (size_t i = 0; i < ps.size(); ++i) {
    auto ones = torch::ones_like(ps[i]);
    fused_adamw_masked(ps[i], gs[i], ms[i], vs[i], ones, lr, beta1, beta2, eps,
                       wd, bc1, bc2);
  }
}

torch::Tensor multi_tensor_sqsum(std::vector<torch::Tensor> tensors) {
  TORCH_CHECK(!tensors.empty());
  auto out = torch::zeros({}, tensors[0].options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentHIPStream();
  for (auto& t : tensors) {
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32
                && t.is_contiguous() && t.numel() % 4 == 0);
    long n4 = t.numel() / 4;
    hipLaunchKernelGGL(sqsum_kernel<float>, dim3(grid_for(n4, 256)), dim3(256),
                       0, stream, t.data_ptr<float>(), 1.0f, n4,
                       out.data_ptr<float>());
    HIP_CHECK_KERNEL();
  }
  return out;
}

// sum over every tensor of (float(g) * gmul)^2: the norm of pending bf16
// gradients without their fp32 copy. numel % 8 as the AdamW that follows.
torch::Tensor multi_tensor_sqsum_bf16(std::vector<torch::Tensor> tensors,
                                      double gmul) {
  TORCH_CHECK(!tensors.empty());
  for (auto& t : tensors)
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16
                && t.is_contiguous() && t.numel() % 8 == 0
                && t.device() == tensors[0].device(),
                "multi_tensor_sqsum_bf16: tensors must be contiguous device "
                "bf16 with numel % 8 == 0");
  auto out = torch::zeros({}, tensors[0].options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentHIPStream();
  for (auto& t : tensors) {
    long n4 = t.numel() / 4;
    hipLaunchKernelGGL(sqsum_kernel<unsigned short>, dim3(grid_for(n4, 256)),
                       dim3(256), 0, stream,
                       (const unsigned short*)t.data_ptr(), (float)gmul, n4,
                       out.data_ptr<float>());
    HIP_CHECK_KERNEL();
  }
  return out;
}

void multi_tensor_scale(std::vector<torch::Tensor> tensors, torch::Tensor scale) {
  // scale stays on device (hipGraph-capture-safe): a host scalar is an error
  TORCH_CHECK(scale.is_cuda() && scale.numel() == 1,
              "multi_tensor_scale: scale must be a device scalar");
  // a tail of numel % 4 elements would be left unscaled: reject, like
  // multi_tensor_sqsum and the AdamW kernels (shards are padded). All
  // tensors are validated before the first launch.
  for (auto& t : tensors)
    TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32
                && t.is_contiguous() && t.numel() % 4 == 0,
                "multi_tensor_scale: tensors must be contiguous device fp32 "
                "with numel % 4 == 0");
  auto stream = at::cuda::getCurrentHIPStream();
  auto s = scale.to(torch::kFloat32).contiguous();
  for (auto& t : tensors) {
    long n4 = t.numel() / 4;
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n4, 256)), dim3(256), 0,
                       stream, t.data_ptr<float>(), n4, s.data_ptr<float>());
    HIP_CHECK_KERNEL();
  }
}
