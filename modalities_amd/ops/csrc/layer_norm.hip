// K5: LayerNorm fwd/bwd for bf16 activations and parameters, f32 accumulation.
// Same kernel class as rms_norm.hip with a mean, a bias and a second column
// reduction: a row lives in the registers of LPR lanes (one wave, or a
// quarter wave for H <= 128 so that the QK-norm head dims keep all 64 lanes
// busy), is read from HBM once with bf16x8 loads (guide G13), and the
// weight/bias gradients go registers -> per-wave LDS slab -> per-block
// partial rows -> column reduce, without atomics: bit-identical run to run.
// Replaces torch's nn.LayerNorm kernels (reference: models/components/
// layer_norms.py, gpt2_model.py:923-930; the ViT and CoCa norms).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int NWAVES = BLOCK / WAVE_SIZE;
constexpr int MAX_H = 8192;
constexpr int MAX_BWD_BLOCKS = 1024;

// Sum over the LPR consecutive lanes that share a row (LPR = 16 or 64).
template <int LPR>
__device__ __forceinline__ float group_reduce_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE_SIZE);
  return v;
}

// -------- forward ----------------------------------------------------------
// y = (x - mean) * rstd * w (+ b);  rstd = rsqrt(mean((x - mean)^2) + eps).
// The variance is taken from the centred values in a second pass over the
// registers: E[x^2] - mean^2 cancels to noise far above eps on a row with a
// large offset.
template <int SLOTS, int LPR>
__global__ void __launch_bounds__(BLOCK)
layernorm_fwd_kernel(const unsigned short* __restrict__ x,
                     const unsigned short* __restrict__ w,
                     const unsigned short* __restrict__ b,  // may be null
                     unsigned short* __restrict__ y,
                     float* __restrict__ mean, float* __restrict__ rstd,
                     int H, long N, float eps) {
  constexpr int RPW = WAVE_SIZE / LPR;  // rows per wave and iteration
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  const int l = lane % LPR;
  const int sub = lane / LPR;
  const int vecH = H / 8;
  const shortx8* wv = reinterpret_cast<const shortx8*>(w);
  const shortx8* bv = reinterpret_cast<const shortx8*>(b);

  for (long base = ((long)blockIdx.x * NWAVES + wid) * RPW; base < N;
       base += (long)gridDim.x * NWAVES * RPW) {
    const long row = base + sub;
    const bool valid = row < N;  // uniform over the LPR lanes of a row
    const long roff = valid ? row * (long)H : 0;
    const shortx8* xv = reinterpret_cast<const shortx8*>(x + roff);
    shortx8* yv = reinterpret_cast<shortx8*>(y + roff);

    shortx8 xr[SLOTS];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
      const int i = l + it * LPR;
      if (valid && i < vecH) {
        xr[it] = xv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += bf16_to_f32((unsigned short)xr[it][j]);
      } else {
        xr[it] = shortx8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    const float m = group_reduce_sum<LPR>(s) / H;

    float q = 0.f;
#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
      const int i = l + it * LPR;
      if (i < vecH) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = bf16_to_f32((unsigned short)xr[it][j]) - m;
          q += d * d;
        }
      }
    }
    const float r = rsqrtf(group_reduce_sum<LPR>(q) / H + eps);
    if (valid && l == 0) {
      mean[row] = m;
      rstd[row] = r;
    }

#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
      const int i = l + it * LPR;
      if (valid && i < vecH) {
        const shortx8 wvv = wv[i];
        shortx8 bvv = shortx8{0, 0, 0, 0, 0, 0, 0, 0}, o;
        if (b != nullptr) bvv = bv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (bf16_to_f32((unsigned short)xr[it][j]) - m) * r;
          o[j] = (short)f32_to_bf16(
              xh * bf16_to_f32((unsigned short)wvv[j]) +
              bf16_to_f32((unsigned short)bvv[j]));
        }
        yv[i] = o;
      }
    }
  }
}

// -------- backward ---------------------------------------------------------
// xhat = (x - mean) * rstd, g = dy * w:
//   dx = rstd * (g - mean_j(g) - xhat * mean_j(g * xhat))
//   dw = sum_rows dy * xhat,  db = sum_rows dy

// Block-wide column sum of per-lane accumulators: every wave spills once to
// its LDS slab (the RPW rows of a quarter-wave layout are folded by shuffle
// first), then the block adds the NWAVES slabs in a fixed order into its
// partial row `out` [H].
template <int SLOTS, int LPR>
__device__ __forceinline__ void block_column_sum(const float (&acc)[SLOTS][8],
                                                 float* slab, float* out,
                                                 int H) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  const int l = lane % LPR;
  const int sub = lane / LPR;
  const int vecH = H / 8;
  float* my_slab = slab + (long)wid * H;
#pragma unroll
  for (int it = 0; it < SLOTS; ++it) {
    const int i = l + it * LPR;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = acc[it][j];
#pragma unroll
      for (int off = LPR; off < WAVE_SIZE; off <<= 1)
        v[j] += __shfl_xor(v[j], off, WAVE_SIZE);
    }
    if (sub == 0 && i < vecH) {
      floatx4* dst = reinterpret_cast<floatx4*>(my_slab + i * 8);
      dst[0] = floatx4{v[0], v[1], v[2], v[3]};
      dst[1] = floatx4{v[4], v[5], v[6], v[7]};
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += BLOCK) {
    float t = 0.f;
#pragma unroll
    for (int sl = 0; sl < NWAVES; ++sl) t += slab[(long)sl * H + i];
    out[i] = t;
  }
  __syncthreads();  // the slab is reused for the next quantity
}

template <int SLOTS, int LPR, bool HAS_BIAS>
__global__ void __launch_bounds__(BLOCK)
layernorm_bwd_kernel(const unsigned short* __restrict__ dy,
                     const unsigned short* __restrict__ x,
                     const unsigned short* __restrict__ w,
                     const float* __restrict__ mean,
                     const float* __restrict__ rstd,
                     unsigned short* __restrict__ dx,
                     float* __restrict__ part,  // [1 + HAS_BIAS, nblocks, H]
                     int H, long N, int rows_per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* slab = reinterpret_cast<float*>(smem_raw);  // [NWAVES, H]
  constexpr int RPW = WAVE_SIZE / LPR;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  const int l = lane % LPR;
  const int sub = lane / LPR;
  const int vecH = H / 8;

  const long row0 = (long)blockIdx.x * rows_per_block;
  const long row1 = min(row0 + rows_per_block, N);

  // Lane l of a row group always owns vec8 columns {l, l+LPR, ...}: its dw
  // and db partials stay in registers over the whole row loop.
  float dwacc[SLOTS][8];
  float dbacc[HAS_BIAS ? SLOTS : 1][8];
#pragma unroll
  for (int it = 0; it < SLOTS; ++it)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dwacc[it][j] = 0.f;
      if (HAS_BIAS) dbacc[HAS_BIAS ? it : 0][j] = 0.f;
    }

  const shortx8* wv = reinterpret_cast<const shortx8*>(w);
  for (long base = row0 + (long)wid * RPW; base < row1;
       base += (long)NWAVES * RPW) {
    const long row = base + sub;
    const bool valid = row < row1;  // uniform over the LPR lanes of a row
    const long roff = valid ? row * (long)H : 0;
    const shortx8* xv = reinterpret_cast<const shortx8*>(x + roff);
    const shortx8* dyv = reinterpret_cast<const shortx8*>(dy + roff);
    shortx8* dxv = reinterpret_cast<shortx8*>(dx + roff);
    const float m = valid ? mean[row] : 0.f;
    const float r = valid ? rstd[row] : 0.f;

    shortx8 xr[SLOTS], dyr[SLOTS];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
      const int i = l + it * LPR;
      if (valid && i < vecH) {
        xr[it] = xv[i];
        dyr[it] = dyv[i];
        const shortx8 wvv = wv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (bf16_to_f32((unsigned short)xr[it][j]) - m) * r;
          const float g = bf16_to_f32((unsigned short)dyr[it][j]) *
                          bf16_to_f32((unsigned short)wvv[j]);
          sg += g;
          sgx += g * xh;
        }
      } else {
        xr[it] = shortx8{0, 0, 0, 0, 0, 0, 0, 0};
        dyr[it] = shortx8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    const float c1 = group_reduce_sum<LPR>(sg) / H;
    const float c2 = group_reduce_sum<LPR>(sgx) / H;

#pragma unroll
    for (int it = 0; it < SLOTS; ++it) {
      const int i = l + it * LPR;
      if (valid && i < vecH) {
        const shortx8 wvv = wv[i];
        shortx8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (bf16_to_f32((unsigned short)xr[it][j]) - m) * r;
          const float dyf = bf16_to_f32((unsigned short)dyr[it][j]);
          const float g = dyf * bf16_to_f32((unsigned short)wvv[j]);
          o[j] = (short)f32_to_bf16(r * (g - c1 - xh * c2));
          dwacc[it][j] += dyf * xh;
          if (HAS_BIAS) dbacc[HAS_BIAS ? it : 0][j] += dyf;
        }
        dxv[i] = o;
      }
    }
  }

  const long nblocks = gridDim.x;
  block_column_sum<SLOTS, LPR>(dwacc, slab, part + (long)blockIdx.x * H, H);
  if constexpr (HAS_BIAS)
    block_column_sum<SLOTS, LPR>(dbacc, slab,
                                 part + (nblocks + blockIdx.x) * H, H);
}

// Column reduce of part [nsets, nrows, H] -> out [nsets, H]. 32 columns x 8
// row groups per block; the 8 group sums are added in a fixed order, so the
// result does not depend on scheduling. grid = (ceil(H / 32), nsets).
constexpr int RED_COLS = 32;
constexpr int RED_GROUPS = BLOCK / RED_COLS;

__global__ void __launch_bounds__(BLOCK)
column_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                     int H, int nrows) {
  __shared__ float sm[RED_GROUPS][RED_COLS];
  const int c = threadIdx.x % RED_COLS;
  const int rg = threadIdx.x / RED_COLS;
  const int col = blockIdx.x * RED_COLS + c;
  const float* p = part + (long)blockIdx.y * nrows * H;
  float acc = 0.f;
  if (col < H)
    for (int r = rg; r < nrows; r += RED_GROUPS) acc += p[(long)r * H + col];
  sm[rg][c] = acc;
  __syncthreads();
  if (rg == 0 && col < H) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < RED_GROUPS; ++k) t += sm[k][c];
    out[(long)blockIdx.y * H + col] = t;
  }
}

void check_row_size(int H, const char* fn) {
  TORCH_CHECK(H >= 8 && H % 8 == 0, fn, ": H must be a positive multiple of 8");
  TORCH_CHECK(H <= MAX_H, fn, ": H too large (max ", MAX_H, ")");
}

// Rows are read with 16-byte loads: H % 8 == 0 keeps every row aligned only
// if the base is. A contiguous view at an odd element offset is not.
void check_aligned(const torch::Tensor& t, const char* fn, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, fn, ": ",
              name, " must be 16-byte aligned");
}

}  // namespace

long layernorm_max_h() { return MAX_H; }

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         c10::optional<torch::Tensor> b,
                                         double eps) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2
              && x.is_contiguous() && x.size(0) >= 1,
              "layernorm_fwd: x must be contiguous device bf16 [N,H], N >= 1");
  const long N = x.size(0);
  TORCH_CHECK(x.size(1) <= MAX_H, "layernorm_fwd: H too large (max ", MAX_H, ")");
  const int H = (int)x.size(1);
  check_row_size(H, "layernorm_fwd");
  TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kBFloat16
              && w.is_contiguous() && w.dim() == 1 && w.numel() == H
              && w.device() == x.device(),
              "layernorm_fwd: w must be contiguous device bf16 [H]");
  const bool has_bias = b.has_value() && b->defined();
  if (has_bias)
    TORCH_CHECK(b->is_cuda() && b->dtype() == torch::kBFloat16
                && b->is_contiguous() && b->dim() == 1 && b->numel() == H
                && b->device() == x.device(),
                "layernorm_fwd: b must be contiguous device bf16 [H]");
  check_aligned(x, "layernorm_fwd", "x");
  check_aligned(w, "layernorm_fwd", "w");
  if (has_bias) check_aligned(*b, "layernorm_fwd", "b");
  auto y = torch::empty_like(x);
  auto mean = torch::empty({N}, x.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({N}, x.options().dtype(torch::kFloat32));
  const int vecH = H / 8;
  const int rpw = vecH <= 16 ? 4 : 1;
  const long rows_per_iter = (long)NWAVES * rpw;
  const int nblocks = (int)min((long)8192, (N + rows_per_iter - 1) / rows_per_iter);
  const int slots = (vecH + WAVE_SIZE - 1) / WAVE_SIZE;
  auto stream = at::cuda::getCurrentHIPStream();
  auto launch = [&](auto* kfn) {
    hipLaunchKernelGGL(kfn, dim3(nblocks), dim3(BLOCK), 0, stream,
                       (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)w.data_ptr(),
                       has_bias ? (const unsigned short*)b->data_ptr() : nullptr,
                       (unsigned short*)y.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), H, N, (float)eps);
  };
  if (vecH <= 16) launch(layernorm_fwd_kernel<1, 16>);
  else if (slots <= 1) launch(layernorm_fwd_kernel<1, 64>);
  else if (slots <= 2) launch(layernorm_fwd_kernel<2, 64>);
  else if (slots <= 5) launch(layernorm_fwd_kernel<5, 64>);
  else if (slots <= 8) launch(layernorm_fwd_kernel<8, 64>);
  else launch(layernorm_fwd_kernel<16, 64>);
  HIP_CHECK_KERNEL();
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd, bool has_bias) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 2
              && x.is_contiguous() && x.size(0) >= 1,
              "layernorm_bwd: x must be contiguous device bf16 [N,H], N >= 1");
  const long N = x.size(0);
  TORCH_CHECK(x.size(1) <= MAX_H, "layernorm_bwd: H too large (max ", MAX_H, ")");
  const int H = (int)x.size(1);
  check_row_size(H, "layernorm_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.dtype() == torch::kBFloat16
              && dy.is_contiguous() && dy.dim() == 2 && dy.size(0) == N
              && dy.size(1) == H && dy.device() == x.device(),
              "layernorm_bwd: dy must be contiguous device bf16 [N,H]");
  TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kBFloat16
              && w.is_contiguous() && w.dim() == 1 && w.numel() == H
              && w.device() == x.device(),
              "layernorm_bwd: w must be contiguous device bf16 [H]");
  TORCH_CHECK(mean.is_cuda() && mean.dtype() == torch::kFloat32
              && mean.is_contiguous() && mean.dim() == 1 && mean.numel() == N
              && mean.device() == x.device(),
              "layernorm_bwd: mean must be contiguous device fp32 [N]");
  TORCH_CHECK(rstd.is_cuda() && rstd.dtype() == torch::kFloat32
              && rstd.is_contiguous() && rstd.dim() == 1 && rstd.numel() == N
              && rstd.device() == x.device(),
              "layernorm_bwd: rstd must be contiguous device fp32 [N]");
  check_aligned(x, "layernorm_bwd", "x");
  check_aligned(dy, "layernorm_bwd", "dy");
  check_aligned(w, "layernorm_bwd", "w");
  const int vecH = H / 8;
  const int rpw = vecH <= 16 ? 4 : 1;
  const long rows_per_iter = (long)NWAVES * rpw;
  // Few, equally loaded blocks: every block writes a partial row per
  // quantity, so their count is the price of the deterministic reduce.
  long nb = min((long)MAX_BWD_BLOCKS, (N + rows_per_iter - 1) / rows_per_iter);
  long rpb = (N + nb - 1) / nb;
  rpb = (rpb + rows_per_iter - 1) / rows_per_iter * rows_per_iter;
  TORCH_CHECK(rpb <= INT_MAX, "layernorm_bwd: too many rows");
  const int rows_per_block = (int)rpb;
  const int nblocks = (int)((N + rpb - 1) / rpb);
  const int nsets = has_bias ? 2 : 1;
  const size_t smem = (size_t)H * NWAVES * sizeof(float);  // <= 128 KiB
  const int slots = (vecH + WAVE_SIZE - 1) / WAVE_SIZE;

  auto f32 = x.options().dtype(torch::kFloat32);
  auto dx = torch::empty_like(x);
  auto part = torch::empty({(long)nsets, (long)nblocks, (long)H}, f32);
  auto dwdb = torch::empty({(long)nsets, (long)H}, f32);
  auto stream = at::cuda::getCurrentHIPStream();
  auto launch = [&](auto* kfn) {
    hipLaunchKernelGGL(kfn, dim3(nblocks), dim3(BLOCK), smem, stream,
                       (const unsigned short*)dy.data_ptr(),
                       (const unsigned short*)x.data_ptr(),
                       (const unsigned short*)w.data_ptr(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       (unsigned short*)dx.data_ptr(), part.data_ptr<float>(),
                       H, N, rows_per_block);
  };
#define LN_BWD_LAUNCH(S, L)                                      \
  do {                                                           \
    if (has_bias) launch(layernorm_bwd_kernel<S, L, true>);      \
    else launch(layernorm_bwd_kernel<S, L, false>);              \
  } while (0)
  if (vecH <= 16) LN_BWD_LAUNCH(1, 16);
  else if (slots <= 1) LN_BWD_LAUNCH(1, 64);
  else if (slots <= 2) LN_BWD_LAUNCH(2, 64);
  else if (slots <= 5) LN_BWD_LAUNCH(5, 64);
  else if (slots <= 8) LN_BWD_LAUNCH(8, 64);
  else LN_BWD_LAUNCH(16, 64);
#undef LN_BWD_LAUNCH
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL(column_reduce_kernel,
                     dim3((H + RED_COLS - 1) / RED_COLS, nsets), dim3(BLOCK),
                     0, stream, part.data_ptr<float>(),
                     dwdb.data_ptr<float>(), H, nblocks);
  HIP_CHECK_KERNEL();
  auto db = has_bias ? dwdb[1] : torch::empty({0}, f32);
  return {dx, dwdb[0], db};
}
