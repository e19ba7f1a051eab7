// Fused variant of the VALU skinny GEMM (decode_gemv.hip) for single-token
// decoding, 1 <= M <= 8, e4m3 or bf16 weights. Three independent options fold
// the elementwise kernels that sit next to a decode GEMM into it:
//
// skinny_linear_fused(x [M,K] bf16, w [N,K] e4m3 | bf16, scale fp32 [N] | None,
//                     bias bf16 [N] | None, norm_weight bf16 [K] | None, eps,
//                     residual bf16 [M,N_out] | None, glu) -> y [M,N_out] bf16
//
//  * NORM (RMSNorm prologue): x is the raw residual stream and
//        acc[m, n] = inv[m] * sum_k (x[m, k] * g[k]) * w[n, k],
//        inv[m] = rsqrt(mean_k x[m, k]^2 + eps).
//    A wave walks the whole K range of its rows, so it meets every x element
//    exactly once: the sum of squares rides on the x pieces the wave loads
//    anyway (main loop, tail passes and the predicated last pass, where a lane
//    without a chunk runs nothing and adds nothing). x * g is formed once per
//    x piece (fp32, unrounded) and reused by the wave's R weight rows; g
//    pieces are 16-byte loads next to the x pieces (L1/L2). inv[m] is applied
//    once per output in the epilogue. A normalised x is never written.
//    Order of the sum of squares of a row, fixed: a lane adds its elements in
//    ascending k into one (even, odd) pair, even + odd, then the xor tree.
//    Neither R, U, MT nor the row's place enters it, so inv[m], and with it y,
//    is bit-identical for every M and every position.
//  * GLU (SwiGLU epilogue): w is the packed [2H, K] gate | up weight, gate
//    rows first; N_out = H. A wave owns R/2 gate rows n.. and the R/2 up rows
//    H + n.., so both halves of an output meet in one lane after the reduce
//    and the gate is computed exactly once: h = silu(a) * u in fp32.
//    A workgroup makes 4 (M <= 2) or 8 (M >= 3) outputs.
//  * RES (residual epilogue): + residual[m, n] (unit stride in N, row stride
//    passed) in fp32 before the single rounding; y is a fresh tensor.
//
// Epilogue order, fixed: * inv[m], * scale[n], + bias[n], gate, + residual,
// one rounding to bf16.
//
// Everything else is the parent kernel's: 16-byte non-temporal weight loads
// straight to VGPRs, all U * R of a trip in flight before the first use; no
// LDS, no atomics, no K split; the dot product's reduction order is the
// parent's, so with no option set the result equals skinny_linear's. Rows
// past N_out re-read the last row and batch rows past M re-read row M-1
// (always inside the tensors); their results are not stored. No launch
// argument depends on the decode step, so the launch is graph-capturable.
// The options are template parameters: an unused one costs nothing.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int FGEMV_THREADS = 256;
constexpr int FGEMV_WAVES = FGEMV_THREADS / WAVE_SIZE;
constexpr int FGEMV_MAX_M = 8;
constexpr int FGEMV_CHUNK_BYTES = 16;

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

constexpr int fgemv_rows(int MT) { return MT <= 2 ? 2 : 4; }     // R
constexpr int fgemv_unroll(int MT) { return MT <= 2 ? 4 : 2; }   // U

__device__ __forceinline__ floatx2 fma2(floatx2 a, floatx2 b, floatx2 c) {
  return __builtin_elementwise_fma(a, b, c);
}

// two adjacent bf16 (little endian: the low half is the earlier element)
__device__ __forceinline__ floatx2 bf16x2_to_f32(unsigned int u) {
  floatx2 r;
  r.x = __uint_as_float(u << 16);
  r.y = __uint_as_float(u & 0xffff0000u);
  return r;
}

// Two adjacent x elements of batch row m, ready for the FMAs: with NORM their
// squares go to the row's sum first and the pair is scaled by its g pair.
template <bool NORM>
__device__ __forceinline__ floatx2 x_pair(unsigned int xu, unsigned int gu,
                                          floatx2& ssq) {
  floatx2 xf = bf16x2_to_f32(xu);
  if constexpr (NORM) {
    ssq = fma2(xf, xf, ssq);
    xf = xf * bf16x2_to_f32(gu);
  }
  return xf;
}

// Multiply chunk c of the R weight rows (held in wq) into every batch row.
template <bool FP8, bool NORM, int MT, int R>
__device__ __forceinline__ void chunk_fma(const uintx4 (&wq)[R],
                                          const unsigned short* const (&xr)[MT],
                                          const unsigned short* g, int c,
                                          floatx2 (&acc)[MT][R],
                                          floatx2 (&ssq)[MT]) {
  if constexpr (FP8) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // 8 elements: weight dwords 2h, 2h + 1
      uintx4 xv[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        xv[m] = *reinterpret_cast<const uintx4*>(xr[m] + (long)c * 16 + h * 8);
      uintx4 gv = {0u, 0u, 0u, 0u};
      if constexpr (NORM)
        gv = *reinterpret_cast<const uintx4*>(g + (long)c * 16 + h * 8);
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        floatx2 wlo[R], whi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const unsigned int u = wq[r][2 * h + d];
          wlo[r] = __builtin_amdgcn_cvt_pk_f32_fp8(u, false);   // bytes 0, 1
          whi[r] = __builtin_amdgcn_cvt_pk_f32_fp8(u, true);    // bytes 2, 3
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const floatx2 x0 = x_pair<NORM>(xv[m][2 * d], gv[2 * d], ssq[m]);
          const floatx2 x1 = x_pair<NORM>(xv[m][2 * d + 1], gv[2 * d + 1],
                                          ssq[m]);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            acc[m][r] = fma2(wlo[r], x0, acc[m][r]);
            acc[m][r] = fma2(whi[r], x1, acc[m][r]);
          }
        }
      }
    }
  } else {
    uintx4 xv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
      xv[m] = *reinterpret_cast<const uintx4*>(xr[m] + (long)c * 8);
    uintx4 gv = {0u, 0u, 0u, 0u};
    if constexpr (NORM) gv = *reinterpret_cast<const uintx4*>(g + (long)c * 8);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      floatx2 wf[R];
#pragma unroll
      for (int r = 0; r < R; ++r) wf[r] = bf16x2_to_f32(wq[r][d]);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const floatx2 x0 = x_pair<NORM>(xv[m][d], gv[d], ssq[m]);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = fma2(wf[r], x0, acc[m][r]);
      }
    }
  }
}

struct FusedArgs {
  const unsigned short* x;      // [M, K], row stride x_sm
  long x_sm;
  const unsigned char* w;       // [N, K] (GLU: N = 2 * n_out)
  const float* scale;           // [N] (FP8) or nullptr
  const unsigned short* bias;   // [N] or nullptr
  const unsigned short* g;      // [K] (NORM)
  const unsigned short* res;    // [M, n_out], row stride res_sm (RES)
  long res_sm;
  unsigned short* y;            // [M, n_out] contiguous
  float eps;
  float k;                      // K
  int M;
  int n_out;
  int C;                        // 16-byte chunks per weight row
};

template <bool FP8, int MT, bool NORM, bool GLU, bool RES>
__global__ __launch_bounds__(FGEMV_THREADS)
void skinny_linear_fused_kernel(const FusedArgs a) {
  constexpr int R = fgemv_rows(MT);
  constexpr int U = fgemv_unroll(MT);
  constexpr int RO = GLU ? R / 2 : R;   // outputs per wave and batch row
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int M = a.M, NO = a.n_out, C = a.C;
  const int n0 = (blockIdx.x * FGEMV_WAVES + wave) * RO;
  if (n0 >= NO) return;   // the whole wave; there is no barrier below

  // weight rows of the wave: outputs n0.. (GLU: their gate rows), then with
  // GLU the matching up rows NO + n0..
  const unsigned char* wr[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int n = (r < RO ? 0 : NO) + min(n0 + r % RO, NO - 1);
    wr[r] = a.w + (long)n * C * FGEMV_CHUNK_BYTES;
  }
  const unsigned short* xr[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xr[m] = a.x + (long)min(m, M - 1) * a.x_sm;

  floatx2 acc[MT][R];
  floatx2 ssq[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    ssq[m] = floatx2{0.f, 0.f};
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = floatx2{0.f, 0.f};
  }

  int c = lane;
  // U passes per trip: every chunk c + u * 64 < C exists
  for (; c + (U - 1) * WAVE_SIZE < C; c += U * WAVE_SIZE) {
    uintx4 wq[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r)
        wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
            wr[r] + (long)(c + u * WAVE_SIZE) * FGEMV_CHUNK_BYTES));
    // all U * R weight loads are in flight before any is used
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
      chunk_fma<FP8, NORM, MT, R>(wq[u], xr, a.g, c + u * WAVE_SIZE, acc, ssq);
  }
  // tail: one pass per trip, only the lanes whose chunk exists
  for (; c < C; c += WAVE_SIZE) {
    uintx4 wq[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      wq[r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
          wr[r] + (long)c * FGEMV_CHUNK_BYTES));
    chunk_fma<FP8, NORM, MT, R>(wq, xr, a.g, c, acc, ssq);
  }

  // lane m * RO + j keeps output (m, n0 + j): its dot product (GLU: the gate
  // row's in `mine`, the up row's in `up`) and its row's sum of squares
  float mine = 0.f, up = 0.f, sq = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if constexpr (NORM) {
      const float t = wave_reduce_sum(ssq[m].x + ssq[m].y);
      if (lane / RO == m) sq = t;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float t = wave_reduce_sum(acc[m][r].x + acc[m][r].y);
      if (lane == m * RO + r % RO) {
        if (r < RO) mine = t; else up = t;
      }
    }
  }
  if (lane < MT * RO) {
    const int m = lane / RO, n = n0 + lane % RO;
    if (m < M && n < NO) {
      float inv = 1.f;
      if constexpr (NORM) inv = rsqrtf(sq / a.k + a.eps);
      float s = mine;
      if constexpr (NORM) s = __fmul_rn(s, inv);
      if constexpr (FP8) s = __fmul_rn(s, a.scale[n]);
      if (a.bias != nullptr) s = __fadd_rn(s, bf16_to_f32(a.bias[n]));
      if constexpr (GLU) {
        float u = up;
        if constexpr (NORM) u = __fmul_rn(u, inv);
        if constexpr (FP8) u = __fmul_rn(u, a.scale[NO + n]);
        if (a.bias != nullptr) u = __fadd_rn(u, bf16_to_f32(a.bias[NO + n]));
        s = __fmul_rn(s / (1.f + expf(-s)), u);
      }
      if constexpr (RES)
        s = __fadd_rn(s, bf16_to_f32(a.res[(long)m * a.res_sm + n]));
      a.y[(long)m * NO + n] = f32_to_bf16(s);
    }
  }
}

template <bool FP8, int MT, bool NORM, bool GLU, bool RES>
void launch_fused(const FusedArgs& a, hipStream_t stream) {
  const int outs_per_wg = FGEMV_WAVES * fgemv_rows(MT) / (GLU ? 2 : 1);
  hipLaunchKernelGGL((skinny_linear_fused_kernel<FP8, MT, NORM, GLU, RES>),
                     dim3((a.n_out + outs_per_wg - 1) / outs_per_wg),
                     dim3(FGEMV_THREADS), 0, stream, a);
  HIP_CHECK_KERNEL();
}

template <bool FP8, bool NORM, bool GLU, bool RES>
void dispatch_m(const FusedArgs& a, hipStream_t stream) {
  if (a.M == 1) launch_fused<FP8, 1, NORM, GLU, RES>(a, stream);
  else if (a.M == 2) launch_fused<FP8, 2, NORM, GLU, RES>(a, stream);
  else if (a.M <= 4) launch_fused<FP8, 4, NORM, GLU, RES>(a, stream);
  else launch_fused<FP8, 8, NORM, GLU, RES>(a, stream);
}

template <bool FP8, bool NORM, bool GLU>
void dispatch_res(const FusedArgs& a, hipStream_t stream) {
  if (a.res != nullptr) dispatch_m<FP8, NORM, GLU, true>(a, stream);
  else dispatch_m<FP8, NORM, GLU, false>(a, stream);
}

template <bool FP8>
void dispatch_options(const FusedArgs& a, bool glu, hipStream_t stream) {
  if (a.g != nullptr) {
    if (glu) dispatch_res<FP8, true, true>(a, stream);
    else dispatch_res<FP8, true, false>(a, stream);
  } else {
    if (glu) dispatch_res<FP8, false, true>(a, stream);
    else dispatch_res<FP8, false, false>(a, stream);
  }
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

torch::Tensor skinny_linear_fused(torch::Tensor x, torch::Tensor w,
                                  c10::optional<torch::Tensor> scale,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> norm_weight,
                                  double eps,
                                  c10::optional<torch::Tensor> residual,
                                  bool glu) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16,
              "skinny_linear_fused: x must be device bf16 [M, K]");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.device() == x.device()
              && w.is_contiguous(),
              "skinny_linear_fused: w must be contiguous [N, K] on x's device");
  const bool fp8 = w.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || w.dtype() == torch::kBFloat16,
              "skinny_linear_fused: w must be float8_e4m3fn or bf16");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= FGEMV_MAX_M,
              "skinny_linear_fused: M must be in [1, ", FGEMV_MAX_M, "], got ",
              M);
  TORCH_CHECK(w.size(1) == K && K >= 16 && K % 16 == 0,
              "skinny_linear_fused: x [M, K] and w [N, K] must share K, a "
              "positive multiple of 16; got ", K, " and ", w.size(1));
  TORCH_CHECK(N >= 1 && N < (1L << 31) && N * K < (1L << 40),
              "skinny_linear_fused: N out of range");
  TORCH_CHECK(!glu || N % 2 == 0,
              "skinny_linear_fused: glu needs an even N (gate | up rows), got ",
              N);
  const long NO = glu ? N / 2 : N;
  TORCH_CHECK(x.stride(1) == 1 && (M == 1 || x.stride(0) % 8 == 0)
              && aligned16(x) && aligned16(w),
              "skinny_linear_fused: x needs unit stride in K and 16-byte "
              "aligned rows; w a 16-byte aligned base");
  TORCH_CHECK(fp8 == scale.has_value(),
              "skinny_linear_fused: e4m3 weights need scale, bf16 weights "
              "none");
  FusedArgs a{};
  if (fp8) {
    TORCH_CHECK(scale->is_cuda() && scale->device() == x.device()
                && scale->dtype() == torch::kFloat32 && scale->dim() == 1
                && scale->size(0) == N && scale->is_contiguous(),
                "skinny_linear_fused: scale must be contiguous device fp32 "
                "[N]");
    a.scale = scale->data_ptr<float>();
  }
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == x.device()
                && bias->dtype() == torch::kBFloat16 && bias->dim() == 1
                && bias->size(0) == N && bias->is_contiguous(),
                "skinny_linear_fused: bias must be contiguous device bf16 [N]");
    a.bias = (const unsigned short*)bias->data_ptr();
  }
  if (norm_weight.has_value()) {
    TORCH_CHECK(norm_weight->is_cuda() && norm_weight->device() == x.device()
                && norm_weight->dtype() == torch::kBFloat16
                && norm_weight->dim() == 1 && norm_weight->size(0) == K
                && norm_weight->is_contiguous() && aligned16(*norm_weight),
                "skinny_linear_fused: norm_weight must be contiguous, 16-byte "
                "aligned device bf16 [K]");
    TORCH_CHECK(eps >= 0.0, "skinny_linear_fused: eps must be >= 0");
    a.g = (const unsigned short*)norm_weight->data_ptr();
  }
  if (residual.has_value()) {
    TORCH_CHECK(residual->is_cuda() && residual->device() == x.device()
                && residual->dtype() == torch::kBFloat16
                && residual->dim() == 2 && residual->size(0) == M
                && residual->size(1) == NO && residual->stride(1) == 1
                && (M == 1 || residual->stride(0) >= NO),
                "skinny_linear_fused: residual must be device bf16 [M, N_out] "
                "with unit stride in N");
    a.res = (const unsigned short*)residual->data_ptr();
    a.res_sm = M == 1 ? NO : residual->stride(0);
  }
  a.x = (const unsigned short*)x.data_ptr();
  a.x_sm = x.stride(0);
  a.w = (const unsigned char*)w.data_ptr();
  auto y = torch::empty({M, NO}, x.options());
  a.y = (unsigned short*)y.data_ptr();
  a.eps = (float)eps;
  a.k = (float)K;
  a.M = (int)M;
  a.n_out = (int)NO;
  a.C = (int)(K * w.element_size() / FGEMV_CHUNK_BYTES);
  auto stream = at::cuda::getCurrentHIPStream();
  if (fp8) dispatch_options<true>(a, glu, stream);
  else dispatch_options<false>(a, glu, stream);
  return y;
}
