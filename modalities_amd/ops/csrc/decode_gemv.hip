// Skinny GEMM for single-token decoding: y[M, N] = x[M, K] . W[N, K]^T with
// 1 <= M <= 8, W streamed once from HBM straight to VGPRs. Inference only.
//
// skinny_linear(x [M,K] bf16, w [N,K] e4m3 | bf16, scale fp32 [N] | None,
//               bias bf16 [N] | None) -> y [M,N] bf16
//
// The cost of these GEMMs is the weight bytes, so the kernel is a weight
// stream with the FMAs hung on it (guide: GEMV / M <= 16 decode weights --
// no LDS round trip, deep unroll, late vmcnt):
//
//  * A weight row is K/E 16-byte chunks (E = 16 e4m3 or 8 bf16 elements per
//    chunk). One wave owns R adjacent rows; lane l takes the chunks l, l+64,
//    l+128, ... of each of them, so one pass of a wave is 1 KiB of a row
//    (GEMV_PASS_BYTES: 1024 e4m3 / 512 bf16 elements). The main loop issues
//    U passes x R rows of 16-byte loads (8 per lane) before the first use;
//    the tail loop takes the remaining passes one at a time, and in the last
//    of them only the lanes whose chunk exists (K = 2560 e4m3 is 2.5 passes).
//  * Every chunk is multiplied into all MT batch rows: the x pieces of a
//    chunk (32 or 16 bytes per batch row, L1/L2 resident) are loaded once per
//    wave pass and reused by the R weight rows.
//  * e4m3 is widened by v_cvt_pk_f32_fp8 (OCP e4m3 on gfx950), bf16 by a
//    shift / mask; products and sums are fp32 FMAs on (even, odd) element
//    pairs (v_pk_fma_f32).
//  * Reduction order of one output (m, n), fixed: a lane adds its chunks in
//    ascending order into one (even, odd) accumulator pair, even + odd, then
//    the xor-shuffle tree over the 64 lanes. Neither R, U, MT nor the row's
//    place in the batch enters it, so a row's result is bit-identical for
//    every M and every position. No atomics, no split of K over workgroups.
//  * Epilogue, unfused and in this order: * scale[n], + bias[n], one rounding
//    to bf16.
//
// Tiling: 256 threads = 4 waves; MT in {1, 2} (M = 1, 2): R = 2, U = 4, 8
// rows per workgroup; MT in {4, 8} (M = 3..8): R = 4, U = 2, 16 rows per
// workgroup. Rows past N re-read row N-1 and batch rows past M re-read row
// M-1 (always inside the tensors); their results are not stored. No launch
// argument depends on the decode step, so the launch is graph-capturable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int GEMV_THREADS = 256;
constexpr int GEMV_WAVES = GEMV_THREADS / WAVE_SIZE;
constexpr int GEMV_MAX_M = 8;
constexpr int GEMV_CHUNK_BYTES = 16;
constexpr int GEMV_PASS_BYTES = WAVE_SIZE * GEMV_CHUNK_BYTES;

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

constexpr int gemv_rows(int MT) { return MT <= 2 ? 2 : 4; }     // R
constexpr int gemv_unroll(int MT) { return MT <= 2 ? 4 : 2; }   // U

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

// Multiply chunk c of the R weight rows (held in wq) into every batch row.
template <bool FP8, int MT, int R>
__device__ __forceinline__ void chunk_fma(const uintx4 (&wq)[R],
                                          const unsigned short* const (&xr)[MT],
                                          int c, floatx2 (&acc)[MT][R]) {
  if constexpr (FP8) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // 8 elements: weight dwords 2h, 2h + 1
      uintx4 xv[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        xv[m] = *reinterpret_cast<const uintx4*>(xr[m] + (long)c * 16 + h * 8);
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
          const floatx2 x0 = bf16x2_to_f32(xv[m][2 * d]);
          const floatx2 x1 = bf16x2_to_f32(xv[m][2 * d + 1]);
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
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      floatx2 wf[R];
#pragma unroll
      for (int r = 0; r < R; ++r) wf[r] = bf16x2_to_f32(wq[r][d]);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const floatx2 x0 = bf16x2_to_f32(xv[m][d]);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = fma2(wf[r], x0, acc[m][r]);
      }
    }
  }
}

template <bool FP8, int MT>
__global__ __launch_bounds__(GEMV_THREADS)
void skinny_linear_kernel(const unsigned short* __restrict__ x, long x_sm,
                          const unsigned char* __restrict__ w,
                          const float* __restrict__ scale,
                          const unsigned short* __restrict__ bias,
                          unsigned short* __restrict__ y, int M, int N,
                          int C) {   // C = 16-byte chunks per weight row
  constexpr int R = gemv_rows(MT);
  constexpr int U = gemv_unroll(MT);
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int n0 = (blockIdx.x * GEMV_WAVES + wave) * R;
  if (n0 >= N) return;   // the whole wave; there is no barrier below

  const unsigned char* wr[R];
#pragma unroll
  for (int r = 0; r < R; ++r)
    wr[r] = w + (long)min(n0 + r, N - 1) * C * GEMV_CHUNK_BYTES;
  const unsigned short* xr[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) xr[m] = x + (long)min(m, M - 1) * x_sm;

  floatx2 acc[MT][R];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = floatx2{0.f, 0.f};

  int c = lane;
  // U passes per trip: every chunk c + u * 64 < C exists
  for (; c + (U - 1) * WAVE_SIZE < C; c += U * WAVE_SIZE) {
    uintx4 wq[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r)
        wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
            wr[r] + (long)(c + u * WAVE_SIZE) * GEMV_CHUNK_BYTES));
    // keep the scheduler from sinking part of the weight loads below the
    // first wait: all U * R of them are in flight before any is used
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
      chunk_fma<FP8, MT, R>(wq[u], xr, c + u * WAVE_SIZE, acc);
  }
  // tail: one pass per trip, only the lanes whose chunk exists
  for (; c < C; c += WAVE_SIZE) {
    uintx4 wq[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      wq[r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
          wr[r] + (long)c * GEMV_CHUNK_BYTES));
    chunk_fma<FP8, MT, R>(wq, xr, c, acc);
  }

  // lane m * R + r keeps output (m, n0 + r)
  float mine = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float t = wave_reduce_sum(acc[m][r].x + acc[m][r].y);
      if (lane == m * R + r) mine = t;
    }
  if (lane < MT * R) {
    const int m = lane / R, n = n0 + lane % R;
    if (m < M && n < N) {
      float s = mine;
      if constexpr (FP8) s = __fmul_rn(s, scale[n]);
      if (bias != nullptr) s = __fadd_rn(s, bf16_to_f32(bias[n]));
      y[(long)m * N + n] = f32_to_bf16(s);
    }
  }
}

template <bool FP8, int MT>
void launch_skinny(const torch::Tensor& x, const torch::Tensor& w,
                   const float* scale, const unsigned short* bias,
                   torch::Tensor& y, hipStream_t stream) {
  const int M = x.size(0), N = w.size(0);
  const int C = (int)(w.size(1) * w.element_size() / GEMV_CHUNK_BYTES);
  const int rows_per_wg = GEMV_WAVES * gemv_rows(MT);
  hipLaunchKernelGGL((skinny_linear_kernel<FP8, MT>),
                     dim3((N + rows_per_wg - 1) / rows_per_wg),
                     dim3(GEMV_THREADS), 0, stream,
                     (const unsigned short*)x.data_ptr(), (long)x.stride(0),
                     (const unsigned char*)w.data_ptr(), scale, bias,
                     (unsigned short*)y.data_ptr(), M, N, C);
  HIP_CHECK_KERNEL();
}

template <bool FP8>
void dispatch_skinny(const torch::Tensor& x, const torch::Tensor& w,
                     const float* scale, const unsigned short* bias,
                     torch::Tensor& y, hipStream_t stream) {
  const long M = x.size(0);
  if (M == 1) launch_skinny<FP8, 1>(x, w, scale, bias, y, stream);
  else if (M == 2) launch_skinny<FP8, 2>(x, w, scale, bias, y, stream);
  else if (M <= 4) launch_skinny<FP8, 4>(x, w, scale, bias, y, stream);
  else launch_skinny<FP8, 8>(x, w, scale, bias, y, stream);
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

long skinny_linear_max_m() { return GEMV_MAX_M; }

torch::Tensor skinny_linear(torch::Tensor x, torch::Tensor w,
                            c10::optional<torch::Tensor> scale,
                            c10::optional<torch::Tensor> bias) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16,
              "skinny_linear: x must be device bf16 [M, K]");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.device() == x.device()
              && w.is_contiguous(),
              "skinny_linear: w must be contiguous [N, K] on x's device");
  const bool fp8 = w.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || w.dtype() == torch::kBFloat16,
              "skinny_linear: w must be float8_e4m3fn or bf16");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= GEMV_MAX_M, "skinny_linear: M must be in [1, ",
              GEMV_MAX_M, "], got ", M);
  TORCH_CHECK(w.size(1) == K && K >= 16 && K % 16 == 0,
              "skinny_linear: x [M, K] and w [N, K] must share K, a positive "
              "multiple of 16; got ", K, " and ", w.size(1));
  TORCH_CHECK(N >= 1 && N < (1L << 31) && N * K < (1L << 40),
              "skinny_linear: N out of range");
  TORCH_CHECK(x.stride(1) == 1 && (M == 1 || x.stride(0) % 8 == 0)
              && aligned16(x) && aligned16(w),
              "skinny_linear: x needs unit stride in K and 16-byte aligned "
              "rows; w a 16-byte aligned base");
  TORCH_CHECK(fp8 == scale.has_value(),
              "skinny_linear: e4m3 weights need scale, bf16 weights none");
  const float* sp = nullptr;
  if (fp8) {
    TORCH_CHECK(scale->is_cuda() && scale->device() == x.device()
                && scale->dtype() == torch::kFloat32 && scale->dim() == 1
                && scale->size(0) == N && scale->is_contiguous(),
                "skinny_linear: scale must be contiguous device fp32 [N]");
    sp = scale->data_ptr<float>();
  }
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == x.device()
                && bias->dtype() == torch::kBFloat16 && bias->dim() == 1
                && bias->size(0) == N && bias->is_contiguous(),
                "skinny_linear: bias must be contiguous device bf16 [N]");
    bp = (const unsigned short*)bias->data_ptr();
  }
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (fp8) dispatch_skinny<true>(x, w, sp, bp, y, stream);
  else dispatch_skinny<false>(x, w, sp, bp, y, stream);
  return y;
}
