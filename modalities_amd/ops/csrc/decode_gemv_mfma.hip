// Skinny GEMM on the matrix cores for decode batches of 1..32 rows:
// y[M, N] = x[M, K] . W[N, K]^T, W streamed once from HBM straight to VGPRs.
// gfx950 only. Inference only.
//
// skinny_linear_mfma(x [M,K] bf16, w [N,K] e4m3 | bf16, scale fp32 [N] | None,
//                    bias bf16 [N] | None) -> y [M,N] bf16
//
// decode_gemv.hip multiplies every weight into every batch row on the VALU,
// so its arithmetic grows with M. Here the arithmetic per weight is one
// conversion (e4m3) or none (bf16), whatever M is:
//
//  * The weight is the MFMA A operand and x^T the B operand of
//    v_mfma_f32_16x16x32_bf16: 16 weight rows n along the instruction's M,
//    16 batch rows m along its N. In its fragment map lane l holds, for A and
//    for B alike, 8 consecutive k of row l % 16 in k-group g = l / 16. The
//    contraction is a plain sum over k, so which k a (g, element) slot stands
//    for is free as long as A and B agree.
//  * A wave step is 64 contiguous bytes of each of 16 weight rows: lane
//    (row, g) takes the 16-byte chunk c = 4 * step + g of its row with one
//    non-temporal load, no LDS stop. For e4m3 that chunk is 16 k: the A
//    fragments of two MFMAs (bytes 0-7, then 8-15), and the lane's x pieces
//    are x[m][16c .. 16c + 15], two 16-byte loads used in the same order.
//    For bf16 the chunk is 8 k, one MFMA, one 16-byte piece of x.
//  * e4m3 -> bf16 is exact: v_cvt_pk_f32_fp8 widens two codes to fp32 and the
//    high halves of the pair are packed into one dword, about one VALU op
//    per weight.
//  * A workgroup owns 16 * RT weight rows and all of K. Its KSPLIT waves take
//    the wave steps w, w + KSPLIT, w + 2 KSPLIT, ... each into accumulators of
//    its own (RT * MTILES * 4 fp32 per lane). A trip of the K loop issues
//    MFMA_GEMV_LOADS 16-byte weight loads per lane before the first use.
//    x pieces come from L2: every piece is read by exactly one wave of the
//    workgroup and reused by its RT row tiles in registers, so staging x in
//    LDS would move the same bytes once more.
//  * Reduction order of one output (m, n), fixed: a wave adds its steps in
//    ascending order through the MFMA accumulator; waves 1.. write their
//    partial tiles to LDS; after one barrier wave 0 adds them to its own in
//    wave order 1, 2, ..., KSPLIT - 1. Neither M, MTILES, RT nor the row's
//    place in the batch enters it, so a row's result is bit-identical for
//    every M and every position. No atomics, no split of K over workgroups.
//  * Epilogue, unfused and in this order: * scale[n], + bias[n], one rounding
//    to bf16. A lane of wave 0 holds four consecutive n of one m.
//  * Tails: weight rows past N re-read row N - 1 and batch rows past M re-read
//    row M - 1 (always inside the tensors); MFMA output columns and rows are
//    independent, and those are never stored. A chunk at or beyond the end of
//    K issues no load; its fragments are zeros.
//
// MTILES = 1 (M <= 16) or 2 (M <= 32). No launch argument depends on the
// decode step, so the launch is graph-capturable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int MFMA_GEMV_MAX_M = 32;
constexpr int MFMA_GEMV_TILE = 16;          // weight rows / batch rows per tile
constexpr int MFMA_GEMV_CHUNK_BYTES = 16;
constexpr int MFMA_GEMV_GROUPS = 4;         // k-groups (chunks per row) per wave step
constexpr int MFMA_GEMV_LOADS = 8;          // weight loads in flight per lane
// tiling when the caller names none (profiles/decode_gemv.md, "MFMA kernel":
// the A/B; ops.skinny_linear_mfma picks RT by N)
constexpr int MFMA_GEMV_RT = 1;
constexpr int MFMA_GEMV_KSPLIT = 8;

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// the bf16 of two fp32 whose low 16 bits are zero (little endian: lo first)
__device__ __forceinline__ unsigned int pack_high_halves(float lo, float hi) {
  // v_perm_b32: selector bytes 0-3 pick from the second operand, 4-7 from
  // the first; result = {lo.b2, lo.b3, hi.b2, hi.b3}
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo),
                               0x07060302u);
}

// eight e4m3 codes (two dwords) -> eight bf16, exactly
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16x8(unsigned int u0,
                                                   unsigned int u1) {
  const floatx2 a = __builtin_amdgcn_cvt_pk_f32_fp8(u0, false);   // bytes 0, 1
  const floatx2 b = __builtin_amdgcn_cvt_pk_f32_fp8(u0, true);    // bytes 2, 3
  const floatx2 c = __builtin_amdgcn_cvt_pk_f32_fp8(u1, false);
  const floatx2 d = __builtin_amdgcn_cvt_pk_f32_fp8(u1, true);
  const uintx4 r = {pack_high_halves(a.x, a.y), pack_high_halves(b.x, b.y),
                    pack_high_halves(c.x, c.y), pack_high_halves(d.x, d.y)};
  return __builtin_bit_cast(bf16x8, r);
}

// One trip of a wave's K loop: the wave steps s0, s0 + KSPLIT, ..., U of them.
// FULL: every chunk of every step exists; otherwise a lane loads only the
// chunks c < C and the steps at or past S are skipped.
template <bool FP8, int MTILES, int RT, int KSPLIT, bool FULL>
__device__ __forceinline__ void mfma_trip(
    const unsigned char* const (&wr)[RT],
    const unsigned short* const (&xr)[MTILES], int s0, int g, int C, int S,
    floatx4 (&acc)[RT][MTILES]) {
  constexpr int U = MFMA_GEMV_LOADS / RT;
  constexpr int H = FP8 ? 2 : 1;     // MFMAs (8 k each) per 16-byte chunk
  constexpr int XE = FP8 ? 16 : 8;   // x elements per chunk
  // x first: its pieces come from L2 and are back before the weights
  uintx4 xv[U][MTILES][H];
  uintx4 wq[U][RT];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = (s0 + u * KSPLIT) * MFMA_GEMV_GROUPS + g;
#pragma unroll
    for (int m = 0; m < MTILES; ++m)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        xv[u][m][h] = uintx4{0u, 0u, 0u, 0u};
        if (FULL || c < C)
          xv[u][m][h] = *reinterpret_cast<const uintx4*>(
              xr[m] + (long)c * XE + h * 8);
      }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = (s0 + u * KSPLIT) * MFMA_GEMV_GROUPS + g;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      wq[u][r] = uintx4{0u, 0u, 0u, 0u};
      if (FULL || c < C)
        wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
            wr[r] + (long)c * MFMA_GEMV_CHUNK_BYTES));
    }
  }
  // keep the scheduler from sinking part of the loads below the first wait:
  // all U * RT weight loads are in flight before any is used
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && s0 + u * KSPLIT >= S) break;   // the whole wave
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        bf16x8 a;
        if constexpr (FP8)
          a = e4m3x8_to_bf16x8(wq[u][r][2 * h], wq[u][r][2 * h + 1]);
        else
          a = __builtin_bit_cast(bf16x8, wq[u][r]);
#pragma unroll
        for (int m = 0; m < MTILES; ++m)
          acc[r][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, xv[u][m][h]), acc[r][m], 0, 0, 0);
      }
  }
}

template <bool FP8, int MTILES, int RT, int KSPLIT>
__global__ __launch_bounds__(KSPLIT * WAVE_SIZE)
void skinny_linear_mfma_kernel(const unsigned short* __restrict__ x, long x_sm,
                               const unsigned char* __restrict__ w,
                               const float* __restrict__ scale,
                               const unsigned short* __restrict__ bias,
                               unsigned short* __restrict__ y, int M, int N,
                               int C) {   // C = 16-byte chunks per weight row
  static_assert(KSPLIT >= 2 && MFMA_GEMV_LOADS % RT == 0, "tiling");
  constexpr int U = MFMA_GEMV_LOADS / RT;
  constexpr int TILES = RT * MTILES;
  __shared__ floatx4 part[(KSPLIT - 1) * TILES * WAVE_SIZE];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const int row = lane & (MFMA_GEMV_TILE - 1);   // n of A, m of B
  const int g = lane / MFMA_GEMV_TILE;           // k-group
  const int n0 = blockIdx.x * (MFMA_GEMV_TILE * RT);

  const unsigned char* wr[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
    wr[r] = w + (long)min(n0 + r * MFMA_GEMV_TILE + row, N - 1) * C
                    * MFMA_GEMV_CHUNK_BYTES;
  const unsigned short* xr[MTILES];
#pragma unroll
  for (int m = 0; m < MTILES; ++m)
    xr[m] = x + (long)min(m * MFMA_GEMV_TILE + row, M - 1) * x_sm;

  floatx4 acc[RT][MTILES];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int m = 0; m < MTILES; ++m) acc[r][m] = floatx4{0.f, 0.f, 0.f, 0.f};

  // wave steps in K (the last may be partial); this wave takes s = wave,
  // wave + KSPLIT, ..., U of them per trip
  const int S = (C + MFMA_GEMV_GROUPS - 1) / MFMA_GEMV_GROUPS;
  int s0 = wave;
  for (; (s0 + (U - 1) * KSPLIT + 1) * MFMA_GEMV_GROUPS <= C;
       s0 += U * KSPLIT)
    mfma_trip<FP8, MTILES, RT, KSPLIT, true>(wr, xr, s0, g, C, S, acc);
  for (; s0 < S; s0 += U * KSPLIT)
    mfma_trip<FP8, MTILES, RT, KSPLIT, false>(wr, xr, s0, g, C, S, acc);

  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int m = 0; m < MTILES; ++m)
        part[((wave - 1) * TILES + r * MTILES + m) * WAVE_SIZE + lane] =
            acc[r][m];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int v = 1; v < KSPLIT; ++v)
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int m = 0; m < MTILES; ++m) {
        const floatx4 p =
            part[((v - 1) * TILES + r * MTILES + m) * WAVE_SIZE + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[r][m][i] = __fadd_rn(acc[r][m][i], p[i]);
      }

  // C/D map: lane (row, g) holds rows 4g .. 4g + 3 (n) of column `row` (m)
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int m = 0; m < MTILES; ++m) {
      const int mm = m * MFMA_GEMV_TILE + row;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + r * MFMA_GEMV_TILE + g * 4 + i;
        if (mm < M && n < N) {
          float s = acc[r][m][i];
          if constexpr (FP8) s = __fmul_rn(s, scale[n]);
          if (bias != nullptr) s = __fadd_rn(s, bf16_to_f32(bias[n]));
          y[(long)mm * N + n] = f32_to_bf16(s);
        }
      }
    }
}

template <bool FP8, int MTILES, int RT, int KSPLIT>
void launch_mfma(const torch::Tensor& x, const torch::Tensor& w,
                 const float* scale, const unsigned short* bias,
                 torch::Tensor& y, hipStream_t stream) {
  const int M = x.size(0), N = w.size(0);
  const int C = (int)(w.size(1) * w.element_size() / MFMA_GEMV_CHUNK_BYTES);
  const int rows_per_wg = MFMA_GEMV_TILE * RT;
  hipLaunchKernelGGL((skinny_linear_mfma_kernel<FP8, MTILES, RT, KSPLIT>),
                     dim3((N + rows_per_wg - 1) / rows_per_wg),
                     dim3(KSPLIT * WAVE_SIZE), 0, stream,
                     (const unsigned short*)x.data_ptr(), (long)x.stride(0),
                     (const unsigned char*)w.data_ptr(), scale, bias,
                     (unsigned short*)y.data_ptr(), M, N, C);
  HIP_CHECK_KERNEL();
}

template <bool FP8, int MTILES>
void dispatch_tiling(int rt, int ksplit, const torch::Tensor& x,
                     const torch::Tensor& w, const float* scale,
                     const unsigned short* bias, torch::Tensor& y,
                     hipStream_t stream) {
  if (rt == 1 && ksplit == 4)
    launch_mfma<FP8, MTILES, 1, 4>(x, w, scale, bias, y, stream);
  else if (rt == 1)
    launch_mfma<FP8, MTILES, 1, 8>(x, w, scale, bias, y, stream);
  else if (ksplit == 4)
    launch_mfma<FP8, MTILES, 2, 4>(x, w, scale, bias, y, stream);
  else
    launch_mfma<FP8, MTILES, 2, 8>(x, w, scale, bias, y, stream);
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

long skinny_linear_mfma_max_m() { return MFMA_GEMV_MAX_M; }

// rt / ksplit: 0 takes the tiling above. RT does not enter a result (the
// Python wrapper picks it by N); KSPLIT does (the order of the partial sums)
// and is named only by the A/B of tools/decode_gemv_bench.py.
torch::Tensor skinny_linear_mfma(torch::Tensor x, torch::Tensor w,
                                 c10::optional<torch::Tensor> scale,
                                 c10::optional<torch::Tensor> bias,
                                 long rt, long ksplit) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16,
              "skinny_linear_mfma: x must be device bf16 [M, K]");
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.device() == x.device()
              && w.is_contiguous(),
              "skinny_linear_mfma: w must be contiguous [N, K] on x's device");
  const bool fp8 = w.dtype() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(fp8 || w.dtype() == torch::kBFloat16,
              "skinny_linear_mfma: w must be float8_e4m3fn or bf16");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= MFMA_GEMV_MAX_M,
              "skinny_linear_mfma: M must be in [1, ", MFMA_GEMV_MAX_M,
              "], got ", M);
  TORCH_CHECK(w.size(1) == K && K >= 16 && K % 16 == 0,
              "skinny_linear_mfma: x [M, K] and w [N, K] must share K, a "
              "positive multiple of 16; got ", K, " and ", w.size(1));
  // chunk and step indices are int in the kernel
  TORCH_CHECK(N >= 1 && N < (1L << 31) && K < (1L << 31)
              && N * K < (1L << 40),
              "skinny_linear_mfma: N or K out of range");
  TORCH_CHECK(x.stride(1) == 1 && (M == 1 || x.stride(0) % 8 == 0)
              && aligned16(x) && aligned16(w),
              "skinny_linear_mfma: x needs unit stride in K and 16-byte "
              "aligned rows; w a 16-byte aligned base");
  TORCH_CHECK(fp8 == scale.has_value(),
              "skinny_linear_mfma: e4m3 weights need scale, bf16 weights none");
  TORCH_CHECK((rt == 0 || rt == 1 || rt == 2)
              && (ksplit == 0 || ksplit == 4 || ksplit == 8),
              "skinny_linear_mfma: rt must be 0, 1 or 2 and ksplit 0, 4 or 8");
  const float* sp = nullptr;
  if (fp8) {
    TORCH_CHECK(scale->is_cuda() && scale->device() == x.device()
                && scale->dtype() == torch::kFloat32 && scale->dim() == 1
                && scale->size(0) == N && scale->is_contiguous(),
                "skinny_linear_mfma: scale must be contiguous device fp32 [N]");
    sp = scale->data_ptr<float>();
  }
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == x.device()
                && bias->dtype() == torch::kBFloat16 && bias->dim() == 1
                && bias->size(0) == N && bias->is_contiguous(),
                "skinny_linear_mfma: bias must be contiguous device bf16 [N]");
    bp = (const unsigned short*)bias->data_ptr();
  }
  const int r = rt == 0 ? MFMA_GEMV_RT : (int)rt;
  const int ks = ksplit == 0 ? MFMA_GEMV_KSPLIT : (int)ksplit;
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (fp8) {
    if (M <= MFMA_GEMV_TILE)
      dispatch_tiling<true, 1>(r, ks, x, w, sp, bp, y, stream);
    else
      dispatch_tiling<true, 2>(r, ks, x, w, sp, bp, y, stream);
  } else {
    if (M <= MFMA_GEMV_TILE)
      dispatch_tiling<false, 1>(r, ks, x, w, sp, bp, y, stream);
    else
      dispatch_tiling<false, 2>(r, ks, x, w, sp, bp, y, stream);
  }
  return y;
}
