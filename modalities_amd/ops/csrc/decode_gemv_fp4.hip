// Skinny GEMM on the matrix cores for weight-only MXFP4 decode weights:
// y[M, N] = x[M, K] . W[N, K]^T for 1 <= M <= 32, W streamed once from HBM
// straight to VGPRs at 0.53 bytes per weight. gfx950 only. Inference only.
//
// skinny_linear_mxfp4(x [M,K] bf16, codes uint8 [N,K/2],
//                     scales uint8 [N, 8, 4, T] (packed, below),
//                     bias bf16 [N] | None, rt) -> y [M,N] bf16
//
// Format (OCP microscaling FP4): a byte j of a row holds the e2m1 code of
// k = 2j in its low nibble and of k = 2j + 1 in its high nibble; one e8m0
// scale byte (2^(byte - 127)) per 32 k. A code times its scale is exact in
// bf16, and v_cvt_scalef32_pk_bf16_fp4 produces exactly that: one byte -> two
// scaled bf16 values, half a VALU op per weight, whatever M is. That is why
// there is one MFMA kernel for every M and no VALU sibling: a VALU kernel
// would spend about two lane-ops per weight at M = 1, which at this byte
// rate is already the vector ALU's limit (from peak rates, not measured).
//
//  * As in decode_gemv_mfma.hip the weight is the A operand and x^T the B
//    operand of v_mfma_f32_16x16x32_bf16: lane l holds, for A and B alike, 8
//    consecutive k of row l % 16 in k-group g = l / 16.
//  * A wave step is 64 contiguous bytes (128 k) of each of 16 weight rows:
//    lane (row, g) takes the 16-byte chunk c = 4 * step + g of its row with
//    one non-temporal load, no LDS stop. The chunk is 32 k: exactly one MX
//    block, so one scale per chunk, and the A fragments of four MFMAs: dword
//    h of the chunk (bytes 4h .. 4h + 3) is k = 32c + 8h .. 32c + 8h + 7,
//    widened by four converts (one per byte). The lane's x pieces are
//    x[m][32c + 8h ..], four 16-byte loads used in the same order.
//  * Scales are not fetched a byte at a time. The wrapper stores them in the
//    order a lane consumes them: [n][wave w][g][t] holds the scale of chunk
//    4 * (w + 8 t) + g, t padded to a multiple of 4 with 127 (2^0). The four
//    steps t = 4q .. 4q + 3 of a lane ("quad" q) are one aligned dword load.
//  * x traffic is what limits the e4m3 kernel at M = 32, and a chunk here
//    carries twice the k: 64 bytes of x per batch row per weight load. So a
//    workgroup owns 16 * RT weight rows with RT up to 4 (the weight
//    registers are half the e4m3 kernel's per k), and every x piece is reused
//    by RT row tiles in registers. A trip issues U = 4 / RT steps: 4 weight
//    loads in flight per lane (the k-depth of the e4m3 kernel's 8) and
//    16 * U * MTILES VGPRs of x. A quad is RT trips.
//  * Reduction order of one output (m, n), fixed: a wave adds its steps in
//    ascending order, the four fragments of a step in ascending order,
//    through the MFMA accumulator; waves 1..7 write their partial tiles to
//    LDS; after one barrier wave 0 adds them to its own in wave order.
//    Neither M, MTILES, RT nor the row's place in the batch enters it, so a
//    row's result is bit-identical for every M and every position. No
//    atomics, no split of K over workgroups.
//  * Epilogue: + bias[n], one rounding to bf16 (the scale is already in).
//  * Tails: weight rows past N re-read row N - 1 and batch rows past M re-read
//    row M - 1 (always inside the tensors); those results are never stored.
//    A wave step at or beyond the end of K issues no load. In the last,
//    partial step a chunk beyond K re-reads the row's last chunk (of W and
//    of x), its weight fragments are set to zero and its padded scale is 1.
//
// No launch argument depends on the decode step: graph-capturable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int FP4_GEMV_MAX_M = 32;
constexpr int FP4_GEMV_TILE = 16;        // weight rows / batch rows per tile
constexpr int FP4_GEMV_CHUNK_BYTES = 16;
constexpr int FP4_GEMV_CHUNK_K = 32;     // one MX block
constexpr int FP4_GEMV_GROUPS = 4;       // k-groups (chunks per row) per wave step
constexpr int FP4_GEMV_KSPLIT = 8;       // waves; fixed: it is in the scale layout
constexpr int FP4_GEMV_QUAD = 4;         // steps of a wave per scale dword
constexpr int FP4_GEMV_LOADS = 4;        // weight loads in flight per lane

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// eight e2m1 codes (one dword, k ascending from the low nibble of byte 0)
// times 2^(sbyte - 127) -> eight bf16, exactly
__device__ __forceinline__ bf16x8 fp4x8_to_bf16x8(unsigned int u, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u, scale, 3);
  return bf16x8{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}

// One trip of a wave's K loop: the wave steps s0, s0 + KSPLIT, ..., U of them;
// their scale bytes are bytes b0 .. b0 + U - 1 of sc[r]. FULL: every chunk of
// every step exists; otherwise the steps at or past S are skipped and the
// chunks c >= C of the last step count as zeros.
template <int MTILES, int RT, int U, bool FULL>
__device__ __forceinline__ void fp4_trip(
    const unsigned char* const (&wr)[RT],
    const unsigned short* const (&xr)[MTILES], const unsigned int (&sc)[RT],
    int b0, int s0, int g, int C, int S, floatx4 (&acc)[RT][MTILES]) {
  constexpr int H = FP4_GEMV_CHUNK_BYTES / 4;   // MFMAs (8 k each) per chunk
  // x first: its pieces come from L2 and are back before the weights
  // Not FULL: s0 is wave-uniform (an SGPR), so skipping a step at or past S
  // is a scalar branch; inside the last, partial step a lane whose chunk is
  // past C loads chunk C - 1 instead (inside the row) and zeroes the weight
  // afterwards. No load sits in a divergent branch, so none is serialised:
  // at K = 2560 a wave has 2 or 3 steps and this is the only path it runs.
  uintx4 xv[U][MTILES][H];
  uintx4 wq[U][RT];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && s0 + u * FP4_GEMV_KSPLIT >= S) break;   // the whole wave
    const int c = (s0 + u * FP4_GEMV_KSPLIT) * FP4_GEMV_GROUPS + g;
    const int cc = FULL ? c : min(c, C - 1);
#pragma unroll
    for (int m = 0; m < MTILES; ++m)
#pragma unroll
      for (int h = 0; h < H; ++h)
        xv[u][m][h] = *reinterpret_cast<const uintx4*>(
            xr[m] + (long)cc * FP4_GEMV_CHUNK_K + h * 8);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && s0 + u * FP4_GEMV_KSPLIT >= S) break;
    const int c = (s0 + u * FP4_GEMV_KSPLIT) * FP4_GEMV_GROUPS + g;
    const int cc = FULL ? c : min(c, C - 1);
#pragma unroll
    for (int r = 0; r < RT; ++r)
      wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(
          wr[r] + (long)cc * FP4_GEMV_CHUNK_BYTES));
  }
  // all U * RT weight loads are in flight before any is used
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && s0 + u * FP4_GEMV_KSPLIT >= S) break;   // the whole wave
    if (!FULL && (s0 + u * FP4_GEMV_KSPLIT) * FP4_GEMV_GROUPS + g >= C) {
#pragma unroll
      for (int r = 0; r < RT; ++r) wq[u][r] = uintx4{0u, 0u, 0u, 0u};
    }
    float scale[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r)   // e8m0 byte -> the fp32 with that exponent
      scale[r] = __uint_as_float(((sc[r] >> (8 * (b0 + u))) & 0xFFu) << 23);
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const bf16x8 a = fp4x8_to_bf16x8(wq[u][r][h], scale[r]);
#pragma unroll
        for (int m = 0; m < MTILES; ++m)
          acc[r][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, xv[u][m][h]), acc[r][m], 0, 0, 0);
      }
  }
}

template <int MTILES, int RT>
__global__ __launch_bounds__(FP4_GEMV_KSPLIT * WAVE_SIZE)
void skinny_linear_mxfp4_kernel(const unsigned short* __restrict__ x, long x_sm,
                                const unsigned char* __restrict__ w,
                                const unsigned char* __restrict__ scales,
                                const unsigned short* __restrict__ bias,
                                unsigned short* __restrict__ y, int M, int N,
                                int C,     // 16-byte chunks (MX blocks) per row
                                int T) {   // padded steps per wave (scales)
  constexpr int KSPLIT = FP4_GEMV_KSPLIT;
  static_assert(FP4_GEMV_LOADS % RT == 0 && FP4_GEMV_QUAD == FP4_GEMV_LOADS,
                "tiling");
  constexpr int U = FP4_GEMV_LOADS / RT;   // steps per trip; RT trips per quad
  constexpr int TILES = RT * MTILES;
  __shared__ floatx4 part[(KSPLIT - 1) * TILES * WAVE_SIZE];
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  // wave-uniform by construction; said so, the step predicates are scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE_SIZE);
  const int row = lane & (FP4_GEMV_TILE - 1);   // n of A, m of B
  const int g = lane / FP4_GEMV_TILE;           // k-group
  const int n0 = blockIdx.x * (FP4_GEMV_TILE * RT);

  const unsigned char* wr[RT];
  const unsigned char* sr[RT];   // this lane's scale bytes, t ascending
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const long n = min(n0 + r * FP4_GEMV_TILE + row, N - 1);
    wr[r] = w + n * C * FP4_GEMV_CHUNK_BYTES;
    sr[r] = scales + ((n * KSPLIT + wave) * FP4_GEMV_GROUPS + g) * T;
  }
  const unsigned short* xr[MTILES];
#pragma unroll
  for (int m = 0; m < MTILES; ++m)
    xr[m] = x + (long)min(m * FP4_GEMV_TILE + row, M - 1) * x_sm;

  floatx4 acc[RT][MTILES];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int m = 0; m < MTILES; ++m) acc[r][m] = floatx4{0.f, 0.f, 0.f, 0.f};

  // wave steps in K (the last may be partial); this wave takes s = wave,
  // wave + KSPLIT, ..., a quad of them per scale dword. s < S implies
  // t = (s - wave) / KSPLIT < T, so every dword read lies inside the row.
  const int S = (C + FP4_GEMV_GROUPS - 1) / FP4_GEMV_GROUPS;
  int s0 = wave, t0 = 0;
  for (; (s0 + (FP4_GEMV_QUAD - 1) * KSPLIT + 1) * FP4_GEMV_GROUPS <= C;
       s0 += FP4_GEMV_QUAD * KSPLIT, t0 += FP4_GEMV_QUAD) {
    unsigned int sc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
      sc[r] = *reinterpret_cast<const unsigned int*>(sr[r] + t0);
#pragma unroll
    for (int p = 0; p < RT; ++p)
      fp4_trip<MTILES, RT, U, true>(wr, xr, sc, p * U, s0 + p * U * KSPLIT, g,
                                    C, S, acc);
  }
  for (; s0 < S; s0 += FP4_GEMV_QUAD * KSPLIT, t0 += FP4_GEMV_QUAD) {
    unsigned int sc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
      sc[r] = *reinterpret_cast<const unsigned int*>(sr[r] + t0);
#pragma unroll
    for (int p = 0; p < RT; ++p)
      if (s0 + p * U * KSPLIT < S)   // the whole wave
        fp4_trip<MTILES, RT, U, false>(wr, xr, sc, p * U,
                                       s0 + p * U * KSPLIT, g, C, S, acc);
  }

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
  // not unrolled: up to 8 tiles per wave, and hoisting all 7 waves' reads
  // would take 224 registers
#pragma unroll 1
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
      const int mm = m * FP4_GEMV_TILE + row;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + r * FP4_GEMV_TILE + g * 4 + i;
        if (mm < M && n < N) {
          float s = acc[r][m][i];
          if (bias != nullptr) s = __fadd_rn(s, bf16_to_f32(bias[n]));
          y[(long)mm * N + n] = f32_to_bf16(s);
        }
      }
    }
}

template <int MTILES, int RT>
void launch_fp4(const torch::Tensor& x, const torch::Tensor& w,
                const torch::Tensor& scales, const unsigned short* bias,
                torch::Tensor& y, hipStream_t stream) {
  const int M = x.size(0), N = w.size(0);
  const int C = (int)(w.size(1) / FP4_GEMV_CHUNK_BYTES);
  const int rows_per_wg = FP4_GEMV_TILE * RT;
  hipLaunchKernelGGL((skinny_linear_mxfp4_kernel<MTILES, RT>),
                     dim3((N + rows_per_wg - 1) / rows_per_wg),
                     dim3(FP4_GEMV_KSPLIT * WAVE_SIZE), 0, stream,
                     (const unsigned short*)x.data_ptr(), (long)x.stride(0),
                     (const unsigned char*)w.data_ptr(),
                     (const unsigned char*)scales.data_ptr(), bias,
                     (unsigned short*)y.data_ptr(), M, N, C,
                     (int)scales.size(3));
  HIP_CHECK_KERNEL();
}

template <int MTILES>
void dispatch_rt(int rt, const torch::Tensor& x, const torch::Tensor& w,
                 const torch::Tensor& scales, const unsigned short* bias,
                 torch::Tensor& y, hipStream_t stream) {
  if (rt == 1) launch_fp4<MTILES, 1>(x, w, scales, bias, y, stream);
  else if (rt == 2) launch_fp4<MTILES, 2>(x, w, scales, bias, y, stream);
  else launch_fp4<MTILES, 4>(x, w, scales, bias, y, stream);
}

bool aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

}  // namespace

// Steps per wave the packed scale layout holds for K: the wave's share of the
// ceil(K / 128) wave steps, rounded up to whole quads.
long skinny_linear_mxfp4_scale_steps(long K) {
  const long S = (K / FP4_GEMV_CHUNK_K + FP4_GEMV_GROUPS - 1) / FP4_GEMV_GROUPS;
  const long per_wave = (S + FP4_GEMV_KSPLIT - 1) / FP4_GEMV_KSPLIT;
  return (per_wave + FP4_GEMV_QUAD - 1) / FP4_GEMV_QUAD * FP4_GEMV_QUAD;
}

// rt: weight-row tiles of 16 per workgroup (1, 2 or 4). It does not enter a
// result; the Python wrapper picks it by N.
torch::Tensor skinny_linear_mxfp4(torch::Tensor x, torch::Tensor codes,
                                  torch::Tensor scales,
                                  c10::optional<torch::Tensor> bias, long rt) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.dtype() == torch::kBFloat16,
              "skinny_linear_mxfp4: x must be device bf16 [M, K]");
  TORCH_CHECK(codes.is_cuda() && codes.dim() == 2
              && codes.device() == x.device() && codes.is_contiguous()
              && codes.dtype() == torch::kUInt8,
              "skinny_linear_mxfp4: codes must be contiguous uint8 [N, K/2] on "
              "x's device");
  const long M = x.size(0), K = x.size(1), N = codes.size(0);
  TORCH_CHECK(M >= 1 && M <= FP4_GEMV_MAX_M,
              "skinny_linear_mxfp4: M must be in [1, ", FP4_GEMV_MAX_M,
              "], got ", M);
  TORCH_CHECK(K >= FP4_GEMV_CHUNK_K && K % FP4_GEMV_CHUNK_K == 0
              && codes.size(1) * 2 == K,
              "skinny_linear_mxfp4: x [M, K] and codes [N, K/2] must share K, "
              "a positive multiple of 32; got ", K, " and ", codes.size(1) * 2);
  // chunk and step indices are int in the kernel
  TORCH_CHECK(N >= 1 && N < (1L << 31) && K < (1L << 31)
              && N * K < (1L << 40),
              "skinny_linear_mxfp4: N or K out of range");
  TORCH_CHECK(x.stride(1) == 1 && (M == 1 || x.stride(0) % 8 == 0)
              && aligned16(x) && aligned16(codes),
              "skinny_linear_mxfp4: x needs unit stride in K and 16-byte "
              "aligned rows; codes a 16-byte aligned base");
  TORCH_CHECK(scales.is_cuda() && scales.device() == x.device()
              && scales.dtype() == torch::kUInt8 && scales.dim() == 4
              && scales.size(0) == N && scales.size(1) == FP4_GEMV_KSPLIT
              && scales.size(2) == FP4_GEMV_GROUPS
              && scales.size(3) == skinny_linear_mxfp4_scale_steps(K)
              && scales.is_contiguous() && aligned16(scales),
              "skinny_linear_mxfp4: scales must be the packed contiguous "
              "device uint8 [N, 8, 4, steps] of pack_mxfp4_scales");
  TORCH_CHECK(rt == 1 || rt == 2 || rt == 4,
              "skinny_linear_mxfp4: rt must be 1, 2 or 4");
  const unsigned short* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->device() == x.device()
                && bias->dtype() == torch::kBFloat16 && bias->dim() == 1
                && bias->size(0) == N && bias->is_contiguous(),
                "skinny_linear_mxfp4: bias must be contiguous device bf16 [N]");
    bp = (const unsigned short*)bias->data_ptr();
  }
  auto y = torch::empty({M, N}, x.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (M <= FP4_GEMV_TILE)
    dispatch_rt<1>((int)rt, x, codes, scales, bp, y, stream);
  else
    dispatch_rt<2>((int)rt, x, codes, scales, bp, y, stream);
  return y;
}
