// K1 decode over an e4m3 KV cache: the quantising prefill store, the fused
// RoPE + quantising append, and split-KV single-token attention that reads
// the codes. Inference only.
//
// Format, per cache row x[D] (one batch row, position and kv head; bf16 in):
//   amax = max |x[d]|, scale = 2^ceil(log2(amax / 448)) (1 when amax == 0),
//   code[d] = e4m3(x[d] / scale), OCP e4m3, round to nearest even.
// codes: float8_e4m3fn [B, Lmax, Hkv, D]; scales: fp32 [B, Lmax, Hkv]. The
// exponent comes from frexp (amax = m * 2^e, m in [0.5, 1), 448 = 0.875 *
// 2^9, so ceil(log2(amax / 448)) = e - 9 + (m > 0.875)) and the division is
// an ldexp: no rounding anywhere before the e4m3 conversion
// (v_cvt_pk_fp8_f32), so the codes and scales are those of the torch
// expression in ops/attention.py bit for bit.
//
// kv_quantize_store(k, v [B,T,Hkv,D] bf16, possibly strided; host pos):
//   writes cache[:, pos : pos + T]. A lane holds 8 adjacent elements (one
//   16-byte load), LQ = 8 (D = 64) or 16 (D = 80: 10 of them hold data;
//   D = 128) adjacent lanes hold a row, so a 256-thread workgroup takes 32
//   or 16 rows. The row stays in registers: amax by xor shuffles over the LQ
//   lanes, then one 8-byte store of codes per lane and one scale per row.
//
// decode_rope_append_fp8: the contract of decode_rope_append (device-side
//   pos[b], optional tables, strided q/k/v). A row is one q, k or v head; a
//   lane holds 4 elements of the lower half and the 4 rotate-half partners
//   of the upper half, so the rotation is lane-local and D / 8 lanes of a
//   group of LQ hold a row. q rows are rotated and stored as bf16; k rows
//   are rotated, rounded to bf16 (the value the bf16 append stores), then
//   quantised like v rows: amax by shuffles, two 4-byte code stores per lane.
//
// decode_attn_fp8_fwd: the contract of decode_attn_fwd (attention_decode.hip)
//   with code and scale caches. The combine launch is shared; the partial
//   kernel is laid out for 1-byte elements:
//   * a 16-byte load carries 16 elements, a row is D / 16 pieces (4, 5, 8),
//     held by LPR = 4 (D = 64) or 8 (D = 80: 5 load; D = 128) adjacent
//     lanes: SLOTS = 256 / LPR = 64 or 32 row slots, and the score of a key
//     is reduced over 2 or 3 shuffle steps instead of 3 or 4.
//   * a lane keeps 16 q and 16 accumulator floats per resident query head,
//     so R <= 4 heads of a GQA group are resident (ngroups = ceil(rep / 4)
//     workgroups share a kv head when rep > 4).
//   * key j of a chunk belongs to slot (j - chunk_start) % SLOTS; a slot
//     takes its keys UNROLL = 4 at a time (eight 16-byte loads and eight
//     scale loads in flight before the first use), then singly: the paths
//     change at chunk offsets SLOTS and 4 * SLOTS (64/256 for D = 64, 32/128
//     for D = 80, 128).
//   * codes are widened by v_cvt_pk_f32_fp8. The K scale multiplies the
//     reduced score once per key, the V scale is folded into p before the
//     accumulation; both are powers of two, so both are exact.
//   * nothing at or beyond kv_lens[b] is read, neither codes nor scales.
#include "attention_decode_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;
typedef __attribute__((ext_vector_type(2))) unsigned int uintx2;

constexpr int DEC8_MAX_R = 4;   // query heads resident per workgroup

// a code cache and its scales, with strides in elements
struct Fp8Cache {
  unsigned char* codes;
  long c_sb, c_sr, c_sh;
  float* scale;
  long s_sb, s_sr, s_sh;
};

// ---------------------------------------------------------------------------
// quantisation of a row held by `lanes` adjacent lanes, 8 elements each
// ---------------------------------------------------------------------------
__device__ __forceinline__ int row_scale_exp(float amax) {
  int e;
  const float m = frexpf(amax, &e);
  return amax > 0.f ? e - 9 + (m > 0.875f ? 1 : 0) : 0;
}

// x[0..7] -> two dwords of e4m3 codes (x[0] in the lowest byte) and the
// row's scale exponent; every lane of the wave must call it
template <int LANES>
__device__ __forceinline__ uintx2 quantize8(const float (&x)[8], int& sexp) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, WAVE_SIZE));
  sexp = row_scale_exp(amax);
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = ldexpf(x[i], -sexp);
  uintx2 c;
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
  c.x = (unsigned int)w;
  w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w, true);
  c.y = (unsigned int)w;
  return c;
}

// source n (0: k, 1: v) row (b, t, h) -> cache n row (b, pos + t, h)
template <int LQ>
__global__ __launch_bounds__(DEC_THREADS)
void kv_quantize_store_kernel(const unsigned short* __restrict__ x0,
                              const unsigned short* __restrict__ x1,
                              long x_sb0, long x_st0, long x_sh0,
                              long x_sb1, long x_st1, long x_sh1,
                              Fp8Cache c0, Fp8Cache c1, long rows, int T,
                              int H, int D, int pos) {
  constexpr int RPB = DEC_THREADS / LQ;
  const int piece = threadIdx.x % LQ;
  const long row = (long)blockIdx.x * RPB + threadIdx.x / LQ;
  const int n = blockIdx.y;
  const bool live = row < rows && piece * 8 < D;
  const long rr = min(row, rows - 1);
  const int h = (int)(rr % H);
  const int t = (int)((rr / H) % T);
  const long b = rr / ((long)H * T);
  const unsigned short* x = n == 0 ? x0 : x1;
  const long sb = n == 0 ? x_sb0 : x_sb1, st = n == 0 ? x_st0 : x_st1;
  const long sh = n == 0 ? x_sh0 : x_sh1;
  const Fp8Cache c = n == 0 ? c0 : c1;

  float xf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) xf[i] = 0.f;
  if (live) {
    const shortx8 v = *reinterpret_cast<const shortx8*>(
        x + b * sb + t * st + h * sh + piece * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) xf[i] = bf16_to_f32((unsigned short)v[i]);
  }
  int sexp;
  const uintx2 codes = quantize8<LQ>(xf, sexp);
  if (!live) return;
  *reinterpret_cast<uintx2*>(c.codes + b * c.c_sb + (long)(pos + t) * c.c_sr
                             + h * c.c_sh + piece * 8) = codes;
  if (piece == 0)
    c.scale[b * c.s_sb + (long)(pos + t) * c.s_sr + h * c.s_sh] =
        ldexpf(1.f, sexp);
}

__device__ __forceinline__ void unpack4(uintx2 u, float* f) {
  f[0] = __uint_as_float(u.x << 16);
  f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16);
  f[3] = __uint_as_float(u.y & 0xffff0000u);
}

__device__ __forceinline__ uintx2 pack4(const float* f) {
  uintx2 u;
  u.x = (unsigned int)f32_to_bf16(f[0])
      | ((unsigned int)f32_to_bf16(f[1]) << 16);
  u.y = (unsigned int)f32_to_bf16(f[2])
      | ((unsigned int)f32_to_bf16(f[3]) << 16);
  return u;
}

// Row = one head of q (rows 0 .. Hq-1), k (the next Hkv) or v (the last
// Hkv) of batch row blockIdx.y. Lane `piece` of a row's LQ lanes holds
// elements [4 piece, 4 piece + 4) and their partners at + D / 2.
template <int LQ>
__global__ __launch_bounds__(DEC_THREADS)
void decode_rope_append_fp8_kernel(
    const unsigned short* __restrict__ q, long q_sb,
    const unsigned short* __restrict__ k, long k_sb,
    const unsigned short* __restrict__ v, long v_sb,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos, unsigned short* __restrict__ q_out,
    Fp8Cache kc, Fp8Cache vc, int Hq, int Hkv, int D, int Lmax) {
  constexpr int RPB = DEC_THREADS / LQ;
  const int halfD = D / 2;
  const int piece = threadIdx.x % LQ;
  const int row = blockIdx.x * RPB + threadIdx.x / LQ;
  const int b = blockIdx.y;
  const bool live = row < Hq + 2 * Hkv && piece * 8 < D;
  const bool is_q = row < Hq;
  const int t = pos[b];
  if (t < 0 || t >= Lmax) {   // the whole workgroup: q is defined as zero
    if (live && is_q) {
      unsigned short* dst = q_out + ((long)b * Hq + row) * D + piece * 4;
      *reinterpret_cast<uintx2*>(dst) = uintx2{0u, 0u};
      *reinterpret_cast<uintx2*>(dst + halfD) = uintx2{0u, 0u};
    }
    return;
  }
  const bool is_k = !is_q && row < Hq + Hkv;
  const int h = is_q ? row : (is_k ? row - Hq : row - Hq - Hkv);

  float xf[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) xf[i] = 0.f;
  if (live) {
    const unsigned short* src =
        (is_q ? q + (long)b * q_sb : is_k ? k + (long)b * k_sb
                                          : v + (long)b * v_sb)
        + (long)h * D + piece * 4;
    unpack4(*reinterpret_cast<const uintx2*>(src), xf);
    unpack4(*reinterpret_cast<const uintx2*>(src + halfD), xf + 4);
    if (cos_t != nullptr && (is_q || is_k)) {
      // the operation order of decode_rope_append_kernel, spelled out so
      // that both kernels round alike whatever the compiler contracts
      float r[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float c = cos_t[t * halfD + piece * 4 + i];
        const float s = sin_t[t * halfD + piece * 4 + i];
        r[i] = __fmaf_rn(xf[i], c, -__fmul_rn(xf[4 + i], s));
        r[4 + i] = __fmaf_rn(xf[4 + i], c, __fmul_rn(xf[i], s));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) xf[i] = bf16_to_f32(f32_to_bf16(r[i]));
    }
    if (is_q) {
      unsigned short* dst = q_out + ((long)b * Hq + row) * D + piece * 4;
      *reinterpret_cast<uintx2*>(dst) = pack4(xf);
      *reinterpret_cast<uintx2*>(dst + halfD) = pack4(xf + 4);
    }
  }
  int sexp;
  const uintx2 codes = quantize8<LQ>(xf, sexp);
  if (!live || is_q) return;
  const Fp8Cache c = is_k ? kc : vc;
  unsigned char* dst = c.codes + (long)b * c.c_sb + (long)t * c.c_sr
      + (long)h * c.c_sh + piece * 4;
  *reinterpret_cast<unsigned int*>(dst) = codes.x;
  *reinterpret_cast<unsigned int*>(dst + halfD) = codes.y;
  if (piece == 0)
    c.scale[(long)b * c.s_sb + (long)t * c.s_sr + (long)h * c.s_sh] =
        ldexpf(1.f, sexp);
}

// ---------------------------------------------------------------------------
// split-KV attention over the codes
// ---------------------------------------------------------------------------
__device__ __forceinline__ void widen16(const uintx4& c, float (&f)[16]) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const floatx2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(c[w], false);
    const floatx2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(c[w], true);
    f[4 * w] = lo.x;
    f[4 * w + 1] = lo.y;
    f[4 * w + 2] = hi.x;
    f[4 * w + 3] = hi.y;
  }
}

template <int D, int R>
__global__ __launch_bounds__(DEC_THREADS)
void decode_fp8_partial_kernel(const unsigned short* __restrict__ q,
                               long q_sb, Fp8Cache kc, Fp8Cache vc,
                               const int* __restrict__ kv_lens,
                               float* __restrict__ ws_ml,
                               float* __restrict__ ws_acc,
                               int Lmax, int Hq, int rep, int ngroups,
                               int chunk, int NC, float scale2) {
  constexpr int LPR = (D == 64) ? 4 : 8;
  constexpr int PIECES = D / 16;
  constexpr int SLOTS = DEC_THREADS / LPR;
  __shared__ float sm_ml[DEC_WAVES][R][2];
  __shared__ float sm_acc[DEC_WAVES][R][D];

  const int c = blockIdx.x;
  const int hk = blockIdx.y / ngroups;
  const int r0 = (blockIdx.y % ngroups) * R;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int piece = lane % LPR;
  const int slot = tid / LPR;
  const bool active = piece < PIECES;
  const int nr = min(R, rep - r0);        // query heads of this workgroup
  const int hq0 = hk * rep + r0;

  int len = kv_lens[b];
  len = min(max(len, 0), Lmax);
  const int start = c * chunk;
  const int end = min(start + chunk, len);
  const long part0 = ((long)b * Hq + hq0) * NC + c;   // + r * NC per head

  if (start >= len) {   // nothing to read: the neutral partial
    for (int i = tid; i < nr * D; i += DEC_THREADS) {
      const int r = i / D, d = i % D;
      ws_acc[(part0 + (long)r * NC) * D + d] = 0.f;
      if (d == 0) {
        ws_ml[(part0 + (long)r * NC) * 2] = -INFINITY;
        ws_ml[(part0 + (long)r * NC) * 2 + 1] = 0.f;
      }
    }
    return;
  }

  // q rows of the group, pre-scaled into the exp2 domain
  float qf[R][16];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int i = 0; i < 16; ++i) qf[r][i] = 0.f;
    if (active && r < nr) {
      const unsigned short* qp =
          q + (long)b * q_sb + (long)(hq0 + r) * D + piece * 16;
#pragma unroll
      for (int hlf = 0; hlf < 2; ++hlf) {
        const shortx8 qq = *reinterpret_cast<const shortx8*>(qp + hlf * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          qf[r][hlf * 8 + i] = bf16_to_f32((unsigned short)qq[i]) * scale2;
      }
    }
  }

  float m[R], l[R], acc[R][16];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[r][i] = 0.f;
  }

  const unsigned char* kb =
      kc.codes + (long)b * kc.c_sb + (long)hk * kc.c_sh + piece * 16;
  const unsigned char* vb =
      vc.codes + (long)b * vc.c_sb + (long)hk * vc.c_sh + piece * 16;
  const float* ksb = kc.scale + (long)b * kc.s_sb + (long)hk * kc.s_sh;
  const float* vsb = vc.scale + (long)b * vc.s_sb + (long)hk * vc.s_sh;
  const uintx4 zero4 = {0u, 0u, 0u, 0u};

  int j = start + slot;
  // UNROLL keys of this slot per trip; every j + u * SLOTS < end <= len
  for (; j + (DEC_UNROLL - 1) * SLOTS < end; j += DEC_UNROLL * SLOTS) {
    uintx4 kk[DEC_UNROLL], vv[DEC_UNROLL];
    float ksc[DEC_UNROLL], vsc[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const long ju = j + u * SLOTS;
      kk[u] = zero4;
      vv[u] = zero4;
      if (active) {
        kk[u] = *reinterpret_cast<const uintx4*>(kb + ju * kc.c_sr);
        vv[u] = *reinterpret_cast<const uintx4*>(vb + ju * vc.c_sr);
      }
      ksc[u] = ksb[ju * kc.s_sr];
      vsc[u] = vsb[ju * vc.s_sr];
    }
    float s[DEC_UNROLL][R];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float kf[16];
      widen16(kk[u], kf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float d0 = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) d0 = fmaf(qf[r][i], kf[i], d0);
        s[u][r] = d0;
      }
    }
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
          s[u][r] += __shfl_xor(s[u][r], off, WAVE_SIZE);
    // s becomes p = exp2(score - m_new)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mn = m[r];
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u) {
        s[u][r] *= ksc[u];
        mn = fmaxf(mn, s[u][r]);
      }
      const float alpha = __builtin_amdgcn_exp2f(m[r] - mn);
      m[r] = mn;
      l[r] *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[r][i] *= alpha;
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u) {
        s[u][r] = __builtin_amdgcn_exp2f(s[u][r] - mn);
        l[r] += s[u][r];
      }
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float vf[16];
      widen16(vv[u], vf);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float pv = s[u][r] * vsc[u];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[r][i] = fmaf(pv, vf[i], acc[r][i]);
      }
    }
  }
  // tail: one key per trip
  for (; j < end; j += SLOTS) {
    uintx4 kk = zero4, vv = zero4;
    if (active) {
      kk = *reinterpret_cast<const uintx4*>(kb + (long)j * kc.c_sr);
      vv = *reinterpret_cast<const uintx4*>(vb + (long)j * vc.c_sr);
    }
    const float ksc = ksb[(long)j * kc.s_sr];
    const float vsc = vsb[(long)j * vc.s_sr];
    float kf[16], vf[16], s[R];
    widen16(kk, kf);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float d0 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) d0 = fmaf(qf[r][i], kf[i], d0);
      s[r] = d0;
    }
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] += __shfl_xor(s[r], off, WAVE_SIZE);
    widen16(vv, vf);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float sr = s[r] * ksc;
      const float mn = fmaxf(m[r], sr);
      const float alpha = __builtin_amdgcn_exp2f(m[r] - mn);
      const float p = __builtin_amdgcn_exp2f(sr - mn);
      const float pv = p * vsc;
      m[r] = mn;
      l[r] = fmaf(l[r], alpha, p);
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[r][i] = fmaf(pv, vf[i], acc[r][i] * alpha);
    }
  }

  // merge the slots of a wave (lane bits LPR .. 32); slot 0 of the wave ends
  // up with the wave's state
#pragma unroll
  for (int off = LPR; off < WAVE_SIZE; off <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float mo = __shfl_xor(m[r], off, WAVE_SIZE);
      const float mn = fmaxf(m[r], mo);
      const float ws = dec_weight(m[r], mn);
      const float wo = dec_weight(mo, mn);
      l[r] = l[r] * ws + __shfl_xor(l[r], off, WAVE_SIZE) * wo;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[r][i] = acc[r][i] * ws
            + __shfl_xor(acc[r][i], off, WAVE_SIZE) * wo;
      m[r] = mn;
    }
  }
  if (lane < LPR && active) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (piece == 0) {
        sm_ml[wave][r][0] = m[r];
        sm_ml[wave][r][1] = l[r];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) sm_acc[wave][r][piece * 16 + i] = acc[r][i];
    }
  }
  __syncthreads();

  // merge the waves in a fixed order and write the partial
  for (int i = tid; i < nr * D; i += DEC_THREADS) {
    const int r = i / D, d = i % D;
    float mw = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) mw = fmaxf(mw, sm_ml[w][r][0]);
    float lw = 0.f, aw = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float wt = dec_weight(sm_ml[w][r][0], mw);
      lw += sm_ml[w][r][1] * wt;
      aw += sm_acc[w][r][d] * wt;
    }
    ws_acc[(part0 + (long)r * NC) * D + d] = aw;
    if (d == 0) {
      ws_ml[(part0 + (long)r * NC) * 2] = mw;
      ws_ml[(part0 + (long)r * NC) * 2 + 1] = lw;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// codes: device e4m3 [B, L, H, D] with unit stride in D and every other
// offset a multiple of `align` bytes; scale: device fp32 [B, L, H]
bool fp8_cache_ok(const torch::Tensor& codes, const torch::Tensor& scale,
                  const torch::Tensor& ref, long align) {
  return codes.is_cuda() && codes.device() == ref.device()
      && codes.dtype() == torch::kFloat8_e4m3fn && codes.dim() == 4
      && codes.stride(3) == 1 && strides_aligned(codes, 3, align)
      && scale.is_cuda() && scale.device() == ref.device()
      && scale.dtype() == torch::kFloat32 && scale.dim() == 3
      && scale.size(0) == codes.size(0) && scale.size(1) == codes.size(1)
      && scale.size(2) == codes.size(2);
}

Fp8Cache fp8_cache(const torch::Tensor& codes, const torch::Tensor& scale) {
  return Fp8Cache{(unsigned char*)codes.data_ptr(), (long)codes.stride(0),
                  (long)codes.stride(1), (long)codes.stride(2),
                  scale.data_ptr<float>(), (long)scale.stride(0),
                  (long)scale.stride(1), (long)scale.stride(2)};
}

bool fp8_head_dim_ok(long D) { return D == 64 || D == 80 || D == 128; }

template <int D, int R>
void launch_fp8_partial(const torch::Tensor& q, const Fp8Cache& kc,
                        const Fp8Cache& vc, const torch::Tensor& kv_lens,
                        torch::Tensor& ws_ml, torch::Tensor& ws_acc, int Lmax,
                        int Hkv, int rep, int chunk, int NC,
                        hipStream_t stream) {
  const int B = q.size(0), Hq = q.size(2);
  const int ngroups = (rep + R - 1) / R;
  const float scale2 = 1.44269504f / sqrtf((float)D);
  hipLaunchKernelGGL((decode_fp8_partial_kernel<D, R>),
                     dim3(NC, Hkv * ngroups, B), dim3(DEC_THREADS), 0, stream,
                     (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                     kc, vc, kv_lens.data_ptr<int>(),
                     ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(), Lmax,
                     Hq, rep, ngroups, chunk, NC, scale2);
}

template <int D>
void launch_fp8_decode(const torch::Tensor& q, const Fp8Cache& kc,
                       const Fp8Cache& vc, const torch::Tensor& kv_lens,
                       torch::Tensor& ws_ml, torch::Tensor& ws_acc,
                       torch::Tensor& o, torch::Tensor& lse, int Lmax,
                       int Hkv, int chunk, int NC, hipStream_t stream) {
  const int B = q.size(0), Hq = q.size(2);
  const int rep = Hq / Hkv;
  if (rep == 1)
    launch_fp8_partial<D, 1>(q, kc, vc, kv_lens, ws_ml, ws_acc, Lmax, Hkv,
                             rep, chunk, NC, stream);
  else if (rep == 2)
    launch_fp8_partial<D, 2>(q, kc, vc, kv_lens, ws_ml, ws_acc, Lmax, Hkv,
                             rep, chunk, NC, stream);
  else
    launch_fp8_partial<D, DEC8_MAX_R>(q, kc, vc, kv_lens, ws_ml, ws_acc,
                                      Lmax, Hkv, rep, chunk, NC, stream);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL((decode_combine_kernel<D>), dim3(Hq, B), dim3(128), 0,
                     stream, ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(),
                     kv_lens.data_ptr<int>(), (unsigned short*)o.data_ptr(),
                     lse.data_ptr<float>(), Lmax, Hq, chunk, NC);
  HIP_CHECK_KERNEL();
}

// x: device bf16 [B, T, H, D], unit stride in D, 16-byte aligned offsets
bool kv_source_ok(const torch::Tensor& x, const torch::Tensor& ref) {
  return x.is_cuda() && x.device() == ref.device()
      && x.dtype() == torch::kBFloat16 && x.dim() == 4
      && x.sizes() == ref.sizes() && x.stride(3) == 1
      && strides_aligned(x, 3, 8);
}

}  // namespace

void kv_quantize_store(torch::Tensor k, c10::optional<torch::Tensor> v,
                       torch::Tensor k_codes, torch::Tensor k_scale,
                       c10::optional<torch::Tensor> v_codes,
                       c10::optional<torch::Tensor> v_scale, long pos) {
  TORCH_CHECK(k.dim() == 4, "kv_quantize_store: k must be [B,T,Hkv,D]");
  const long B = k.size(0), T = k.size(1), H = k.size(2), D = k.size(3);
  TORCH_CHECK(fp8_head_dim_ok(D),
              "kv_quantize_store: head_dim must be 64, 80 or 128, got ", D);
  TORCH_CHECK(v.has_value() == v_codes.has_value()
              && v.has_value() == v_scale.has_value(),
              "kv_quantize_store: give v, v_codes and v_scale or none of "
              "them");
  const int nsrc = v.has_value() ? 2 : 1;
  TORCH_CHECK(kv_source_ok(k, k) && (nsrc == 1 || kv_source_ok(*v, k)),
              "kv_quantize_store: k, v must be device bf16 [B,T,Hkv,D] of one "
              "shape, unit stride in D and 16-byte aligned batch/row/head "
              "strides");
  const torch::Tensor& vcod = nsrc == 2 ? *v_codes : k_codes;
  const torch::Tensor& vsc = nsrc == 2 ? *v_scale : k_scale;
  TORCH_CHECK(fp8_cache_ok(k_codes, k_scale, k, 8)
              && fp8_cache_ok(vcod, vsc, k, 8)
              && k_codes.sizes() == vcod.sizes() && k_codes.size(0) == B
              && k_codes.size(2) == H && k_codes.size(3) == D,
              "kv_quantize_store: the caches must be device float8_e4m3fn "
              "[B,Lmax,Hkv,D] (unit stride in D, 8-byte aligned strides) "
              "with fp32 scales [B,Lmax,Hkv]");
  TORCH_CHECK(pos >= 0 && pos + T <= k_codes.size(1),
              "kv_quantize_store: rows ", pos, " .. ", pos + T,
              " do not fit a cache of ", k_codes.size(1));
  const long rows = B * T * H;
  if (rows == 0) return;
  TORCH_CHECK(T < (1L << 30) && H < (1L << 30) && rows < (1L << 40),
              "kv_quantize_store: too many rows");
  const torch::Tensor& vv = nsrc == 2 ? *v : k;
  auto stream = at::cuda::getCurrentHIPStream();
  const int LQ = D == 64 ? 8 : 16;
  const long rpb = DEC_THREADS / LQ;
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb), nsrc);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(DEC_THREADS), 0, stream,
                       (const unsigned short*)k.data_ptr(),
                       (const unsigned short*)vv.data_ptr(),
                       (long)k.stride(0), (long)k.stride(1),
                       (long)k.stride(2), (long)vv.stride(0),
                       (long)vv.stride(1), (long)vv.stride(2),
                       fp8_cache(k_codes, k_scale), fp8_cache(vcod, vsc),
                       rows, (int)T, (int)H, (int)D, (int)pos);
  };
  if (LQ == 8) launch(kv_quantize_store_kernel<8>);
  else launch(kv_quantize_store_kernel<16>);
  HIP_CHECK_KERNEL();
}

torch::Tensor decode_rope_append_fp8(torch::Tensor q, torch::Tensor k,
                                     torch::Tensor v,
                                     c10::optional<torch::Tensor> cos_t,
                                     c10::optional<torch::Tensor> sin_t,
                                     torch::Tensor pos, torch::Tensor k_codes,
                                     torch::Tensor k_scale,
                                     torch::Tensor v_codes,
                                     torch::Tensor v_scale) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && k_codes.dim() == 4,
              "decode_rope_append_fp8: q/k/v must be [B,1,H,D], caches "
              "[B,Lmax,Hkv,D]");
  const long B = q.size(0), Hq = q.size(2), D = q.size(3), Hkv = k.size(2);
  const long Lmax = k_codes.size(1);
  TORCH_CHECK(fp8_head_dim_ok(D), "decode_rope_append_fp8: head_dim must be "
              "64, 80 or 128, got ", D);
  TORCH_CHECK(token_ok(q, B, Hq, D) && token_ok(k, B, Hkv, D)
              && token_ok(v, B, Hkv, D) && k.device() == q.device()
              && v.device() == q.device() && strides_aligned(q, 1, 4)
              && strides_aligned(k, 1, 4) && strides_aligned(v, 1, 4),
              "decode_rope_append_fp8: q [B,1,Hq,D], k/v [B,1,Hkv,D] must be "
              "device bf16 with contiguous heads and 8-byte aligned rows");
  TORCH_CHECK(fp8_cache_ok(k_codes, k_scale, q, 4)
              && fp8_cache_ok(v_codes, v_scale, q, 4)
              && k_codes.sizes() == v_codes.sizes() && k_codes.size(0) == B
              && k_codes.size(2) == Hkv && k_codes.size(3) == D,
              "decode_rope_append_fp8: the caches must be device "
              "float8_e4m3fn [B,Lmax,Hkv,D] of one shape (unit stride in D, "
              "4-byte aligned strides) with fp32 scales [B,Lmax,Hkv]");
  TORCH_CHECK(index_ok(pos, q, B), "decode_rope_append_fp8: pos must be a "
              "contiguous device int32 [B]");
  TORCH_CHECK(cos_t.has_value() == sin_t.has_value(),
              "decode_rope_append_fp8: give both RoPE tables or neither");
  const float* cp = nullptr;
  const float* sp = nullptr;
  if (cos_t.has_value()) {
    TORCH_CHECK(table_ok(*cos_t, Lmax, D) && table_ok(*sin_t, Lmax, D)
                && cos_t->device() == q.device()
                && sin_t->device() == q.device()
                && Lmax * (D / 2) < (1L << 31),
                "decode_rope_append_fp8: cos/sin must be contiguous device "
                "fp32 [>=Lmax, D/2]");
    cp = cos_t->data_ptr<float>();
    sp = sin_t->data_ptr<float>();
  }
  TORCH_CHECK(B <= 65535 && Hq + 2 * Hkv < (1L << 24),
              "decode_rope_append_fp8: batch or head count too large");
  auto q_out = torch::empty({B, 1, Hq, D}, q.options());
  if (B == 0) return q_out;
  auto stream = at::cuda::getCurrentHIPStream();
  const int LQ = D == 64 ? 8 : 16;
  const long rpb = DEC_THREADS / LQ;
  const dim3 grid((unsigned)((Hq + 2 * Hkv + rpb - 1) / rpb), (unsigned)B);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(DEC_THREADS), 0, stream,
                       (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                       (const unsigned short*)k.data_ptr(), (long)k.stride(0),
                       (const unsigned short*)v.data_ptr(), (long)v.stride(0),
                       cp, sp, pos.data_ptr<int>(),
                       (unsigned short*)q_out.data_ptr(),
                       fp8_cache(k_codes, k_scale),
                       fp8_cache(v_codes, v_scale), (int)Hq, (int)Hkv, (int)D,
                       (int)Lmax);
  };
  if (LQ == 8) launch(decode_rope_append_fp8_kernel<8>);
  else launch(decode_rope_append_fp8_kernel<16>);
  HIP_CHECK_KERNEL();
  return q_out;
}

std::vector<torch::Tensor> decode_attn_fp8_fwd(torch::Tensor q,
                                               torch::Tensor k_codes,
                                               torch::Tensor k_scale,
                                               torch::Tensor v_codes,
                                               torch::Tensor v_scale,
                                               torch::Tensor kv_lens,
                                               long kv_chunk) {
  TORCH_CHECK(q.dim() == 4 && k_codes.dim() == 4,
              "decode_attn_fp8: q must be [B,1,Hq,D], caches [B,Lmax,Hkv,D]");
  const long B = q.size(0), Hq = q.size(2), D = q.size(3);
  const long Lmax = k_codes.size(1), Hkv = k_codes.size(2);
  TORCH_CHECK(fp8_head_dim_ok(D),
              "decode_attn_fp8: head_dim must be 64, 80 or 128, got ", D);
  TORCH_CHECK(token_ok(q, B, Hq, D) && strides_aligned(q, 1, 8),
              "decode_attn_fp8: q must be device bf16 [B,1,Hq,D] with "
              "contiguous heads and a 16-byte aligned row stride");
  TORCH_CHECK(fp8_cache_ok(k_codes, k_scale, q, 16)
              && fp8_cache_ok(v_codes, v_scale, q, 16)
              && k_codes.sizes() == v_codes.sizes() && k_codes.size(0) == B
              && k_codes.size(3) == D,
              "decode_attn_fp8: the caches must be device float8_e4m3fn "
              "[B,Lmax,Hkv,D] of one shape (unit stride in D, 16-byte "
              "aligned batch/row/head strides) with fp32 scales "
              "[B,Lmax,Hkv]");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0,
              "decode_attn_fp8: Hq must be a multiple of Hkv");
  TORCH_CHECK(index_ok(kv_lens, q, B),
              "decode_attn_fp8: kv_lens must be a contiguous device int32 "
              "[B]");
  TORCH_CHECK(kv_chunk == 0 || (kv_chunk >= DEC_KV_CHUNK_MIN
                                && kv_chunk % DEC_KV_CHUNK_MIN == 0),
              "decode_attn_fp8: kv_chunk must be 0 (default ", DEC_KV_CHUNK,
              ") or a multiple of ", DEC_KV_CHUNK_MIN,
              "; the smallest legal value is ", DEC_KV_CHUNK_MIN);
  const long chunk = kv_chunk == 0 ? DEC_KV_CHUNK : kv_chunk;
  const long NC = std::max<long>(1, (Lmax + chunk - 1) / chunk);
  const long rep = Hq / Hkv;
  const long ngroups = (rep + DEC8_MAX_R - 1) / DEC8_MAX_R;
  TORCH_CHECK(B <= 65535 && Hkv * ngroups <= 65535 && Hq <= 65535
              && Lmax < (1L << 30),
              "decode_attn_fp8: batch, head count or cache length too large");

  auto o = torch::empty({B, 1, Hq, D}, q.options());
  auto lse = torch::empty({B, Hq, 1}, q.options().dtype(torch::kFloat32));
  if (B == 0 || Hq == 0) return {o, lse};
  auto ws_ml = torch::empty({B, Hq, NC, 2}, lse.options());
  auto ws_acc = torch::empty({B, Hq, NC, D}, lse.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const Fp8Cache kc = fp8_cache(k_codes, k_scale);
  const Fp8Cache vc = fp8_cache(v_codes, v_scale);
  if (D == 64)
    launch_fp8_decode<64>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                          (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else if (D == 80)
    launch_fp8_decode<80>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                          (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else
    launch_fp8_decode<128>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                           (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  return {o, lse};
}
