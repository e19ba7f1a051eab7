// K1 decode: split-KV single-token attention over a preallocated KV cache,
// plus the fused RoPE + cache-append step that feeds it. Inference only.
//
// decode_attn_fwd(q [B,1,Hq,D], k_cache/v_cache [B,Lmax,Hkv,D], kv_lens [B])
// Row b attends to cache rows 0 .. kv_lens[b]-1 (clamped to [0, Lmax]). The
// lengths live on the device, so a captured graph replays the same launch
// for every token. Two launches, no hand-off between workgroups inside one:
//
//  partial  grid (NC, Hkv * ngroups, B), 256 threads. One workgroup owns one
//           (batch row, kv head, kv chunk) and R <= 8 query heads of the GQA
//           group (ngroups = ceil(rep / R) when rep > 8), so K and V are read
//           once per kv head. A cache row of D bf16 is D/8 16-byte pieces;
//           TPR = 8 (D = 64) or 16 (D = 80: 10 of them load; D = 128) adjacent
//           lanes hold one row, so the workgroup has SLOTS = 256 / TPR row
//           slots (32 or 16). Key j of the chunk belongs to slot
//           (j - chunk_start) % SLOTS. A slot walks its keys UNROLL = 4 at a
//           time (all eight 16-byte loads in flight before the math), then
//           one at a time for the tail: the code paths change at chunk
//           offsets that are multiples of SLOTS and of UNROLL * SLOTS
//           (16/64 for D = 80, 128; 32/128 for D = 64).
//           Scores are VALU dot products reduced over the TPR lanes; each slot
//           keeps an fp32 online softmax (m, l, acc) per query head in the
//           exp2 domain. Slots merge by wave shuffles, the 4 waves through
//           LDS, and the workgroup writes the unnormalised partial
//           (m, l, acc[D]) per query head.
//           A load is issued only for j < min(len, chunk_end): rows at or
//           beyond the length are never read (they may hold anything). A chunk
//           wholly beyond the length writes the neutral partial (-inf, 0, 0).
//  combine  grid (Hq, B), 128 threads: merges the ceil(len / chunk) partials
//           of a row with exp2(m_s - m) weights, writes o (bf16) and lse
//           (fp32, natural log). Length 0 gives o = 0, lse = -inf.
//
// The chunk length is the compile-time DEC_KV_CHUNK (or the kv_chunk
// override), never a function of Lmax, B or other rows, and nothing is
// accumulated with atomics: a row's result is bit-identical whatever cache
// it sits in and whatever shares its batch.
//
// decode_rope_append: one launch rotates the new token's q and k at table
// row pos[b] (rotate-half, the table layout of elementwise.hip), returns the
// rotated q and stores k and v to cache[b, pos[b]]. Null tables = plain
// append. Rows with pos[b] outside [0, Lmax) write nothing to the cache.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_WAVES = DEC_THREADS / WAVE_SIZE;
constexpr int DEC_UNROLL = 4;
constexpr int DEC_KV_CHUNK = 256;      // default keys per workgroup
constexpr int DEC_KV_CHUNK_MIN = 16;   // smallest override (and its multiple)
constexpr int DEC_MAX_R = 8;           // query heads resident per workgroup

__device__ __forceinline__ float dec_weight(float m, float m_new) {
  // exp2(m - m_new) with the empty state (m = -inf) weighing nothing, also
  // when m_new is -inf as well
  return m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - m_new);
}

template <int D, int R>
__global__ __launch_bounds__(DEC_THREADS)
void decode_partial_kernel(const unsigned short* __restrict__ q, long q_sb,
                           const unsigned short* __restrict__ kc, long k_sb,
                           long k_sr, long k_sh,
                           const unsigned short* __restrict__ vc, long v_sb,
                           long v_sr, long v_sh,
                           const int* __restrict__ kv_lens,
                           float* __restrict__ ws_ml,
                           float* __restrict__ ws_acc,
                           int Lmax, int Hq, int rep, int ngroups, int chunk,
                           int NC, float scale2) {
  constexpr int TPR = (D == 64) ? 8 : 16;
  constexpr int PIECES = D / 8;
  constexpr int SLOTS = DEC_THREADS / TPR;
  __shared__ float sm_ml[DEC_WAVES][R][2];
  __shared__ float sm_acc[DEC_WAVES][R][D];

  const int c = blockIdx.x;
  const int hk = blockIdx.y / ngroups;
  const int r0 = (blockIdx.y % ngroups) * R;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int piece = lane % TPR;
  const int slot = tid / TPR;
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
  float qf[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[r][i] = 0.f;
    if (active && r < nr) {
      const shortx8 qq = *reinterpret_cast<const shortx8*>(
          q + (long)b * q_sb + (long)(hq0 + r) * D + piece * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        qf[r][i] = bf16_to_f32((unsigned short)qq[i]) * scale2;
    }
  }

  float m[R], l[R], acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[r][i] = 0.f;
  }

  const unsigned short* kb = kc + (long)b * k_sb + (long)hk * k_sh + piece * 8;
  const unsigned short* vb = vc + (long)b * v_sb + (long)hk * v_sh + piece * 8;
  const shortx8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  int j = start + slot;
  // UNROLL keys of this slot per trip; every j + u * SLOTS < end <= len
  for (; j + (DEC_UNROLL - 1) * SLOTS < end; j += DEC_UNROLL * SLOTS) {
    shortx8 kk[DEC_UNROLL], vv[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      kk[u] = zero8;
      vv[u] = zero8;
      if (active) {
        kk[u] = *reinterpret_cast<const shortx8*>(
            kb + (long)(j + u * SLOTS) * k_sr);
        vv[u] = *reinterpret_cast<const shortx8*>(
            vb + (long)(j + u * SLOTS) * v_sr);
      }
    }
    float s[DEC_UNROLL][R];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float kf[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) kf[i] = bf16_to_f32((unsigned short)kk[u][i]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float d0 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d0 = fmaf(qf[r][i], kf[i], d0);
        s[u][r] = d0;
      }
    }
#pragma unroll
    for (int off = TPR / 2; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
          s[u][r] += __shfl_xor(s[u][r], off, WAVE_SIZE);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mn = m[r];
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u) mn = fmaxf(mn, s[u][r]);
      const float alpha = __builtin_amdgcn_exp2f(m[r] - mn);
      m[r] = mn;
      l[r] *= alpha;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r][i] *= alpha;
#pragma unroll
      for (int u = 0; u < DEC_UNROLL; ++u) {
        const float p = __builtin_amdgcn_exp2f(s[u][r] - mn);
        l[r] += p;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          acc[r][i] = fmaf(p, bf16_to_f32((unsigned short)vv[u][i]), acc[r][i]);
      }
    }
  }
  // tail: one key per trip
  for (; j < end; j += SLOTS) {
    shortx8 kk = zero8, vv = zero8;
    if (active) {
      kk = *reinterpret_cast<const shortx8*>(kb + (long)j * k_sr);
      vv = *reinterpret_cast<const shortx8*>(vb + (long)j * v_sr);
    }
    float kf[8], s[R];
#pragma unroll
    for (int i = 0; i < 8; ++i) kf[i] = bf16_to_f32((unsigned short)kk[i]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float d0 = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) d0 = fmaf(qf[r][i], kf[i], d0);
      s[r] = d0;
    }
#pragma unroll
    for (int off = TPR / 2; off > 0; off >>= 1)
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] += __shfl_xor(s[r], off, WAVE_SIZE);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float mn = fmaxf(m[r], s[r]);
      const float alpha = __builtin_amdgcn_exp2f(m[r] - mn);
      const float p = __builtin_amdgcn_exp2f(s[r] - mn);
      m[r] = mn;
      l[r] = fmaf(l[r], alpha, p);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        acc[r][i] = fmaf(p, bf16_to_f32((unsigned short)vv[i]),
                         acc[r][i] * alpha);
    }
  }

  // merge the slots of a wave (lane bits TPR .. 32); slot 0 of the wave ends
  // up with the wave's state
#pragma unroll
  for (int off = TPR; off < WAVE_SIZE; off <<= 1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float mo = __shfl_xor(m[r], off, WAVE_SIZE);
      const float mn = fmaxf(m[r], mo);
      const float ws = dec_weight(m[r], mn);
      const float wo = dec_weight(mo, mn);
      l[r] = l[r] * ws + __shfl_xor(l[r], off, WAVE_SIZE) * wo;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        acc[r][i] = acc[r][i] * ws
            + __shfl_xor(acc[r][i], off, WAVE_SIZE) * wo;
      m[r] = mn;
    }
  }
  if (lane < TPR && active) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (piece == 0) {
        sm_ml[wave][r][0] = m[r];
        sm_ml[wave][r][1] = l[r];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_acc[wave][r][piece * 8 + i] = acc[r][i];
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

// One thread = 4 elements: a rotate-half (lo, hi) pair of pairs of q or k, as
// rope_kernel in elementwise.hip, or 4 adjacent elements of v.
__global__ void decode_rope_append_kernel(
    const unsigned short* __restrict__ q, long q_sb,
    const unsigned short* __restrict__ k, long k_sb,
    const unsigned short* __restrict__ v, long v_sb,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int* __restrict__ pos, unsigned short* __restrict__ q_out,
    unsigned short* __restrict__ kc, long kc_sb, long kc_sr, long kc_sh,
    unsigned short* __restrict__ vc, long vc_sb, long vc_sr, long vc_sh,
    int Hq, int Hkv, int D, int Lmax) {
  const int halfD = D / 2;
  const int pairs2 = D / 4;
  const int nq = Hq * pairs2, nk = Hkv * pairs2;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nq + 2 * nk) return;
  const int b = blockIdx.y;
  const int t = pos[b];
  const bool ok = t >= 0 && t < Lmax;
  if (w < nq + nk) {
    const bool is_q = w < nq;
    const int ww = is_q ? w : w - nq;
    const int h = ww / pairs2;
    const int j2 = (ww % pairs2) * 2;
    unsigned short* dst = is_q
        ? q_out + ((long)b * Hq + h) * D
        : kc + (long)b * kc_sb + (long)t * kc_sr + (long)h * kc_sh;
    if (!ok) {   // no table row, no cache row: q is defined as zero
      if (is_q) {
        *reinterpret_cast<unsigned int*>(dst + j2) = 0u;
        *reinterpret_cast<unsigned int*>(dst + halfD + j2) = 0u;
      }
      return;
    }
    const unsigned short* src = is_q ? q + (long)b * q_sb + (long)h * D
                                     : k + (long)b * k_sb + (long)h * D;
    const unsigned int lo_u = *reinterpret_cast<const unsigned int*>(src + j2);
    const unsigned int hi_u =
        *reinterpret_cast<const unsigned int*>(src + halfD + j2);
    if (cos_t == nullptr) {
      *reinterpret_cast<unsigned int*>(dst + j2) = lo_u;
      *reinterpret_cast<unsigned int*>(dst + halfD + j2) = hi_u;
      return;
    }
    const float lo0 = bf16_to_f32((unsigned short)(lo_u & 0xffff));
    const float lo1 = bf16_to_f32((unsigned short)(lo_u >> 16));
    const float hi0 = bf16_to_f32((unsigned short)(hi_u & 0xffff));
    const float hi1 = bf16_to_f32((unsigned short)(hi_u >> 16));
    const float c0 = cos_t[t * halfD + j2], c1 = cos_t[t * halfD + j2 + 1];
    const float s0 = sin_t[t * halfD + j2], s1 = sin_t[t * halfD + j2 + 1];
    const float o_lo0 = lo0 * c0 - hi0 * s0;
    const float o_lo1 = lo1 * c1 - hi1 * s1;
    const float o_hi0 = hi0 * c0 + lo0 * s0;
    const float o_hi1 = hi1 * c1 + lo1 * s1;
    *reinterpret_cast<unsigned int*>(dst + j2) =
        (unsigned int)f32_to_bf16(o_lo0)
        | ((unsigned int)f32_to_bf16(o_lo1) << 16);
    *reinterpret_cast<unsigned int*>(dst + halfD + j2) =
        (unsigned int)f32_to_bf16(o_hi0)
        | ((unsigned int)f32_to_bf16(o_hi1) << 16);
  } else {
    if (!ok) return;
    const int ww = w - nq - nk;
    const int h = ww / pairs2;
    const int e = (ww % pairs2) * 4;
    const unsigned short* src = v + (long)b * v_sb + (long)h * D + e;
    unsigned short* dst =
        vc + (long)b * vc_sb + (long)t * vc_sr + (long)h * vc_sh + e;
    *reinterpret_cast<unsigned int*>(dst) =
        *reinterpret_cast<const unsigned int*>(src);
    *reinterpret_cast<unsigned int*>(dst + 2) =
        *reinterpret_cast<const unsigned int*>(src + 2);
  }
}

// x: bf16 [B, 1, H, D] whose heads are contiguous; rows may be strided
// (a view into a fused-QKV projection output)
bool token_ok(const torch::Tensor& x, long B, long H, long D) {
  return x.is_cuda() && x.dtype() == torch::kBFloat16 && x.dim() == 4
      && x.size(0) == B && x.size(1) == 1 && x.size(2) == H && x.size(3) == D
      && x.stride(3) == 1 && (H == 1 || x.stride(2) == D);
}

// every element offset a multiple of `elems`, base aligned accordingly
bool strides_aligned(const torch::Tensor& x, int ndims, long elems) {
  if (reinterpret_cast<uintptr_t>(x.data_ptr()) % (2 * elems) != 0)
    return false;
  for (int i = 0; i < ndims; ++i)
    if (x.size(i) > 1 && x.stride(i) % elems != 0) return false;
  return true;
}

bool cache_ok(const torch::Tensor& c, const torch::Tensor& ref) {
  return c.is_cuda() && c.dtype() == torch::kBFloat16 && c.dim() == 4
      && c.device() == ref.device() && c.stride(3) == 1;
}

// t is a contiguous device fp32 [>= T, D/2] cos or sin table
bool table_ok(const torch::Tensor& t, long T, long D) {
  return t.is_cuda() && t.dtype() == torch::kFloat32 && t.dim() == 2
      && t.is_contiguous() && t.size(0) >= T && t.size(1) == D / 2;
}

bool index_ok(const torch::Tensor& t, const torch::Tensor& ref, long B) {
  return t.is_cuda() && t.device() == ref.device()
      && t.dtype() == torch::kInt32 && t.dim() == 1 && t.size(0) == B
      && t.is_contiguous();
}

template <int D, int R>
void launch_partial(const torch::Tensor& q, const torch::Tensor& kc,
                    const torch::Tensor& vc, const torch::Tensor& kv_lens,
                    torch::Tensor& ws_ml, torch::Tensor& ws_acc, int rep,
                    int chunk, int NC, hipStream_t stream) {
  const int B = q.size(0), Hq = q.size(2), Hkv = kc.size(2);
  const int Lmax = kc.size(1);
  const int ngroups = (rep + R - 1) / R;
  const float scale2 = 1.44269504f / sqrtf((float)D);
  hipLaunchKernelGGL((decode_partial_kernel<D, R>),
                     dim3(NC, Hkv * ngroups, B), dim3(DEC_THREADS), 0, stream,
                     (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                     (const unsigned short*)kc.data_ptr(), (long)kc.stride(0),
                     (long)kc.stride(1), (long)kc.stride(2),
                     (const unsigned short*)vc.data_ptr(), (long)vc.stride(0),
                     (long)vc.stride(1), (long)vc.stride(2),
                     kv_lens.data_ptr<int>(), ws_ml.data_ptr<float>(),
                     ws_acc.data_ptr<float>(), Lmax, Hq, rep, ngroups, chunk,
                     NC, scale2);
}

template <int D>
void launch_decode(const torch::Tensor& q, const torch::Tensor& kc,
                   const torch::Tensor& vc, const torch::Tensor& kv_lens,
                   torch::Tensor& ws_ml, torch::Tensor& ws_acc,
                   torch::Tensor& o, torch::Tensor& lse, int chunk, int NC,
                   hipStream_t stream) {
  const int B = q.size(0), Hq = q.size(2), Hkv = kc.size(2);
  const int rep = Hq / Hkv;
  if (rep == 1)
    launch_partial<D, 1>(q, kc, vc, kv_lens, ws_ml, ws_acc, rep, chunk, NC,
                         stream);
  else if (rep == 2)
    launch_partial<D, 2>(q, kc, vc, kv_lens, ws_ml, ws_acc, rep, chunk, NC,
                         stream);
  else if (rep <= 4)
    launch_partial<D, 4>(q, kc, vc, kv_lens, ws_ml, ws_acc, rep, chunk, NC,
                         stream);
  else
    launch_partial<D, DEC_MAX_R>(q, kc, vc, kv_lens, ws_ml, ws_acc, rep,
                                 chunk, NC, stream);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL((decode_combine_kernel<D>), dim3(Hq, B), dim3(128), 0,
                     stream, ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(),
                     kv_lens.data_ptr<int>(), (unsigned short*)o.data_ptr(),
                     lse.data_ptr<float>(), (int)kc.size(1), Hq, chunk, NC);
  HIP_CHECK_KERNEL();
}

}  // namespace

long decode_attn_kv_chunk() { return DEC_KV_CHUNK; }
long decode_attn_kv_chunk_min() { return DEC_KV_CHUNK_MIN; }

std::vector<torch::Tensor> decode_attn_fwd(torch::Tensor q,
                                           torch::Tensor k_cache,
                                           torch::Tensor v_cache,
                                           torch::Tensor kv_lens,
                                           long kv_chunk) {
  TORCH_CHECK(q.dim() == 4 && k_cache.dim() == 4,
              "decode_attn: q must be [B,1,Hq,D], caches [B,Lmax,Hkv,D]");
  const long B = q.size(0), Hq = q.size(2), D = q.size(3);
  const long Lmax = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(D == 64 || D == 80 || D == 128,
              "decode_attn: head_dim must be 64, 80 or 128, got ", D);
  TORCH_CHECK(token_ok(q, B, Hq, D) && strides_aligned(q, 1, 8),
              "decode_attn: q must be device bf16 [B,1,Hq,D] with contiguous "
              "heads and a 16-byte aligned row stride");
  TORCH_CHECK(cache_ok(k_cache, q) && cache_ok(v_cache, q)
              && k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B
              && k_cache.size(3) == D && strides_aligned(k_cache, 3, 8)
              && strides_aligned(v_cache, 3, 8),
              "decode_attn: k_cache/v_cache must be device bf16 "
              "[B,Lmax,Hkv,D] of one shape, unit stride in D and 16-byte "
              "aligned batch/row/head strides");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0,
              "decode_attn: Hq must be a multiple of Hkv");
  TORCH_CHECK(index_ok(kv_lens, q, B),
              "decode_attn: kv_lens must be a contiguous device int32 [B]");
  TORCH_CHECK(kv_chunk == 0 || (kv_chunk >= DEC_KV_CHUNK_MIN
                                && kv_chunk % DEC_KV_CHUNK_MIN == 0),
              "decode_attn: kv_chunk must be 0 (default ", DEC_KV_CHUNK,
              ") or a multiple of ", DEC_KV_CHUNK_MIN,
              "; the smallest legal value is ", DEC_KV_CHUNK_MIN);
  const long chunk = kv_chunk == 0 ? DEC_KV_CHUNK : kv_chunk;
  const long NC = std::max<long>(1, (Lmax + chunk - 1) / chunk);
  const long rep = Hq / Hkv;
  const long ngroups = (rep + DEC_MAX_R - 1) / DEC_MAX_R;
  TORCH_CHECK(B <= 65535 && Hkv * ngroups <= 65535 && Hq <= 65535
              && Lmax < (1L << 30),
              "decode_attn: batch, head count or cache length too large");

  auto o = torch::empty({B, 1, Hq, D}, q.options());
  auto lse = torch::empty({B, Hq, 1}, q.options().dtype(torch::kFloat32));
  if (B == 0 || Hq == 0) return {o, lse};
  auto ws_ml = torch::empty({B, Hq, NC, 2}, lse.options());
  auto ws_acc = torch::empty({B, Hq, NC, D}, lse.options());
  auto stream = at::cuda::getCurrentHIPStream();
  if (D == 64)
    launch_decode<64>(q, k_cache, v_cache, kv_lens, ws_ml, ws_acc, o, lse,
                      (int)chunk, (int)NC, stream);
  else if (D == 80)
    launch_decode<80>(q, k_cache, v_cache, kv_lens, ws_ml, ws_acc, o, lse,
                      (int)chunk, (int)NC, stream);
  else
    launch_decode<128>(q, k_cache, v_cache, kv_lens, ws_ml, ws_acc, o, lse,
                       (int)chunk, (int)NC, stream);
  return {o, lse};
}

torch::Tensor decode_rope_append(torch::Tensor q, torch::Tensor k,
                                 torch::Tensor v,
                                 c10::optional<torch::Tensor> cos_t,
                                 c10::optional<torch::Tensor> sin_t,
                                 torch::Tensor pos, torch::Tensor k_cache,
                                 torch::Tensor v_cache) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && k_cache.dim() == 4,
              "decode_rope_append: q/k/v must be [B,1,H,D], caches "
              "[B,Lmax,Hkv,D]");
  const long B = q.size(0), Hq = q.size(2), D = q.size(3), Hkv = k.size(2);
  const long Lmax = k_cache.size(1);
  TORCH_CHECK(D % 4 == 0, "decode_rope_append: head_dim must be divisible "
              "by 4");
  TORCH_CHECK(token_ok(q, B, Hq, D) && token_ok(k, B, Hkv, D)
              && token_ok(v, B, Hkv, D) && k.device() == q.device()
              && v.device() == q.device() && strides_aligned(q, 1, 2)
              && strides_aligned(k, 1, 2) && strides_aligned(v, 1, 2),
              "decode_rope_append: q [B,1,Hq,D], k/v [B,1,Hkv,D] must be "
              "device bf16 with contiguous heads and 4-byte aligned rows");
  TORCH_CHECK(cache_ok(k_cache, q) && cache_ok(v_cache, q)
              && k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B
              && k_cache.size(2) == Hkv && k_cache.size(3) == D
              && strides_aligned(k_cache, 3, 2)
              && strides_aligned(v_cache, 3, 2),
              "decode_rope_append: caches must be device bf16 "
              "[B,Lmax,Hkv,D] of one shape with unit stride in D");
  TORCH_CHECK(index_ok(pos, q, B),
              "decode_rope_append: pos must be a contiguous device int32 [B]");
  TORCH_CHECK(cos_t.has_value() == sin_t.has_value(),
              "decode_rope_append: give both RoPE tables or neither");
  const float* cp = nullptr;
  const float* sp = nullptr;
  if (cos_t.has_value()) {
    TORCH_CHECK(table_ok(*cos_t, Lmax, D) && table_ok(*sin_t, Lmax, D)
                && cos_t->device() == q.device()
                && sin_t->device() == q.device()
                && Lmax * (D / 2) < (1L << 31),
                "decode_rope_append: cos/sin must be contiguous device fp32 "
                "[>=Lmax, D/2]");
    cp = cos_t->data_ptr<float>();
    sp = sin_t->data_ptr<float>();
  }
  TORCH_CHECK(B <= 65535, "decode_rope_append: batch too large");
  auto q_out = torch::empty({B, 1, Hq, D}, q.options());
  if (B == 0) return q_out;
  const long work = (Hq + 2 * Hkv) * (D / 4);
  auto stream = at::cuda::getCurrentHIPStream();
  hipLaunchKernelGGL(decode_rope_append_kernel,
                     dim3((work + 255) / 256, B), dim3(256), 0, stream,
                     (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                     (const unsigned short*)k.data_ptr(), (long)k.stride(0),
                     (const unsigned short*)v.data_ptr(), (long)v.stride(0),
                     cp, sp, pos.data_ptr<int>(),
                     (unsigned short*)q_out.data_ptr(),
                     (unsigned short*)k_cache.data_ptr(),
                     (long)k_cache.stride(0), (long)k_cache.stride(1),
                     (long)k_cache.stride(2),
                     (unsigned short*)v_cache.data_ptr(),
                     (long)v_cache.stride(0), (long)v_cache.stride(1),
                     (long)v_cache.stride(2), (int)Hq, (int)Hkv, (int)D,
                     (int)Lmax);
  HIP_CHECK_KERNEL();
  return q_out;
}
