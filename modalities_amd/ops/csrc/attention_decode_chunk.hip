// K1 decode, multi-token: split-KV attention of T >= 2 new tokens per batch
// row over a preallocated KV cache (bf16, or e4m3 codes with per-row scales),
// on the matrix cores. Inference only.
//
// decode_attn_chunk_fwd(q [B,T,Hq,D], k_cache/v_cache [B,Lmax,Hkv,D],
//                       kv_lens [B]) -> (o [B,T,Hq,D] bf16, lse [B,Hq,T] fp32)
// decode_attn_chunk_fp8_fwd: the same over code caches and fp32 scales
//                       [B,Lmax,Hkv] (the format of attention_decode_fp8.hip).
// kv_lens[b] (clamped to [0, Lmax]) counts the valid cache rows of batch row
// b including the T new ones; query t sees the rows j < kv_lens[b] - (T-1-t).
// A query that sees no row gives o = 0, lse = -inf. The lengths live on the
// device. Two launches, no hand-off between workgroups inside one:
//
//  partial  grid (NC, Hkv * ntiles, B), 256 threads. The T * rep query rows
//           of a kv head (row = t * rep + head-in-group) are cut into tiles
//           of 16; one workgroup owns one (batch row, kv head, row tile, kv
//           chunk), so K and V are read from HBM once per 16 query rows. Its
//           4 waves take the chunk's 32-key steps interleaved (wave w: steps
//           w, w + 4, ...) into private (m, l, acc) state.
//           Scores: S^T = K . Q^T with v_mfma_f32_16x16x32_bf16, two 16-key
//           tiles per step. K is the A operand: lane (key = lane % 16, g =
//           lane / 16) loads the 8 elements d = 32 s + 8 g of its key for
//           MFMA step s straight from HBM to VGPRs (D = 80: the third step
//           is zero-padded, only g < 2 load). Q^T is the B operand (lane =
//           (query, g), the same d), loaded once and kept in registers. All
//           K and V loads of a step (8 / 11 / 16 per lane for D = 64 / 80 /
//           128) are issued before the first is used, and the loads of the
//           wave's next step are issued right after the score MFMAs of the
//           current one, before its softmax and P.V.
//           Softmax: in the 16x16 result lane (query, g) holds keys 4 g + i
//           of each tile; fp32 online softmax in the exp2 domain, the max
//           reduced over the lane's 8 values and then over the 4 lane groups
//           by two xor shuffles; l stays a per-lane partial sum until the end.
//           Steps whose keys all lie below kv_lens[b] - T + 1 are visible to
//           every query and skip the per-column bound.
//           P.V: O^T += V^T . P^T with the same MFMA. P^T, rounded to bf16,
//           is the B operand as it stands: k-slot e of lane group g is key
//           4 g + e of the first tile (e < 4) or 4 g + e - 4 of the second.
//           V^T is the A operand under the same key permutation; V is the
//           one operand that goes through LDS: a wave writes its 32 V rows
//           row-major into an image of its own (pitch D + 8 elements) and
//           reads them back transposed with ds_read_b64_tr_b16. The image is
//           private to the wave and LDS operations of a wave complete in
//           order, so the loop has no barrier.
//           The waves merge through LDS in wave order and the workgroup
//           writes one unnormalised fp32 partial (m, l, acc[D]) per query.
//           Nothing at or beyond min(len, chunk end) is loaded, neither
//           rows, codes nor scales; such keys enter as zeros and are masked.
//  combine  grid (T * Hq, B), 128 threads: decode_combine_kernel's merge
//           with the length taken per query, lse stored as [B, Hq, T], and a
//           query without keys defined as o = 0, lse = -inf (the shared
//           kernel knows one length per batch row, hence the variant here).
//
// FP8: codes are widened to bf16 in registers (v_cvt_pk_f32_fp8 + v_perm_b32,
// exact). The K scale multiplies the fp32 score of its key, the V scale is
// folded into p before p is rounded (powers of two: exact); l sums the
// unscaled p. Deviation from 16-byte loads: a lane's operand piece is 8
// elements in both formats, so the FP8 kernel issues 8-byte loads; the four
// lane groups of a key still cover 32 contiguous bytes per step.
//
// The chunk length is DCH_KV_CHUNK or the kv_chunk override (a multiple of
// the 32 keys of a wave step), never a function of Lmax, B or other rows,
// and nothing is accumulated with atomics: a query's result is bit-identical
// whatever cache it sits in and whatever shares its batch.
#include <type_traits>

#include "attention_decode_common.h"
#include "attn_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

constexpr int DCH_KV_CHUNK = 256;     // default keys per workgroup
constexpr int DCH_WAVE_KEYS = 32;     // keys a wave consumes per step
constexpr int DCH_KV_CHUNK_MIN = DCH_WAVE_KEYS;   // smallest override
constexpr int DCH_ROWS = 16;          // query rows per workgroup

// a cache with strides in elements; scale is null for bf16
struct ChunkCache {
  const unsigned char* data;
  long sb, sr, sh;
  const float* scale;
  long s_sb, s_sr, s_sh;
};

__device__ __forceinline__ unsigned int pack_high_halves(float lo, float hi) {
  // {lo.b2, lo.b3, hi.b2, hi.b3}: the bf16 of two fp32 with zero low halves
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo),
                               0x07060302u);
}

// 8 elements of a cache row as they come from memory, and as an MFMA fragment
template <bool FP8> struct Piece {
  using Raw = std::conditional_t<FP8, uintx2, uintx4>;
  static __device__ __forceinline__ Raw zero() {
    if constexpr (FP8) return uintx2{0u, 0u};
    else return uintx4{0u, 0u, 0u, 0u};
  }
  // p: the row's first byte, d: element offset (a multiple of 8)
  static __device__ __forceinline__ Raw load(const unsigned char* p, int d) {
    if constexpr (FP8) return *reinterpret_cast<const uintx2*>(p + d);
    else return *reinterpret_cast<const uintx4*>(p + 2 * d);
  }
  static __device__ __forceinline__ uintx4 widen(const Raw& r) {
    if constexpr (FP8) {
      const floatx2 a = __builtin_amdgcn_cvt_pk_f32_fp8(r.x, false);
      const floatx2 b = __builtin_amdgcn_cvt_pk_f32_fp8(r.x, true);
      const floatx2 c = __builtin_amdgcn_cvt_pk_f32_fp8(r.y, false);
      const floatx2 d = __builtin_amdgcn_cvt_pk_f32_fp8(r.y, true);
      return uintx4{pack_high_halves(a.x, a.y), pack_high_halves(b.x, b.y),
                    pack_high_halves(c.x, c.y), pack_high_halves(d.x, d.y)};
    } else {
      return r;
    }
  }
};

template <int D, bool FP8>
__global__ __launch_bounds__(DEC_THREADS)
void chunk_partial_kernel(const unsigned short* __restrict__ q, long q_sb,
                          long q_st, ChunkCache kc, ChunkCache vc,
                          const int* __restrict__ kv_lens,
                          float* __restrict__ ws_ml,
                          float* __restrict__ ws_acc,
                          int Lmax, int T, int Hq, int rep, int ntiles,
                          int chunk, int NC, float scale2) {
  using P = Piece<FP8>;
  using Raw = typename P::Raw;
  constexpr int ES = FP8 ? 1 : 2;            // bytes per cache element
  constexpr int NS = (D + 31) / 32;          // score MFMA steps per key tile
  constexpr int NDT = D / 16;                // 16-wide d tiles of O^T
  constexpr int PPR = D / 8;                 // 8-element pieces per row
  constexpr int NV = DCH_WAVE_KEYS * PPR / WAVE_SIZE;   // V pieces per lane
  constexpr int PITCH = D + 8;               // V image row pitch, elements
  constexpr int VIMG = DCH_WAVE_KEYS * PITCH * 2;       // bytes per wave
  constexpr int MRG = DEC_WAVES * DCH_ROWS * (D + 2) * 4;
  constexpr int SMEM = DEC_WAVES * VIMG > MRG ? DEC_WAVES * VIMG : MRG;
  static_assert(DCH_WAVE_KEYS * PPR % WAVE_SIZE == 0, "V staging split");
  // the V images while the waves walk their keys, the merge buffers after
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

  const int c = blockIdx.x;
  const int hk = blockIdx.y / ntiles;
  const int tile = blockIdx.y % ntiles;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int col = lane & 15;                 // key of A, query of B and C
  const int g = lane >> 4;
  const int R = T * rep;                     // query rows of this kv head

  int len = kv_lens[b];
  len = min(max(len, 0), Lmax);
  const int start = c * chunk;
  const int end = min(start + chunk, len);
  // the combine launch skips the chunks that hold no key of a query
  if (start >= len) return;

  // this lane's query (as B operand and in the result): row, bound, Q^T
  const int row = tile * DCH_ROWS + col;
  const bool row_ok = row < R;
  const int qt = row_ok ? row / rep : 0;
  const int qh = hk * rep + (row_ok ? row % rep : 0);
  const int bound = row_ok ? len - (T - 1 - qt) : 0;   // keys j < bound
  uintx4 qfrag[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    qfrag[s] = uintx4{0u, 0u, 0u, 0u};
    const int d = 32 * s + 8 * g;
    if (row_ok && d < D)
      qfrag[s] = *reinterpret_cast<const uintx4*>(
          q + (long)b * q_sb + (long)qt * q_st + (long)qh * D + d);
  }

  const unsigned char* kb = kc.data + ((long)b * kc.sb + (long)hk * kc.sh) * ES;
  const unsigned char* vb = vc.data + ((long)b * vc.sb + (long)hk * vc.sh) * ES;
  const float* ksb = nullptr;
  const float* vsb = nullptr;
  if constexpr (FP8) {
    ksb = kc.scale + (long)b * kc.s_sb + (long)hk * kc.s_sh;
    vsb = vc.scale + (long)b * vc.s_sb + (long)hk * vc.s_sh;
  }

  unsigned char* vimg = smem + wave * VIMG;
  // transposing read: lane group g, lane lam of it, rows 4 g + (lam >> 2)
  const unsigned trb = attnc::lds_addr(vimg)
      + (unsigned)(((4 * g + (col >> 2)) * PITCH + 4 * (col & 3)) * 2);

  float m = -INFINITY, l = 0.f;
  floatx4 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  Raw kreg[2][NS], vreg[NV];
  float ksc[2][4], vsc[2][4];
  // every load of the 32-key step at j0; keys at or beyond `end` load nothing
  auto issue = [&](int j0) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int j = j0 + tt * 16 + col;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int d = 32 * s + 8 * g;
        kreg[tt][s] = P::zero();
        if (j < end && d < D)
          kreg[tt][s] = P::load(kb + (long)j * kc.sr * ES, d);
      }
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int x = lane + n * WAVE_SIZE;
      const int j = j0 + x / PPR;
      vreg[n] = P::zero();
      if (j < end) vreg[n] = P::load(vb + (long)j * vc.sr * ES, (x % PPR) * 8);
    }
    if constexpr (FP8) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = j0 + tt * 16 + 4 * g + i;
          ksc[tt][i] = 0.f;
          vsc[tt][i] = 0.f;
          if (j < end) {
            ksc[tt][i] = ksb[(long)j * kc.s_sr];
            vsc[tt][i] = vsb[(long)j * vc.s_sr];
          }
        }
    }
  };

  int j0 = start + wave * DCH_WAVE_KEYS;
  if (j0 < end) issue(j0);
  for (; j0 < end; j0 += DEC_WAVES * DCH_WAVE_KEYS) {
    // ---- V rows into the wave's image ------------------------------------
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int x = lane + n * WAVE_SIZE;
      *reinterpret_cast<uintx4*>(vimg + ((x / PPR) * PITCH + (x % PPR) * 8) * 2)
          = P::widen(vreg[n]);
    }
    // ---- S^T = K Q^T -----------------------------------------------------
    floatx4 st[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      st[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s)
        st[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(bf16x8, P::widen(kreg[tt][s])),
            __builtin_bit_cast(bf16x8, qfrag[s]), st[tt], 0, 0, 0);
    }
    float sc[8], vs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = st[e >> 2][e & 3] * scale2;
      vs[e] = 1.f;
      if constexpr (FP8) {
        sc[e] *= ksc[e >> 2][e & 3];
        vs[e] = vsc[e >> 2][e & 3];
      }
    }
    const int jcur = j0;
    // ---- the next step's loads, before this step's softmax and P.V --------
    if (j0 + DEC_WAVES * DCH_WAVE_KEYS < end)
      issue(j0 + DEC_WAVES * DCH_WAVE_KEYS);

    // ---- online softmax; only the trailing steps apply the bound ----------
    if (jcur + DCH_WAVE_KEYS > len - T + 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = jcur + (e >> 2) * 16 + 4 * g + (e & 3);
        if (j >= bound) sc[e] = -INFINITY;
      }
    }
    float mx = sc[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, sc[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE_SIZE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE_SIZE));
    const float m_new = fmaxf(m, mx);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_safe);   // m = -inf: 0
    m = m_new;
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[dt][i] *= alpha;
    float p[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = __builtin_amdgcn_exp2f(sc[e] - m_safe);
      l += p[e];
      p[e] *= vs[e];
    }
    const uintx4 pw = {attnc::cvt_pk_bf16(p[0], p[1]),
                       attnc::cvt_pk_bf16(p[2], p[3]),
                       attnc::cvt_pk_bf16(p[4], p[5]),
                       attnc::cvt_pk_bf16(p[6], p[7])};
    const bf16x8 pfrag = __builtin_bit_cast(bf16x8, pw);

    // ---- O^T += V^T P^T: batched transposing reads, one drain -------------
    uintx2 rv[2 * NDT];
    asm volatile("" ::: "memory");   // the image stores stay above the reads
    attnc::static_for<NDT>([&](auto dt_) {
      constexpr int dt = decltype(dt_)::value;
      rv[2 * dt] = attnc::tr_read_b64_off<dt * 32>(trb);
      rv[2 * dt + 1] = attnc::tr_read_b64_off<dt * 32 + 16 * PITCH * 2>(trb);
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const uintx4 vw = {rv[2 * dt][0], rv[2 * dt][1], rv[2 * dt + 1][0],
                         rv[2 * dt + 1][1]};
      acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, vw), pfrag, acc[dt], 0, 0, 0);
    }
  }

  // ---- merge the waves in a fixed order and write the partial -------------
  l += __shfl_xor(l, 16, WAVE_SIZE);
  l += __shfl_xor(l, 32, WAVE_SIZE);
  __syncthreads();   // every wave is done with its V image
  float* sm_ml = reinterpret_cast<float*>(smem);            // [W][16][2]
  float* sm_acc = sm_ml + DEC_WAVES * DCH_ROWS * 2;         // [W][16][D]
  if (g == 0) {
    sm_ml[(wave * DCH_ROWS + col) * 2] = m;
    sm_ml[(wave * DCH_ROWS + col) * 2 + 1] = l;
  }
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
    *reinterpret_cast<floatx4*>(
        sm_acc + (wave * DCH_ROWS + col) * D + dt * 16 + 4 * g) = acc[dt];
  __syncthreads();

  const long HqT = (long)T * Hq;
  for (int i = tid; i < DCH_ROWS * D; i += DEC_THREADS) {
    const int r = i / D, d = i % D;
    const int rr = tile * DCH_ROWS + r;
    if (rr >= R) continue;
    float mw = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w)
      mw = fmaxf(mw, sm_ml[(w * DCH_ROWS + r) * 2]);
    float lw = 0.f, aw = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float wt = dec_weight(sm_ml[(w * DCH_ROWS + r) * 2], mw);
      lw += sm_ml[(w * DCH_ROWS + r) * 2 + 1] * wt;
      aw += sm_acc[(w * DCH_ROWS + r) * D + d] * wt;
    }
    // the partial of query (t, head) sits where decode_combine_kernel looks
    // for head t * Hq + head of T * Hq
    const long hp = (long)(rr / rep) * Hq + hk * rep + rr % rep;
    const long part = ((long)b * HqT + hp) * NC + c;
    ws_acc[part * D + d] = aw;
    if (d == 0) {
      ws_ml[part * 2] = mw;
      ws_ml[part * 2 + 1] = lw;
    }
  }
}

// decode_combine_kernel with one length per query: head index t * Hq + h.
template <int D>
__global__ __launch_bounds__(128)
void chunk_combine_kernel(const float* __restrict__ ws_ml,
                          const float* __restrict__ ws_acc,
                          const int* __restrict__ kv_lens,
                          unsigned short* __restrict__ o,
                          float* __restrict__ lse,
                          int Lmax, int T, int Hq, int chunk, int NC) {
  const int hp = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  const int t = hp / Hq, h = hp % Hq;
  int len = kv_lens[b];
  len = min(max(len, 0), Lmax);
  const int n = max(len - (T - 1 - t), 0);       // keys this query sees
  const int ncl = (n + chunk - 1) / chunk;       // chunks that hold them
  const long base = ((long)b * T * Hq + hp) * NC;
  float mx = -INFINITY;
  for (int s = 0; s < ncl; ++s) mx = fmaxf(mx, ws_ml[(base + s) * 2]);
  float lsum = 0.f, a = 0.f;
  for (int s = 0; s < ncl; ++s) {
    const float wt = dec_weight(ws_ml[(base + s) * 2], mx);
    lsum += ws_ml[(base + s) * 2 + 1] * wt;
    if (d < D) a += ws_acc[(base + s) * D + d] * wt;
  }
  if (d < D)
    o[((long)b * T * Hq + hp) * D + d] = f32_to_bf16(ncl > 0 ? a / lsum : 0.f);
  if (d == 0)
    lse[((long)b * Hq + h) * T + t] =
        ncl > 0 ? (mx + log2f(lsum)) * 0.69314718056f : -INFINITY;
}

// q: device bf16 [B, T, Hq, D], heads contiguous, token and batch strides
// free but 16-byte aligned
bool chunk_q_ok(const torch::Tensor& q) {
  return q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 4
      && q.stride(3) == 1 && (q.size(2) == 1 || q.stride(2) == q.size(3))
      && strides_aligned(q, 2, 8);
}

bool chunk_cache_ok(const torch::Tensor& c, const torch::Tensor& q, bool fp8) {
  return c.is_cuda() && c.device() == q.device() && c.dim() == 4
      && c.dtype() == (fp8 ? torch::kFloat8_e4m3fn : torch::kBFloat16)
      && c.stride(3) == 1 && strides_aligned(c, 3, fp8 ? 16 : 8);
}

bool chunk_scale_ok(const torch::Tensor& s, const torch::Tensor& codes) {
  return s.is_cuda() && s.device() == codes.device()
      && s.dtype() == torch::kFloat32 && s.dim() == 3
      && s.size(0) == codes.size(0) && s.size(1) == codes.size(1)
      && s.size(2) == codes.size(2);
}

ChunkCache chunk_cache(const torch::Tensor& c, const torch::Tensor* scale) {
  ChunkCache r{(const unsigned char*)c.data_ptr(), (long)c.stride(0),
               (long)c.stride(1), (long)c.stride(2), nullptr, 0, 0, 0};
  if (scale != nullptr) {
    r.scale = scale->data_ptr<float>();
    r.s_sb = scale->stride(0);
    r.s_sr = scale->stride(1);
    r.s_sh = scale->stride(2);
  }
  return r;
}

template <int D, bool FP8>
void launch_chunk(const torch::Tensor& q, const ChunkCache& kc,
                  const ChunkCache& vc, const torch::Tensor& kv_lens,
                  torch::Tensor& ws_ml, torch::Tensor& ws_acc,
                  torch::Tensor& o, torch::Tensor& lse, int Lmax, int Hkv,
                  int chunk, int NC, hipStream_t stream) {
  const int B = q.size(0), T = q.size(1), Hq = q.size(2);
  const int rep = Hq / Hkv;
  const int ntiles = (T * rep + DCH_ROWS - 1) / DCH_ROWS;
  const float scale2 = 1.44269504f / sqrtf((float)D);
  hipLaunchKernelGGL((chunk_partial_kernel<D, FP8>),
                     dim3(NC, Hkv * ntiles, B), dim3(DEC_THREADS), 0, stream,
                     (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                     (long)q.stride(1), kc, vc, kv_lens.data_ptr<int>(),
                     ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(), Lmax,
                     T, Hq, rep, ntiles, chunk, NC, scale2);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL((chunk_combine_kernel<D>), dim3(T * Hq, B), dim3(128), 0,
                     stream, ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(),
                     kv_lens.data_ptr<int>(), (unsigned short*)o.data_ptr(),
                     lse.data_ptr<float>(), Lmax, T, Hq, chunk, NC);
  HIP_CHECK_KERNEL();
}

template <bool FP8>
std::vector<torch::Tensor> chunk_fwd(const char* name, const torch::Tensor& q,
                                     const torch::Tensor& k_cache,
                                     const torch::Tensor* k_scale,
                                     const torch::Tensor& v_cache,
                                     const torch::Tensor* v_scale,
                                     const torch::Tensor& kv_lens,
                                     long kv_chunk) {
  TORCH_CHECK(q.dim() == 4 && k_cache.dim() == 4, name,
              ": q must be [B,T,Hq,D], caches [B,Lmax,Hkv,D]");
  const long B = q.size(0), T = q.size(1), Hq = q.size(2), D = q.size(3);
  const long Lmax = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(T >= 2, name, ": q must hold T >= 2 tokens per row, got ", T,
              " (decode_attn_fwd serves T == 1)");
  TORCH_CHECK(D == 64 || D == 80 || D == 128, name,
              ": head_dim must be 64, 80 or 128, got ", D);
  TORCH_CHECK(chunk_q_ok(q), name, ": q must be device bf16 [B,T,Hq,D] with "
              "contiguous heads and 16-byte aligned token and batch strides");
  TORCH_CHECK(chunk_cache_ok(k_cache, q, FP8) && chunk_cache_ok(v_cache, q, FP8)
              && k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B
              && k_cache.size(3) == D, name, ": k_cache/v_cache must be device ",
              FP8 ? "float8_e4m3fn" : "bf16", " [B,Lmax,Hkv,D] of one shape, "
              "unit stride in D and 16-byte aligned batch/row/head strides");
  if (FP8)
    TORCH_CHECK(chunk_scale_ok(*k_scale, k_cache)
                && chunk_scale_ok(*v_scale, v_cache), name,
                ": k_scale/v_scale must be device fp32 [B,Lmax,Hkv]");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, name,
              ": Hq must be a multiple of Hkv");
  TORCH_CHECK(index_ok(kv_lens, q, B), name,
              ": kv_lens must be a contiguous device int32 [B]");
  TORCH_CHECK(kv_chunk == 0 || (kv_chunk >= DCH_KV_CHUNK_MIN
                                && kv_chunk % DCH_KV_CHUNK_MIN == 0), name,
              ": kv_chunk must be 0 (default ", DCH_KV_CHUNK,
              ") or a multiple of ", DCH_KV_CHUNK_MIN,
              "; the smallest legal value is ", DCH_KV_CHUNK_MIN);
  const long chunk = kv_chunk == 0 ? DCH_KV_CHUNK : kv_chunk;
  const long NC = std::max<long>(1, (Lmax + chunk - 1) / chunk);
  const long rep = Hq / Hkv;
  const long ntiles = (T * rep + DCH_ROWS - 1) / DCH_ROWS;
  TORCH_CHECK(B <= 65535 && Hkv * ntiles <= 65535 && T * Hq < (1L << 31)
              && T < (1L << 20) && Lmax < (1L << 30), name,
              ": batch, token count, head count or cache length too large");

  auto o = torch::empty({B, T, Hq, D}, q.options());
  auto lse = torch::empty({B, Hq, T}, q.options().dtype(torch::kFloat32));
  if (B == 0 || Hq == 0) return {o, lse};
  auto ws_ml = torch::empty({B, T * Hq, NC, 2}, lse.options());
  auto ws_acc = torch::empty({B, T * Hq, NC, D}, lse.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const ChunkCache kc = chunk_cache(k_cache, k_scale);
  const ChunkCache vc = chunk_cache(v_cache, v_scale);
  if (D == 64)
    launch_chunk<64, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                          (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else if (D == 80)
    launch_chunk<80, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                          (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else
    launch_chunk<128, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                           (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  return {o, lse};
}

}  // namespace

long decode_attn_chunk_kv_chunk() { return DCH_KV_CHUNK; }
long decode_attn_chunk_kv_chunk_min() { return DCH_KV_CHUNK_MIN; }
long decode_attn_chunk_wave_keys() { return DCH_WAVE_KEYS; }

std::vector<torch::Tensor> decode_attn_chunk_fwd(torch::Tensor q,
                                                 torch::Tensor k_cache,
                                                 torch::Tensor v_cache,
                                                 torch::Tensor kv_lens,
                                                 long kv_chunk) {
  return chunk_fwd<false>("decode_attn_chunk", q, k_cache, nullptr, v_cache,
                          nullptr, kv_lens, kv_chunk);
}

std::vector<torch::Tensor> decode_attn_chunk_fp8_fwd(torch::Tensor q,
                                                     torch::Tensor k_codes,
                                                     torch::Tensor k_scale,
                                                     torch::Tensor v_codes,
                                                     torch::Tensor v_scale,
                                                     torch::Tensor kv_lens,
                                                     long kv_chunk) {
  return chunk_fwd<true>("decode_attn_chunk_fp8", q, k_codes, &k_scale,
                         v_codes, &v_scale, kv_lens, kv_chunk);
}
