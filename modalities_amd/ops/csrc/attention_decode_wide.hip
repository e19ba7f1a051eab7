// K1 decode, long multi-token steps: split-KV attention of T >= 2 new tokens
// per batch row over a preallocated KV cache (bf16, or e4m3 codes with
// per-row scales), on the matrix cores, for the row counts at which
// attention_decode_chunk.hip re-streams the cache once per 16 query rows: a
// chunk of a chunked prefill, the next turn of a cached chat, a long
// speculative verify step. Inference only.
//
// decode_attn_wide_fwd(q [B,T,Hq,D], k_cache/v_cache [B,Lmax,Hkv,D],
//                      kv_lens [B]) -> (o [B,T,Hq,D] bf16, lse [B,Hq,T] fp32)
// decode_attn_wide_fp8_fwd: the same over code caches and fp32 scales
//                      [B,Lmax,Hkv].
// The contract is that of attention_decode_chunk.hip: kv_lens[b] (clamped to
// [0, Lmax]) counts the valid rows including the T new ones, query t sees the
// rows j < kv_lens[b] - (T-1-t), a query without keys gives o = 0, lse =
// -inf, q and the caches are read through their strides, and nothing at or
// beyond a row's length is loaded, neither rows, codes nor scales.
//
//  partial  grid (NC, Hkv * nblocks, B), 256 threads. The T * rep query rows
//           of a kv head (row = t * rep + head-in-group) are cut into blocks
//           of 64; one workgroup owns one (batch row, kv head, row block, kv
//           chunk), so cache bytes leave HBM / L2 once per 64 query rows.
//           Wave w owns the 16-row tile w of the block: its Q^T fragments and
//           its (m, l, acc) state stay in registers for the whole key walk.
//           Staging: the walk goes in steps of 32 keys. All 256 threads move
//           a step's K and V rows HBM -> VGPR -> LDS in 8-element pieces (16
//           bytes of bf16, 8 bytes of e4m3 codes, widened to bf16 at the LDS
//           write with v_cvt_pk_f32_fp8 + v_perm_b32: once per 64 query rows)
//           and the step's fp32 scales into a small LDS array. Two LDS
//           buffers, issue-early / write-late as in attention_v2.hip: before
//           the compute of step s the registers holding step s + 1 are
//           written to the other buffer and the loads of step s + 2 are
//           issued; one barrier per step.
//           LDS images: K and V row-major with a pitch of D + 8 elements. A
//           lane (key = lane % 16, g = lane / 16) reads the 8 elements d =
//           32 s + 8 g of its key as the A operand of score step s with one
//           16-byte read (D = 80: the third step is zero-padded, only g < 2
//           read). V is read back transposed with ds_read_b64_tr_b16.
//           Math, in the chunk kernel's lane layout: S^T = K . Q^T with
//           v_mfma_f32_16x16x32_bf16, two 16-key tiles per step; fp32 online
//           softmax in the exp2 domain; P^T, rounded to bf16, is the B
//           operand of O^T += V^T . P^T as it stands. FP8: the K scale
//           multiplies the fp32 score, the V scale is folded into p.
//           Bounds are per query row. The workgroup walks the chunk's keys
//           below the block's largest limit and loads nothing beyond; a
//           chunk that starts at or beyond that limit ends at once (no query
//           of the block has a key there, and the combine launch reads only
//           the chunks that hold keys of its query, so nothing has to be
//           written). A wave skips the MFMAs of a step wholly beyond its
//           tile's largest limit, and the per-column mask of a step wholly
//           below its tile's smallest limit (the tile's, not the block's:
//           the same result, more steps skipped). Staging and the barrier
//           are outside these branches, so all waves keep one schedule.
//           Each wave writes the unnormalised fp32 partial (m, l, acc[D]) of
//           its 16 queries straight from registers: no merge between waves.
//  combine  grid (T * Hq, B), 128 threads: the per-query merge of
//           attention_decode_chunk.hip (that kernel sits in the other file's
//           anonymous namespace, hence the copy here).
//
// The chunk length is WD_KV_CHUNK or the kv_chunk override (a multiple of
// the 32-key step), never a function of Lmax, B or other rows, and nothing
// is accumulated with atomics. A masked key contributes exactly nothing
// (alpha = 1, p = 0), so a query's result is bit-identical whatever cache it
// sits in, whatever shares its batch and whatever shares its tile.
// Workspace: B * T * Hq * NC * (D + 2) fp32 with NC = ceil(Lmax / chunk).
#include <type_traits>

#include "attention_decode_common.h"
#include "attn_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

constexpr int WD_KV_CHUNK = 1024;     // default keys per workgroup
constexpr int WD_STEP = 32;           // keys staged and consumed per step
constexpr int WD_KV_CHUNK_MIN = WD_STEP;          // smallest override
constexpr int WD_TILE = 16;           // query rows per wave
constexpr int WD_ROWS = DEC_WAVES * WD_TILE;      // query rows per workgroup

// a cache with strides in elements; scale is null for bf16
struct WideCache {
  const unsigned char* data;
  long sb, sr, sh;
  const float* scale;
  long s_sb, s_sr, s_sh;
};

__device__ __forceinline__ unsigned int wd_pack_high_halves(float lo,
                                                            float hi) {
  // {lo.b2, lo.b3, hi.b2, hi.b3}: the bf16 of two fp32 with zero low halves
  return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo),
                               0x07060302u);
}

// 8 elements of a cache row as they come from memory, and as bf16 for LDS
template <bool FP8> struct WidePiece {
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
      return uintx4{wd_pack_high_halves(a.x, a.y),
                    wd_pack_high_halves(b.x, b.y),
                    wd_pack_high_halves(c.x, c.y),
                    wd_pack_high_halves(d.x, d.y)};
    } else {
      return r;
    }
  }
};

template <int D, bool FP8>
__global__ __launch_bounds__(DEC_THREADS)
void wide_partial_kernel(const unsigned short* __restrict__ q, long q_sb,
                         long q_st, WideCache kc, WideCache vc,
                         const int* __restrict__ kv_lens,
                         float* __restrict__ ws_ml,
                         float* __restrict__ ws_acc,
                         int Lmax, int T, int Hq, int rep, int nblk,
                         int chunk, int NC, float scale2) {
  using P = WidePiece<FP8>;
  using Raw = typename P::Raw;
  constexpr int ES = FP8 ? 1 : 2;            // bytes per cache element
  constexpr int NS = (D + 31) / 32;          // score MFMA steps per key tile
  constexpr int NDT = D / 16;                // 16-wide d tiles of O^T
  constexpr int PPR = D / 8;                 // 8-element pieces per row
  constexpr int NPC = WD_STEP * PPR;         // pieces per image
  constexpr int NP = (NPC + DEC_THREADS - 1) / DEC_THREADS;   // per thread
  constexpr int PITCH = D + 8;               // image row pitch, elements
  constexpr int IMG = WD_STEP * PITCH * 2;   // bytes per image
  constexpr int SCL = FP8 ? 2 * WD_STEP * 4 : 0;   // K scales, then V scales
  constexpr int BUF = 2 * IMG + SCL;         // K image, V image, scales
  static_assert(IMG % 16 == 0 && BUF % 16 == 0, "16-byte LDS accesses");
  static_assert(2 * WD_STEP <= DEC_THREADS, "one scale per thread");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];

  const int c = blockIdx.x;
  const int hk = blockIdx.y / nblk;
  const int blk = blockIdx.y % nblk;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const int col = lane & 15;                 // key of A, query of B and C
  const int g = lane >> 4;
  const int R = T * rep;                     // query rows of this kv head

  int len = kv_lens[b];
  len = min(max(len, 0), Lmax);
  // the walk: this chunk's keys below the block's largest limit (<= len)
  const int r0 = blk * WD_ROWS;
  const int start = c * chunk;
  const int hi = min(start + chunk,
                     len - (T - 1 - (min(r0 + WD_ROWS, R) - 1) / rep));
  if (start >= hi) return;   // the combine launch never reads this chunk

  // the wave's tile: smallest and largest limit of its rows (0: no row)
  const int w0 = r0 + wave * WD_TILE;
  const bool wave_ok = w0 < R;
  const int wave_lo = wave_ok ? len - (T - 1 - w0 / rep) : 0;
  const int wave_hi =
      wave_ok ? len - (T - 1 - (min(w0 + WD_TILE, R) - 1) / rep) : 0;

  // this lane's query (as B operand and in the result): row, bound, Q^T
  const int row = w0 + col;
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

  // ---- staging: piece x of a step is row x / PPR, elements 8 (x % PPR) ----
  Raw kreg[NP], vreg[NP];
  float sreg = 0.f;
  // every load of the 32-key step at j0; keys at or beyond `hi` load nothing
  auto load = [&](int j0) {
#pragma unroll
    for (int n = 0; n < NP; ++n) {
      const int x = tid + n * DEC_THREADS;
      const int j = j0 + x / PPR;
      kreg[n] = P::zero();
      vreg[n] = P::zero();
      if ((NPC % DEC_THREADS == 0 || x < NPC) && j < hi) {
        kreg[n] = P::load(kb + (long)j * kc.sr * ES, (x % PPR) * 8);
        vreg[n] = P::load(vb + (long)j * vc.sr * ES, (x % PPR) * 8);
      }
    }
    if constexpr (FP8) {
      sreg = 0.f;
      const int j = j0 + (tid & (WD_STEP - 1));
      if (tid < 2 * WD_STEP && j < hi)
        sreg = tid < WD_STEP ? ksb[(long)j * kc.s_sr] : vsb[(long)j * vc.s_sr];
    }
  };
  // the registers into a buffer; unloaded keys enter as zeros
  auto store = [&](unsigned char* buf) {
#pragma unroll
    for (int n = 0; n < NP; ++n) {
      const int x = tid + n * DEC_THREADS;
      if (NPC % DEC_THREADS == 0 || x < NPC) {
        const int off = ((x / PPR) * PITCH + (x % PPR) * 8) * 2;
        *reinterpret_cast<uintx4*>(buf + off) = P::widen(kreg[n]);
        *reinterpret_cast<uintx4*>(buf + IMG + off) = P::widen(vreg[n]);
      }
    }
    if constexpr (FP8) {
      if (tid < 2 * WD_STEP)
        reinterpret_cast<float*>(buf + 2 * IMG)[tid] = sreg;
    }
  };

  // A-operand read: key col of a tile, elements 8 g of a score step
  const int k_off = (col * PITCH + 8 * g) * 2;
  // transposing read: lane group g, lane lam of it, rows 4 g + (lam >> 2)
  const unsigned trb0 = attnc::lds_addr(smem + IMG)
      + (unsigned)(((4 * g + (col >> 2)) * PITCH + 4 * (col & 3)) * 2);

  float m = -INFINITY, l = 0.f;
  floatx4 acc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) acc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (hi - start + WD_STEP - 1) / WD_STEP;
  load(start);
  store(smem);
  __syncthreads();
  if (nsteps > 1) load(start + WD_STEP);
  for (int s = 0; s < nsteps; ++s) {
    // step s + 1 into the other buffer, the loads of step s + 2 in flight
    if (s + 1 < nsteps) {
      store(smem + ((s + 1) & 1) * BUF);
      if (s + 2 < nsteps) load(start + (s + 2) * WD_STEP);
    }
    const int j0 = start + s * WD_STEP;
    if (j0 < wave_hi) {
      const unsigned char* cur = smem + (s & 1) * BUF;
      // ---- S^T = K Q^T ---------------------------------------------------
      floatx4 st[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        st[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
          uintx4 kf = uintx4{0u, 0u, 0u, 0u};
          if (32 * ss + 32 <= D || 32 * ss + 8 * g < D)
            kf = *reinterpret_cast<const uintx4*>(
                cur + tt * 16 * PITCH * 2 + ss * 64 + k_off);
          st[tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, kf),
              __builtin_bit_cast(bf16x8, qfrag[ss]), st[tt], 0, 0, 0);
        }
      }
      float sc[8], vs[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sc[e] = st[e >> 2][e & 3] * scale2;
        vs[e] = 1.f;
      }
      if constexpr (FP8) {
        const float* scl = reinterpret_cast<const float*>(cur + 2 * IMG);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const floatx4 k4 =
              *reinterpret_cast<const floatx4*>(scl + tt * 16 + 4 * g);
          const floatx4 v4 = *reinterpret_cast<const floatx4*>(
              scl + WD_STEP + tt * 16 + 4 * g);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[tt * 4 + i] *= k4[i];
            vs[tt * 4 + i] = v4[i];
          }
        }
      }

      // ---- online softmax; only the trailing steps apply the bound --------
      if (j0 + WD_STEP > wave_lo) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int j = j0 + (e >> 2) * 16 + 4 * g + (e & 3);
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

      // ---- O^T += V^T P^T: batched transposing reads, one drain -----------
      const unsigned trb = trb0 + (unsigned)((s & 1) * BUF);
      uintx2 rv[2 * NDT];
      asm volatile("" ::: "memory");
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
    __syncthreads();   // step s is read, step s + 1 has landed
  }

  // ---- the wave's 16 partials, straight from registers --------------------
  l += __shfl_xor(l, 16, WAVE_SIZE);
  l += __shfl_xor(l, 32, WAVE_SIZE);
  if (!row_ok) return;
  // the partial of query (t, head) sits where the combine kernel looks for
  // head t * Hq + head of T * Hq
  const long part = (((long)b * T + qt) * Hq + qh) * NC + c;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
    *reinterpret_cast<floatx4*>(ws_acc + part * D + dt * 16 + 4 * g) = acc[dt];
  if (g == 0) {
    ws_ml[part * 2] = m;
    ws_ml[part * 2 + 1] = l;
  }
}

// The merge over a query's chunks, one length per query: head index
// t * Hq + h. A query without keys is o = 0, lse = -inf.
template <int D>
__global__ __launch_bounds__(128)
void wide_combine_kernel(const float* __restrict__ ws_ml,
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
bool wide_q_ok(const torch::Tensor& q) {
  return q.is_cuda() && q.dtype() == torch::kBFloat16 && q.dim() == 4
      && q.stride(3) == 1 && (q.size(2) == 1 || q.stride(2) == q.size(3))
      && strides_aligned(q, 2, 8);
}

bool wide_cache_ok(const torch::Tensor& c, const torch::Tensor& q, bool fp8) {
  return c.is_cuda() && c.device() == q.device() && c.dim() == 4
      && c.dtype() == (fp8 ? torch::kFloat8_e4m3fn : torch::kBFloat16)
      && c.stride(3) == 1 && strides_aligned(c, 3, fp8 ? 16 : 8);
}

bool wide_scale_ok(const torch::Tensor& s, const torch::Tensor& codes) {
  return s.is_cuda() && s.device() == codes.device()
      && s.dtype() == torch::kFloat32 && s.dim() == 3
      && s.size(0) == codes.size(0) && s.size(1) == codes.size(1)
      && s.size(2) == codes.size(2);
}

WideCache wide_cache(const torch::Tensor& c, const torch::Tensor* scale) {
  WideCache r{(const unsigned char*)c.data_ptr(), (long)c.stride(0),
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
void launch_wide(const torch::Tensor& q, const WideCache& kc,
                 const WideCache& vc, const torch::Tensor& kv_lens,
                 torch::Tensor& ws_ml, torch::Tensor& ws_acc,
                 torch::Tensor& o, torch::Tensor& lse, int Lmax, int Hkv,
                 int chunk, int NC, hipStream_t stream) {
  const int B = q.size(0), T = q.size(1), Hq = q.size(2);
  const int rep = Hq / Hkv;
  const int nblk = (T * rep + WD_ROWS - 1) / WD_ROWS;
  const float scale2 = 1.44269504f / sqrtf((float)D);
  hipLaunchKernelGGL((wide_partial_kernel<D, FP8>),
                     dim3(NC, Hkv * nblk, B), dim3(DEC_THREADS), 0, stream,
                     (const unsigned short*)q.data_ptr(), (long)q.stride(0),
                     (long)q.stride(1), kc, vc, kv_lens.data_ptr<int>(),
                     ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(), Lmax,
                     T, Hq, rep, nblk, chunk, NC, scale2);
  HIP_CHECK_KERNEL();
  hipLaunchKernelGGL((wide_combine_kernel<D>), dim3(T * Hq, B), dim3(128), 0,
                     stream, ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(),
                     kv_lens.data_ptr<int>(), (unsigned short*)o.data_ptr(),
                     lse.data_ptr<float>(), Lmax, T, Hq, chunk, NC);
  HIP_CHECK_KERNEL();
}

template <bool FP8>
std::vector<torch::Tensor> wide_fwd(const char* name, const torch::Tensor& q,
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
  TORCH_CHECK(wide_q_ok(q), name, ": q must be device bf16 [B,T,Hq,D] with "
              "contiguous heads and 16-byte aligned token and batch strides");
  TORCH_CHECK(wide_cache_ok(k_cache, q, FP8) && wide_cache_ok(v_cache, q, FP8)
              && k_cache.sizes() == v_cache.sizes() && k_cache.size(0) == B
              && k_cache.size(3) == D, name, ": k_cache/v_cache must be device ",
              FP8 ? "float8_e4m3fn" : "bf16", " [B,Lmax,Hkv,D] of one shape, "
              "unit stride in D and 16-byte aligned batch/row/head strides");
  if (FP8)
    TORCH_CHECK(wide_scale_ok(*k_scale, k_cache)
                && wide_scale_ok(*v_scale, v_cache), name,
                ": k_scale/v_scale must be device fp32 [B,Lmax,Hkv]");
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, name,
              ": Hq must be a multiple of Hkv");
  TORCH_CHECK(index_ok(kv_lens, q, B), name,
              ": kv_lens must be a contiguous device int32 [B]");
  TORCH_CHECK(kv_chunk == 0 || (kv_chunk >= WD_KV_CHUNK_MIN
                                && kv_chunk % WD_KV_CHUNK_MIN == 0), name,
              ": kv_chunk must be 0 (default ", WD_KV_CHUNK,
              ") or a multiple of ", WD_KV_CHUNK_MIN,
              "; the smallest legal value is ", WD_KV_CHUNK_MIN);
  const long chunk = kv_chunk == 0 ? WD_KV_CHUNK : kv_chunk;
  const long NC = std::max<long>(1, (Lmax + chunk - 1) / chunk);
  const long rep = Hq / Hkv;
  const long nblk = (T * rep + WD_ROWS - 1) / WD_ROWS;
  TORCH_CHECK(B <= 65535 && Hkv * nblk <= 65535 && T * Hq < (1L << 31)
              && T < (1L << 20) && Lmax < (1L << 30), name,
              ": batch, token count, head count or cache length too large");

  auto o = torch::empty({B, T, Hq, D}, q.options());
  auto lse = torch::empty({B, Hq, T}, q.options().dtype(torch::kFloat32));
  if (B == 0 || Hq == 0) return {o, lse};
  auto ws_ml = torch::empty({B, T * Hq, NC, 2}, lse.options());
  auto ws_acc = torch::empty({B, T * Hq, NC, D}, lse.options());
  auto stream = at::cuda::getCurrentHIPStream();
  const WideCache kc = wide_cache(k_cache, k_scale);
  const WideCache vc = wide_cache(v_cache, v_scale);
  if (D == 64)
    launch_wide<64, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                         (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else if (D == 80)
    launch_wide<80, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                         (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  else
    launch_wide<128, FP8>(q, kc, vc, kv_lens, ws_ml, ws_acc, o, lse,
                          (int)Lmax, (int)Hkv, (int)chunk, (int)NC, stream);
  return {o, lse};
}

}  // namespace

long decode_attn_wide_kv_chunk() { return WD_KV_CHUNK; }
long decode_attn_wide_kv_chunk_min() { return WD_KV_CHUNK_MIN; }
long decode_attn_wide_key_step() { return WD_STEP; }
long decode_attn_wide_rows() { return WD_ROWS; }

std::vector<torch::Tensor> decode_attn_wide_fwd(torch::Tensor q,
                                                torch::Tensor k_cache,
                                                torch::Tensor v_cache,
                                                torch::Tensor kv_lens,
                                                long kv_chunk) {
  return wide_fwd<false>("decode_attn_wide", q, k_cache, nullptr, v_cache,
                         nullptr, kv_lens, kv_chunk);
}

std::vector<torch::Tensor> decode_attn_wide_fp8_fwd(torch::Tensor q,
                                                    torch::Tensor k_codes,
                                                    torch::Tensor k_scale,
                                                    torch::Tensor v_codes,
                                                    torch::Tensor v_scale,
                                                    torch::Tensor kv_lens,
                                                    long kv_chunk) {
  return wide_fwd<true>("decode_attn_wide_fp8", q, k_codes, &k_scale,
                        v_codes, &v_scale, kv_lens, kv_chunk);
}
