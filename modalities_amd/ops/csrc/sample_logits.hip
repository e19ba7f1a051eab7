// Token sampler for the decode step: temperature, top-k, top-p and the draw in
// one kernel, from the logits where lm_head left them to the int64 id the
// next step reads. Inference only.
//
// sample_logits(logits [B,V] bf16 | fp32 (row-strided), u fp32 [B] in [0,1),
//               out_ids int64 [B] | [B,1], temperature, top_k, top_p)
//
// Semantics (ops/sampling.py holds the torch reference):
//   temperature <= 0: the lowest index among the maxima. Otherwise, with
//   z = logits / temperature,
//   top-k : keep z >= (k-th largest z), ties included;
//   top-p : pr = softmax over the top-k survivors, G(i) = mass of survivors
//           with z strictly greater than z_i; keep i iff G(i) <= top_p (the
//           top token always stays, a tie class stays or goes whole);
//   draw  : w = pr * keep, c = inclusive prefix sum of w in vocabulary order;
//           the smallest i with w_i > 0 and c_i > u * c_last (the last i with
//           w_i > 0 when rounding leaves none).
//
// Nothing is sorted. One workgroup of 1024 threads (16 waves) owns a row and
// passes over it several times:
//
//  * Keys. An element is turned into an order-preserving unsigned key of its
//    own width (16 bits for bf16, 32 for fp32; -0 counts as +0). Dividing by
//    a positive temperature is monotone, so both thresholds are found on the
//    keys of the stored values: exact, ties need no special case.
//  * Where the keys live. The load pass writes the row's keys to LDS when
//    they fit beside the histograms in what the device reports (160 KB on
//    gfx950: bf16 up to V = 73,088, fp32 up to V = 36,544), and every later
//    pass reads 16-byte LDS chunks. A longer row (fp32 at V = 50,257 or
//    50,304) is re-read from global memory, L2 resident, in every pass. A
//    row whose base is 16-byte aligned is loaded in 16-byte pieces; any other
//    (odd V in a contiguous [B,V]) takes element-wide loads, coalesced in
//    the LDS load pass. Greedy is a single pass over global memory.
//  * Top-k threshold: radix select from the top, 8 bits per level (2 levels
//    for bf16, 4 for fp32). A level counts the digit of the elements that
//    share the prefix found so far into one 256-bin LDS histogram; a wave
//    aggregates its increments (one atomic per distinct digit and wave step,
//    by a leader lane). Wave 0 then scans the bins from the top.
//  * Top-p threshold: the same descent with a mass histogram: a bin holds
//    the sum of exp2(z * log2e - m) of its elements. Sums have one order: a
//    wave sums the lanes that share a digit by the xor-shuffle tree and its
//    leader adds that to the wave's own 256 bins, wave step by wave step;
//    wave 0 then adds the 16 partials of a bin in wave order and scans the
//    bins by a shuffle scan. The lowest bin that holds mass and whose
//    strictly-greater mass G is <= top_p * total is descended into. No float
//    atomics; which thread handles an element depends on its index alone, so
//    a row gives the same token at every batch position, alignment and run.
//  * Draw: a thread owns a contiguous run of chunks and sums its kept
//    weights in index order; shuffle scan inside a wave, wave sums in wave
//    order through LDS. The first thread whose inclusive sum passes
//    u * total walks its run again (same operations, same order) and writes
//    the id. For u >= 1/2 the same scan runs from the back of the vocabulary
//    against (1 - u) * total, so masses near either end keep their own
//    precision.
//
// No launch argument depends on the decode step and nothing is allocated:
// the launch is graph-capturable.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <limits.h>
#include <cmath>
#include "common.h"

namespace {

constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / WAVE_SIZE;
constexpr int SMP_BINS = 256;
constexpr int SMP_MAX_V = 1 << 24;

typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

struct SampleShared {
  float mass[SMP_WAVES][SMP_BINS];   // per-wave partial mass histograms
  unsigned int count[SMP_BINS];
  float wave_sum[SMP_WAVES];
  unsigned long long best;           // greedy: key << 32 | ~index
  unsigned int key_max;
  unsigned int digit;
  unsigned int k_rem;
  float carried;
  int first;
  int last;
};

// static LDS of the kernel, rounded up: what the row's keys cannot have
constexpr size_t SMP_STATIC_LDS = (sizeof(SampleShared) + 255) / 256 * 256;

template <typename K> struct KeyTraits;
template <> struct KeyTraits<unsigned short> {
  static constexpr int BITS = 16;
  static constexpr int E = 8;   // keys per 16-byte chunk
};
template <> struct KeyTraits<unsigned int> {
  static constexpr int BITS = 32;
  static constexpr int E = 4;
};

template <typename K>
__device__ __forceinline__ unsigned int to_key(unsigned int raw) {
  constexpr int BITS = KeyTraits<K>::BITS;
  constexpr unsigned int SIGN = 1u << (BITS - 1);
  constexpr unsigned int MASK = SIGN | (SIGN - 1);
  if ((raw & (SIGN - 1)) == 0) raw = 0;   // -0 is +0
  return (raw & SIGN) ? (~raw & MASK) : (raw | SIGN);
}

template <typename K>
__device__ __forceinline__ float key_value(unsigned int key) {
  constexpr int BITS = KeyTraits<K>::BITS;
  constexpr unsigned int SIGN = 1u << (BITS - 1);
  constexpr unsigned int MASK = SIGN | (SIGN - 1);
  const unsigned int raw = (key & SIGN) ? (key & ~SIGN) : (~key & MASK);
  return __uint_as_float(BITS == 16 ? raw << 16 : raw);
}

template <typename K>
__device__ __forceinline__ void unpack(const uintx4& v,
                                       unsigned int (&k)[KeyTraits<K>::E]) {
  if constexpr (KeyTraits<K>::BITS == 16) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      k[2 * d] = v[d] & 0xffffu;
      k[2 * d + 1] = v[d] >> 16;
    }
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) k[d] = v[d];
  }
}

// A row: raw elements in global memory, or (LDS) its keys in shared memory.
// chunk(c) yields the keys of elements c*E .. c*E+E-1; those at or beyond V
// are unspecified and the caller masks them. c < ceil(V / E).
template <typename K, bool LDS>
struct Row {
  static constexpr int E = KeyTraits<K>::E;
  const K* g;
  const K* s;
  int V;
  bool vec;   // g is 16-byte aligned

  __device__ __forceinline__ void chunk(int c, unsigned int (&k)[E]) const {
    if constexpr (LDS) {
      unpack<K>(*reinterpret_cast<const uintx4*>(s + (long)c * E), k);
    } else {
      const int i0 = c * E;
      if (vec && i0 + E <= V) {
        unpack<K>(*reinterpret_cast<const uintx4*>(g + i0), k);
#pragma unroll
        for (int j = 0; j < E; ++j) k[j] = to_key<K>(k[j]);
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j)
          k[j] = i0 + j < V ? to_key<K>(g[i0 + j]) : 0u;
      }
    }
  }
};

// Inclusive suffix sum over the lanes of a wave (lane l: lanes l .. 63), by
// a fixed shuffle ladder.
template <typename T>
__device__ __forceinline__ T wave_suffix_sum(T v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const T o = __shfl_down(v, off, WAVE_SIZE);
    if (lane + off < WAVE_SIZE) v += o;
  }
  return v;
}

__device__ __forceinline__ float wave_prefix_sum(float v, int lane) {
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const float o = __shfl_up(v, off, WAVE_SIZE);
    if (lane >= off) v += o;
  }
  return v;
}

// One wave step of a count histogram: the lanes that share a digit add
// their number with one atomic, issued by the first of them.
__device__ __forceinline__ void wave_count(unsigned int* hist, bool active,
                                           unsigned int digit, int lane) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned int d = __shfl(digit, leader, WAVE_SIZE);
    const unsigned long long same = __ballot(active && digit == d);
    if (lane == leader) atomicAdd(&hist[d], (unsigned int)__popcll(same));
    todo &= ~same;
  }
}

// The same for mass, into the wave's own bins: the xor tree sums the lanes
// of a digit, the leader adds the sum to the bin. One writer per bin and
// step, steps in program order: the bin's sum has a fixed order.
__device__ __forceinline__ void wave_mass(float* hist, bool active,
                                          unsigned int digit, float w,
                                          int lane) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned int d = __shfl(digit, leader, WAVE_SIZE);
    const bool mine = active && digit == d;
    const unsigned long long same = __ballot(mine);
    const float s = wave_reduce_sum(mine ? w : 0.f);
    if (lane == leader) hist[d] += s;
    todo &= ~same;
  }
}

template <typename K, bool LDS>
struct Sampler {
  static constexpr int BITS = KeyTraits<K>::BITS;
  static constexpr int E = KeyTraits<K>::E;
  static constexpr int LEVELS = BITS / 8;

  Row<K, LDS> row;
  SampleShared& sh;
  int nchunks;
  int tid, lane, wave;
  float scale;   // log2(e) / temperature
  float m;       // max z, in the exp2 domain

  __device__ __forceinline__ float weight(unsigned int key) const {
    return __builtin_amdgcn_exp2f(fmaf(key_value<K>(key), scale, -m));
  }

  // does key carry `prefix` above the digit of `level`?
  static __device__ __forceinline__ bool in_prefix(unsigned int key, int level,
                                                   unsigned int prefix) {
    return level == 0 || (key >> (BITS - 8 * level)) == prefix;
  }
  static __device__ __forceinline__ unsigned int digit_of(unsigned int key,
                                                          int level) {
    return (key >> (BITS - 8 * (level + 1))) & (SMP_BINS - 1);
  }

  // The k-th largest key of the row, 1 <= k <= V.
  __device__ unsigned int kth_largest(unsigned int k) {
    unsigned int prefix = 0;
    for (int level = 0; level < LEVELS; ++level) {
      if (tid < SMP_BINS) sh.count[tid] = 0;
      __syncthreads();
      for (int c0 = 0; c0 < nchunks; c0 += SMP_THREADS) {
        const int c = c0 + tid;
        unsigned int key[E] = {};
        if (c < nchunks) row.chunk(c, key);
#pragma unroll
        for (int j = 0; j < E; ++j) {
          const bool on = c < nchunks && c * E + j < row.V
                          && in_prefix(key[j], level, prefix);
          wave_count(sh.count, on, digit_of(key[j], level), lane);
        }
      }
      __syncthreads();
      if (wave == 0) {   // lane l holds bins 4l .. 4l+3; scan from the top
        unsigned int n[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) n[q] = sh.count[4 * lane + q];
        const unsigned int mine = n[0] + n[1] + n[2] + n[3];
        unsigned int above = wave_suffix_sum(mine, lane) - mine;
#pragma unroll
        for (int q = 3; q >= 0; --q) {
          if (above < k && above + n[q] >= k) {
            sh.digit = 4 * lane + q;
            sh.k_rem = k - above;
          }
          above += n[q];
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sh.digit;
      k = sh.k_rem;
    }
    return prefix;
  }

  // The smallest key >= floor_key whose strictly-greater mass among the
  // keys >= floor_key is <= top_p of their whole mass.
  __device__ unsigned int nucleus_floor(unsigned int floor_key, float top_p) {
    unsigned int prefix = 0;
    float carried = 0.f;   // mass above the prefix' range
    float budget = 0.f;    // top_p * total; wave 0 holds it
    for (int level = 0; level < LEVELS; ++level) {
      for (int i = tid; i < SMP_WAVES * SMP_BINS; i += SMP_THREADS)
        (&sh.mass[0][0])[i] = 0.f;
      __syncthreads();
      for (int c0 = 0; c0 < nchunks; c0 += SMP_THREADS) {
        const int c = c0 + tid;
        unsigned int key[E] = {};
        if (c < nchunks) row.chunk(c, key);
#pragma unroll
        for (int j = 0; j < E; ++j) {
          bool on = c < nchunks && c * E + j < row.V && key[j] >= floor_key
                    && in_prefix(key[j], level, prefix);
          const float w = on ? weight(key[j]) : 0.f;
          on = on && w > 0.f;
          wave_mass(sh.mass[wave], on, digit_of(key[j], level), w, lane);
        }
      }
      __syncthreads();
      if (wave == 0) {
        float b[4];   // b[q]: mass of bin 4*lane + q, partials in wave order
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float a = 0.f;
#pragma unroll
          for (int w = 0; w < SMP_WAVES; ++w) a += sh.mass[w][4 * lane + q];
          b[q] = a;
        }
        // up[q]: mass of this lane's bins above bin q
        float up[4];
        up[3] = 0.f;
        up[2] = b[3];
        up[1] = b[2] + up[2];
        up[0] = b[1] + up[1];
        const float incl = wave_suffix_sum(b[0] + up[0], lane);
        float above = __shfl_down(incl, 1, WAVE_SIZE);
        if (lane == WAVE_SIZE - 1) above = 0.f;
        if (level == 0) budget = top_p * __shfl(incl, 0, WAVE_SIZE);
        int pick = SMP_BINS;
        float g_pick = carried;
#pragma unroll
        for (int q = 3; q >= 0; --q) {
          const float g = carried + (above + up[q]);
          if (b[q] > 0.f && g <= budget) {
            pick = 4 * lane + q;
            g_pick = g;
          }
        }
        int lowest = pick;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
          lowest = min(lowest, __shfl_xor(lowest, off, WAVE_SIZE));
        if (lowest == SMP_BINS) {   // no bin qualifies: keep the whole prefix
          if (lane == 0) {
            sh.digit = 0;
            sh.carried = carried;
          }
        } else if (pick == lowest) {
          sh.digit = lowest;
          sh.carried = g_pick;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sh.digit;
      carried = sh.carried;
    }
    return prefix;
  }

  // Visit the kept elements of chunks cb .. ce-1 with their weights, in
  // vocabulary order or (REV) against it; f(index, weight) returns true to
  // stop.
  template <bool REV, typename F>
  __device__ __forceinline__ void visit(unsigned int floor_key, int cb, int ce,
                                        F f) const {
    for (int n = 0; n < ce - cb; ++n) {
      const int c = REV ? ce - 1 - n : cb + n;
      unsigned int key[E];
      row.chunk(c, key);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const int jj = REV ? E - 1 - j : j;
        if (c * E + jj < row.V && key[jj] >= floor_key)
          if (f(c * E + jj, weight(key[jj]))) return;
      }
    }
  }

  // Draw from the keys >= floor_key. With c the inclusive prefix sum of the
  // weights in vocabulary order and T its last value, the smallest i with
  // c_i > u T is also the largest i whose inclusive suffix sum is
  // >= (1 - u) T. u < 1/2 scans from the front, u >= 1/2 (REV) from the
  // back, so a small mass at either end is compared at its own precision
  // and not at T's. REV mirrors everything: thread t owns the run of
  // thread 1023 - t and walks it backwards; "first" below is in scan order.
  template <bool REV>
  __device__ void draw(unsigned int floor_key, float u, long long* out) {
    const int per_thread = (nchunks + SMP_THREADS - 1) / SMP_THREADS;
    const int owner = REV ? SMP_THREADS - 1 - tid : tid;
    const int cb = min(owner * per_thread, nchunks);
    const int ce = min(cb + per_thread, nchunks);
    float seg = 0.f;
    visit<REV>(floor_key, cb, ce, [&](int, float w) {
      seg += w;
      return false;
    });
    const float incl_w = wave_prefix_sum(seg, lane);
    if (lane == WAVE_SIZE - 1) sh.wave_sum[wave] = incl_w;
    if (tid == 0) {
      sh.first = INT_MAX;
      sh.last = -1;
    }
    __syncthreads();
    float base = 0.f, total = 0.f;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) {
      if (w == wave) base = total;
      total += sh.wave_sum[w];
    }
    float before = __shfl_up(incl_w, 1, WAVE_SIZE);
    if (lane == 0) before = 0.f;
    const float excl = base + before;
    const float target = (REV ? 1.f - u : u) * total;
    auto reached = [&](float c) { return REV ? c >= target : c > target; };
    if (seg > 0.f) {
      atomicMax(&sh.last, tid);
      if (reached(excl + seg)) atomicMin(&sh.first, tid);
    }
    __syncthreads();
    const int chosen = sh.first != INT_MAX ? sh.first : sh.last;
    if (chosen < 0) {   // no weight anywhere (a row of -inf or NaN)
      if (tid == 0) *out = 0;
      return;
    }
    if (tid != chosen) return;
    // the same weights in the same order as seg: run ends at seg
    float run = 0.f;
    int last = -1;
    visit<REV>(floor_key, cb, ce, [&](int i, float w) {
      if (w > 0.f) {
        run += w;
        last = i;
      }
      return w > 0.f && reached(excl + run);
    });
    *out = last;   // where the walk stopped, or the last weight it met
  }
};

template <typename K, bool LDS>
__global__ __launch_bounds__(SMP_THREADS)
void sample_logits_kernel(const K* __restrict__ logits, long row_stride,
                          const float* __restrict__ u,
                          long long* __restrict__ out, long out_stride, int V,
                          float scale, int top_k, float top_p, bool greedy) {
  constexpr int E = KeyTraits<K>::E;
  __shared__ SampleShared sh;
  extern __shared__ __attribute__((aligned(16))) char smp_row_raw[];
  K* keys = reinterpret_cast<K*>(smp_row_raw);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  const K* g = logits + (long)blockIdx.x * row_stride;
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  const int nchunks = (V + E - 1) / E;
  long long* out_row = out + (long)blockIdx.x * out_stride;

  if (tid == 0) {
    sh.best = 0;
    sh.key_max = 0;
  }
  __syncthreads();

  if (greedy) {   // one pass: largest key, lowest index
    const Row<K, false> row{g, nullptr, V, vec};
    unsigned long long best = 0;
    for (int c = tid; c < nchunks; c += SMP_THREADS) {
      unsigned int key[E];
      row.chunk(c, key);
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const unsigned int i = c * E + j;
        if (i < (unsigned int)V) {
          const unsigned long long cand =
              ((unsigned long long)key[j] << 32) | (0xffffffffu - i);
          best = cand > best ? cand : best;
        }
      }
    }
    atomicMax(&sh.best, best);
    __syncthreads();
    if (tid == 0)
      *out_row = (long long)(0xffffffffu - (unsigned int)sh.best);
    return;
  }

  // load pass: the row's largest key, and (LDS) its keys into shared memory
  unsigned int key_max = 0;
  if (LDS && !vec) {
    for (int i = tid; i < V; i += SMP_THREADS) {
      const unsigned int key = to_key<K>(g[i]);
      keys[i] = (K)key;
      key_max = max(key_max, key);
    }
  } else {
    const Row<K, false> row{g, nullptr, V, vec};
    for (int c = tid; c < nchunks; c += SMP_THREADS) {
      unsigned int key[E];
      row.chunk(c, key);   // keys beyond V are 0
#pragma unroll
      for (int j = 0; j < E; ++j)
        if (c * E + j < V) key_max = max(key_max, key[j]);
      if constexpr (LDS) {
        uintx4 v;
        if constexpr (E == 8) {
#pragma unroll
          for (int d = 0; d < 4; ++d) v[d] = key[2 * d] | (key[2 * d + 1] << 16);
        } else {
#pragma unroll
          for (int d = 0; d < 4; ++d) v[d] = key[d];
        }
        *reinterpret_cast<uintx4*>(keys + (long)c * E) = v;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    key_max = max(key_max, __shfl_xor(key_max, off, WAVE_SIZE));
  if (lane == 0) atomicMax(&sh.key_max, key_max);
  __syncthreads();

  Sampler<K, LDS> s{Row<K, LDS>{g, keys, V, vec}, sh, nchunks, tid, lane, wave,
                    scale, key_value<K>(sh.key_max) * scale};
  unsigned int floor_key = 0;
  if (top_k > 0 && top_k < V) floor_key = s.kth_largest((unsigned int)top_k);
  if (top_p > 0.f && top_p < 1.f)
    floor_key = max(floor_key, s.nucleus_floor(floor_key, top_p));
  float ur = u[blockIdx.x];
  ur = fminf(fmaxf(ur, 0.f), 0x1.fffffep-1f);
  if (ur < 0.5f) s.template draw<false>(floor_key, ur, out_row);
  else s.template draw<true>(floor_key, ur, out_row);
}

template <typename K, bool LDS>
void launch_sample(const torch::Tensor& logits, const torch::Tensor& u,
                   torch::Tensor& out, float scale, int top_k, float top_p,
                   bool greedy, size_t row_bytes, size_t row_bytes_max,
                   hipStream_t stream) {
  auto kernel = sample_logits_kernel<K, LDS>;
  if (LDS) {
    static bool raised = false;   // dynamic LDS beyond the 64 KB default
    if (!raised) {
      hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(kernel),
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_bytes_max);
      TORCH_CHECK(e == hipSuccess, "sample_logits: cannot raise the LDS "
                  "limit: ", hipGetErrorString(e));
      raised = true;
    }
  }
  hipLaunchKernelGGL(kernel, dim3(logits.size(0)), dim3(SMP_THREADS),
                     LDS ? row_bytes : 0, stream,
                     (const K*)logits.data_ptr(), (long)logits.stride(0),
                     u.data_ptr<float>(), (long long*)out.data_ptr(),
                     (long)out.stride(0), (int)logits.size(1), scale, top_k,
                     top_p, greedy);
  HIP_CHECK_KERNEL();
}

size_t lds_per_block(int device) {
  static int cached[64] = {0};
  if (device < 0 || device >= 64) return 0;
  if (cached[device] == 0) {
    int v = 0;
    hipError_t e = hipDeviceGetAttribute(
        &v, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
    TORCH_CHECK(e == hipSuccess, "sample_logits: ", hipGetErrorString(e));
    cached[device] = v > 0 ? v : -1;
  }
  return cached[device] > 0 ? (size_t)cached[device] : 0;
}

}  // namespace

// 1 when a [., V] row of this element size is staged in LDS on `device`, 0
// when every pass re-reads global memory.
long sample_logits_row_in_lds(long V, long elem_size, long device) {
  const size_t row_bytes = ((size_t)V * elem_size + 15) / 16 * 16;
  return row_bytes + SMP_STATIC_LDS <= lds_per_block((int)device);
}

void sample_logits(torch::Tensor logits, torch::Tensor u,
                   torch::Tensor out_ids, double temperature, long top_k,
                   double top_p) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2,
              "sample_logits: logits must be a device [B, V] tensor");
  const bool bf16 = logits.dtype() == torch::kBFloat16;
  TORCH_CHECK(bf16 || logits.dtype() == torch::kFloat32,
              "sample_logits: logits must be bf16 or fp32");
  const long B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && V >= 1 && V <= SMP_MAX_V,
              "sample_logits: B must be in [1, 65535] and V in [1, ",
              SMP_MAX_V, "], got ", B, " and ", V);
  TORCH_CHECK((V == 1 || logits.stride(1) == 1) && logits.stride(0) >= 0,
              "sample_logits: logits need unit stride in V");
  TORCH_CHECK(u.is_cuda() && u.device() == logits.device()
              && u.dtype() == torch::kFloat32 && u.dim() == 1
              && u.size(0) == B && u.is_contiguous(),
              "sample_logits: u must be contiguous device fp32 [B]");
  TORCH_CHECK(out_ids.is_cuda() && out_ids.device() == logits.device()
              && out_ids.dtype() == torch::kInt64 && out_ids.size(0) == B
              && (out_ids.dim() == 1
                  || (out_ids.dim() == 2 && out_ids.size(1) == 1))
              && (B == 1 || out_ids.stride(0) >= 1),
              "sample_logits: out_ids must be device int64 [B] or [B, 1]");
  const bool greedy = !(temperature > 0.0);
  const float scale = greedy ? 1.f : (float)(1.4426950408889634 / temperature);
  TORCH_CHECK(std::isfinite(scale) && scale > 0.f,
              "sample_logits: temperature out of range: ", temperature);
  const int k = (int)std::min<long>(std::max<long>(top_k, 0), V);
  const float p = (top_p > 0.0 && top_p < 1.0) ? (float)top_p : 0.f;
  auto stream = at::cuda::getCurrentHIPStream();
  const size_t row_bytes = ((size_t)V * logits.element_size() + 15) / 16 * 16;
  const bool lds = !greedy && sample_logits_row_in_lds(
      V, logits.element_size(), logits.get_device());
  const size_t row_bytes_max =
      lds ? lds_per_block(logits.get_device()) - SMP_STATIC_LDS : 0;
  if (bf16) {
    if (lds) launch_sample<unsigned short, true>(logits, u, out_ids, scale, k,
                                                 p, greedy, row_bytes, row_bytes_max,
                                                 stream);
    else launch_sample<unsigned short, false>(logits, u, out_ids, scale, k, p,
                                              greedy, row_bytes, row_bytes_max, stream);
  } else {
    if (lds) launch_sample<unsigned int, true>(logits, u, out_ids, scale, k,
                                               p, greedy, row_bytes, row_bytes_max,
                                                 stream);
    else launch_sample<unsigned int, false>(logits, u, out_ids, scale, k, p,
                                            greedy, row_bytes, row_bytes_max, stream);
  }
}
