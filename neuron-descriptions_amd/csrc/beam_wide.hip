// Wide beam search: the beam merge and the per-row
// top-k for beam widths whose candidates do not fit LDS (126 <= beam <= 1024).
//
// Both kernels select by the rule of beam_merge_kernel / row_select_reg_kernel
// (decoder.hip): value descending, ties to the lowest index.  They find the
// k-th largest order-preserving key by bisection, gather what lies above it,
// take the entries equal to it in index order until k are held, and sort the
// <= 1024 winners with a bitonic network over (key desc, index asc).  Nothing
// depends on the order in which an atomic lands: slots filled through a counter
// are sorted afterwards, everything else is placed by a prefix scan.
//
// The kernels of decoder.hip are not touched by any of this; the helpers below
// restate its block reductions and key mapping (same operations, same order).
#include "common.h"

namespace milan {
namespace {

constexpr float kFloatMin = -3.402823466e+38f;  // torch.finfo(f32).min
constexpr int kWideSlots = 1024;                // winners of one selection
constexpr int kRowRegs = 24;                    // as row_select_reg_kernel

__device__ inline unsigned fkey(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float funkey(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ inline float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ inline float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
// sum / max / min of one integer per thread over the 256 threads (red: 4 words)
__device__ inline int block_count(int c, int* red) {
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ inline unsigned block_umax(unsigned v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (int)v;
  __syncthreads();
  return max(max((unsigned)red[0], (unsigned)red[1]), max((unsigned)red[2], (unsigned)red[3]));
}
__device__ inline unsigned block_umin(unsigned v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (int)v;
  __syncthreads();
  return min(min((unsigned)red[0], (unsigned)red[1]), min((unsigned)red[2], (unsigned)red[3]));
}
// exclusive prefix of one integer per thread, in thread order
__device__ inline int block_excl_scan(int v, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  __syncthreads();
  if (lane == 63) red[wave] = incl;
  __syncthreads();
  int base = incl - v;
  for (int w = 0; w < wave; ++w) base += red[w];
  return base;
}
// s[0..1024) (LDS, written by the caller, no barrier needed before the call)
// becomes its own exclusive prefix sum; returns the total
__device__ inline int block_excl_scan_1024(int* s, int* red) {
  __syncthreads();
  const int4 v = reinterpret_cast<const int4*>(s)[threadIdx.x];
  const int t0 = v.x, t1 = t0 + v.y, t2 = t1 + v.z, t3 = t2 + v.w;
  const int base = block_excl_scan(t3, red);
  reinterpret_cast<int4*>(s)[threadIdx.x] = make_int4(base, base + t0, base + t1, base + t2);
  const int total = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return total;
}

// One winner: key in the high word, ~index in the low word, so that a descending
// order of the 64-bit value is (key descending, index ascending).  0 pads: the key
// of every non-NaN float is > 0.
__device__ inline unsigned long long slot_of(unsigned key, int idx) {
  return ((unsigned long long)key << 32) | (unsigned)~idx;
}
__device__ inline unsigned slot_key(unsigned long long s) { return (unsigned)(s >> 32); }
__device__ inline int slot_idx(unsigned long long s) { return (int)~(unsigned)s; }

// s[0..P) descending, P a power of two <= 1024; 256 threads
__device__ inline void bitonic_desc(unsigned long long* s, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (P >> 1); t += 256) {
        const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
        const int q = i | stride;
        const unsigned long long a = s[i], b = s[q];
        const bool desc = (i & size) == 0;
        if (desc ? a < b : a > b) { s[i] = b; s[q] = a; }
      }
    }
  __syncthreads();
}
__device__ inline int pow2_at_least(int k) {
  int P = 1;
  while (P < k) P <<= 1;
  return P;
}

// ---------------------------------------------------------------------------
// beam merge
// ---------------------------------------------------------------------------
// Per neuron, the `beam` best of the beam_prev * beam candidates
// cand_v[p][j] + last_lp[p] (the addition of beam_merge_kernel), read from
// global memory.  Every parent's list arrives sorted (value descending) and
// adding one fp32 number is monotone, so a parent's entries at or above a
// threshold are a prefix of its list: the bisection counts them by binary
// search inside the list, between the bounds the earlier rounds left.  Parent
// p belongs to thread p % 256 (beam_prev <= 1024: at most 4 per thread).
// Ties inside a list are already in flat-index order, so "the lowest flat
// indices among the entries equal to the threshold" are prefixes again, shared
// out over the parents by a prefix sum.  ~40 loads per parent instead of the
// whole candidate matrix.
__global__ __launch_bounds__(256) void beam_merge_wide_kernel(
    const float* __restrict__ cand_v, const int* __restrict__ cand_i,
    const float* __restrict__ last_lp, int beam_prev, int beam,
    float* __restrict__ new_lp, int* __restrict__ new_tok,
    int* __restrict__ new_bp) {
  __shared__ unsigned long long slot[kWideSlots];
  __shared__ __attribute__((aligned(16))) int scan[kWideSlots];
  __shared__ int red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* cv = cand_v + (long)n * beam_prev * beam;
  const float* lpn = last_lp ? last_lp + (long)n * beam_prev : nullptr;
  float lp[4];
  int a[4], b[4];  // count(key > hi) and count(key >= lo) of the parent
  unsigned hi = 0u;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int p = tid + 256 * u;
    const bool has = p < beam_prev;
    lp[u] = (has && lpn) ? lpn[p] : 0.f;
    a[u] = 0;
    b[u] = has ? beam : 0;
    if (has) hi = max(hi, fkey(cv[(long)p * beam] + lp[u]));
  }
  hi = block_umax(hi, red);
  unsigned lo = 0u;  // largest T with count(key >= T) >= beam lies in [lo, hi]
  while (lo < hi) {  // block-uniform
    const unsigned mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);
    int c[4], mine = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // entries [0, x) have key >= mid, entries [y, beam) have key < mid
      int x = a[u], y = b[u];
      const float* row = cv + (long)(tid + 256 * u) * beam;
      while (x < y) {
        const int m = (x + y) >> 1;
        if (fkey(row[m] + lp[u]) >= mid) x = m + 1; else y = m;
      }
      c[u] = x;
      mine += x;
    }
    const int total = block_count(mine, red);
    if (total >= beam) {
      lo = mid;
#pragma unroll
      for (int u = 0; u < 4; ++u) b[u] = c[u];
    } else {
      hi = mid - 1u;
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = c[u];
    }
  }
  // lo == hi == T: a = entries above T (all taken), b - a = entries equal to T
  int mine = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    scan[tid + 256 * u] = b[u] - a[u];
    mine += a[u];
  }
  const int need = beam - block_count(mine, red);
  block_excl_scan_1024(scan, red);
  int take[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int left = need - scan[tid + 256 * u];
    const int eq = b[u] - a[u];
    take[u] = a[u] + (left <= 0 ? 0 : (left < eq ? left : eq));
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) scan[tid + 256 * u] = take[u];
  block_excl_scan_1024(scan, red);  // first slot of every parent's prefix
  const int P = pow2_at_least(beam);
  for (int q = tid; q < P; q += 256) {
    unsigned long long s = 0ull;
    if (q < beam) {
      int x = 0, y = beam_prev - 1;  // the last parent whose first slot is <= q
      while (x < y) {
        const int m = (x + y + 1) >> 1;
        if (scan[m] <= q) x = m; else y = m - 1;
      }
      const int j = q - scan[x];  // < beam, whatever the lists held
      const float v = cv[(long)x * beam + j] + (lpn ? lpn[x] : 0.f);
      s = slot_of(fkey(v), x * beam + j);
    }
    slot[q] = s;
  }
  bitonic_desc(slot, P);
  const int* ci = cand_i + (long)n * beam_prev * beam;
  for (int j = tid; j < beam; j += 256) {
    const unsigned long long s = slot[j];
    const int idx = slot_idx(s);
    new_lp[(long)n * beam + j] = funkey(slot_key(s));
    new_tok[(long)n * beam + j] = ci[idx];
    new_bp[(long)n * beam + j] = idx / beam;
  }
}

// ---------------------------------------------------------------------------
// per-row top-k, 2 <= k <= 1024
// ---------------------------------------------------------------------------
// The tail both row kernels share: `above` winners (key > T) already sit in
// slot[0..above) in any order, the ties have been appended behind them in
// index order; pad, sort, write.
__device__ inline void finish_row(unsigned long long* slot, int k,
                                  float* __restrict__ out_v, int* __restrict__ out_i) {
  const int P = pow2_at_least(k);
  for (int q = k + threadIdx.x; q < P; q += 256) slot[q] = 0ull;
  bitonic_desc(slot, P);
  for (int j = threadIdx.x; j < k; j += 256) {
    const unsigned long long s = slot[j];
    out_v[j] = funkey(slot_key(s));
    out_i[j] = slot_idx(s);
  }
}

// allennlp's forced distribution of a finished row (0 at stop, finfo.min elsewhere)
__device__ inline void forced_row(int k, int stop, float* __restrict__ out_v,
                                  int* __restrict__ out_i) {
  for (int j = threadIdx.x; j < k; j += 256) {
    out_v[j] = j == 0 ? 0.f : kFloatMin;
    out_i[j] = j == 0 ? stop : (j - 1 < stop ? j - 1 : j);
  }
}

// V <= 24 * 256: the row stays in registers, as in row_select_reg_kernel, whose
// float operations for pred these are.
__global__ __launch_bounds__(256) void row_select_wide_reg_kernel(
    const float* __restrict__ logits, const float* __restrict__ lm_logits,
    float lambda, int V, int k, const int64_t* __restrict__ last_tok, int stop,
    float* __restrict__ cand_v, int* __restrict__ cand_i) {
  __shared__ unsigned long long slot[kWideSlots];
  __shared__ unsigned bitmap[kRowRegs * 8];  // one bit per column: key == T
  __shared__ int pre[kRowRegs * 8];
  __shared__ float red[8];
  __shared__ int redi[4];
  __shared__ unsigned above;
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)r * V;
  float p[kRowRegs];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < kRowRegs; ++j) {
    const int i = tid + 256 * j;
    p[j] = i < V ? x[i] : -INFINITY;
    mx = fmaxf(mx, p[j]);
  }
  mx = block_max(mx, red);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kRowRegs; ++j)
    if (tid + 256 * j < V) s += expf(p[j] - mx);
  s = block_sum(s, red);
  const float ls = logf(s);
  if (lm_logits) {
    const float* y = lm_logits + (long)r * V;
    float q[kRowRegs];
    float my = -INFINITY;
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j) {
      const int i = tid + 256 * j;
      q[j] = i < V ? y[i] : -INFINITY;
      my = fmaxf(my, q[j]);
    }
    my = block_max(my, red);
    float sy = 0.f;
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j)
      if (tid + 256 * j < V) sy += expf(q[j] - my);
    sy = block_sum(sy, red);
    const float lsy = logf(sy);
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j)
      p[j] = ((p[j] - mx) - ls) - lambda * ((q[j] - my) - lsy);
  } else {
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j) p[j] = (p[j] - mx) - ls;
  }
  float* out_v = cand_v + (long)r * k;
  int* out_i = cand_i + (long)r * k;
  if (last_tok && last_tok[r] == stop) {  // block-uniform
    forced_row(k, stop, out_v, out_i);
    return;
  }
  unsigned key[kRowRegs];
  unsigned kmax = 0u, kmin = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < kRowRegs; ++j) {
    const bool ok = tid + 256 * j < V;
    key[j] = ok ? fkey(p[j]) : 0u;  // below every real key
    if (ok) { kmax = max(kmax, key[j]); kmin = min(kmin, key[j]); }
  }
  unsigned hi = block_umax(kmax, redi);
  unsigned lo = block_umin(kmin, redi);
  // largest T with count(key >= T) >= k   (count(key >= lo) = V >= k)
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);
    int c = 0;
#pragma unroll
    for (int j = 0; j < kRowRegs; ++j) c += key[j] >= mid;
    if (block_count(c, redi) >= k) lo = mid; else hi = mid - 1u;
  }
  const unsigned T = lo;  // > 0: padding keys never reach it
  if (tid == 0) above = 0u;
  if (tid < kRowRegs * 8) bitmap[tid] = 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowRegs; ++j) {
    const int i = tid + 256 * j;
    if (key[j] > T) {
      slot[atomicAdd(&above, 1u)] = slot_of(key[j], i);  // fewer than k of them
    } else if (key[j] == T) {
      atomicOr(&bitmap[i >> 5], 1u << (i & 31));
    }
  }
  __syncthreads();
  // ties: the k - above lowest columns, ranked through the bitmap's prefix counts
  const int ngt = (int)above;
  const int words = tid < kRowRegs * 8 ? __popc(bitmap[tid]) : 0;
  const int before = block_excl_scan(words, redi);
  if (tid < kRowRegs * 8) pre[tid] = before;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowRegs; ++j) {
    const int i = tid + 256 * j;
    if (key[j] == T) {
      const int rank = pre[i >> 5] + __popc(bitmap[i >> 5] & ((1u << (i & 31)) - 1u));
      if (ngt + rank < k) slot[ngt + rank] = slot_of(T, i);
    }
  }
  finish_row(slot, k, out_v, out_i);
}

// Larger vocabularies: the row lives in LDS, as in row_select_kernel, whose float
// operations for pred these are.  Dynamic LDS: V floats.
__global__ __launch_bounds__(256) void row_select_wide_kernel(
    const float* __restrict__ logits, const float* __restrict__ lm_logits,
    float lambda, int V, int k, const int64_t* __restrict__ last_tok, int stop,
    float* __restrict__ cand_v, int* __restrict__ cand_i) {
  extern __shared__ __attribute__((aligned(16))) float pred[];  // [V]
  __shared__ unsigned long long slot[kWideSlots];
  __shared__ float red[8];
  __shared__ int redi[4];
  __shared__ unsigned above;
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)r * V;
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 256) { const float v = x[i]; pred[i] = v; mx = fmaxf(mx, v); }
  mx = block_max(mx, red);
  float s = 0.f;
  for (int i = tid; i < V; i += 256) s += expf(pred[i] - mx);
  s = block_sum(s, red);
  const float ls = logf(s);
  if (lm_logits) {
    const float* y = lm_logits + (long)r * V;
    float my = -INFINITY;
    for (int i = tid; i < V; i += 256) my = fmaxf(my, y[i]);
    my = block_max(my, red);
    float sy = 0.f;
    for (int i = tid; i < V; i += 256) sy += expf(y[i] - my);
    sy = block_sum(sy, red);
    const float lsy = logf(sy);
    for (int i = tid; i < V; i += 256)
      pred[i] = ((pred[i] - mx) - ls) - lambda * ((y[i] - my) - lsy);
  } else {
    for (int i = tid; i < V; i += 256) pred[i] = (pred[i] - mx) - ls;
  }
  float* out_v = cand_v + (long)r * k;
  int* out_i = cand_i + (long)r * k;
  if (last_tok && last_tok[r] == stop) {  // block-uniform
    forced_row(k, stop, out_v, out_i);
    return;
  }
  __syncthreads();
  unsigned lo = 0u, hi = 0xFFFFFFFFu;  // count(key >= lo) = V >= k
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);
    int c = 0;
    for (int i = tid; i < V; i += 256) c += fkey(pred[i]) >= mid;
    if (block_count(c, redi) >= k) lo = mid; else hi = mid - 1u;
  }
  const unsigned T = lo;
  if (tid == 0) above = 0u;
  __syncthreads();
  // thread t owns the columns [t * span, (t + 1) * span): its ties are ranked behind
  // those of the threads before it
  const int span = (V + 255) / 256;
  const int i0 = tid * span < V ? tid * span : V;
  const int i1 = i0 + span < V ? i0 + span : V;
  int ties = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned key = fkey(pred[i]);
    if (key > T) slot[atomicAdd(&above, 1u)] = slot_of(key, i);  // fewer than k of them
    else ties += key == T;
  }
  int rank = block_excl_scan(ties, redi);  // (its barriers publish `above`)
  const int ngt = (int)above;
  for (int i = i0; i < i1 && ngt + rank < k; ++i)
    if (fkey(pred[i]) == T) { slot[ngt + rank] = slot_of(T, i); ++rank; }
  finish_row(slot, k, out_v, out_i);
}

}  // namespace

int launch_beam_merge_wide(const float* cand_v, const int* cand_i,
                           const float* last_lp, int n, int beam_prev, int beam,
                           float* new_lp, int* new_tok, int* new_bp,
                           hipStream_t s) {
  MILAN_REQUIRE(n > 0 && beam >= 1 && beam <= kWideSlots && beam_prev >= 1 &&
                    beam_prev <= kWideSlots,
                MILAN_ERR_ARG,
                "beam merge: beam_size=%d (previous step %d) must be in 1..%d", beam,
                beam_prev, kWideSlots);
  hipLaunchKernelGGL(beam_merge_wide_kernel, dim3(n), dim3(256), 0, s, cand_v,
                     cand_i, last_lp, beam_prev, beam, new_lp, new_tok, new_bp);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

bool row_select_wide_ok(int V, int k) {
  return k >= 2 && k <= kWideSlots && k <= V &&
         sizeof(float) * (size_t)V + 16 * 1024 <= 160 * 1024;
}

int launch_row_select_wide(const float* logits, const float* lm_logits,
                           float lambda, int rows, int V, int k,
                           const int64_t* last_tok, int stop, float* cand_v,
                           int* cand_i, hipStream_t s) {
  MILAN_REQUIRE(k >= 2 && k <= kWideSlots && k <= V, MILAN_ERR_ARG,
                "row select: beam_size=%d must be in 2..min(%d, vocab_size %d)", k,
                kWideSlots, V);
  if (V <= kRowRegs * 256) {
    hipLaunchKernelGGL(row_select_wide_reg_kernel, dim3(rows), dim3(256), 0, s,
                       logits, lm_logits, lambda, V, k, last_tok, stop, cand_v,
                       cand_i);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const size_t lds = sizeof(float) * (size_t)V;  // + 8.1 KB static
  MILAN_REQUIRE(lds + 16 * 1024 <= 160 * 1024, MILAN_ERR_SHAPE,
                "vocab_size %d too large for the wide row-select kernel", V);
  if (lds + 16 * 1024 > 64 * 1024)
    MILAN_TRY(ensure_lds_attr(reinterpret_cast<const void*>(row_select_wide_kernel), (int)lds));
  hipLaunchKernelGGL(row_select_wide_kernel, dim3(rows), dim3(256), lds, s, logits,
                     lm_logits, lambda, V, k, last_tok, stop, cand_v, cand_i);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace milan
