// LanguageModel training (src/milan/lms.py:134-265): the loss, forward and backward of
// Embedding -> nn.LSTM(E, H, layers, dropout) -> Linear(H, V) -> LogSoftmax -> NLLLoss
// (ignore_index = pad) over a padded (rows, L) batch.
//
// Precision: every contraction here is the exact fp32 MFMA (v_mfma_f32_16x16x4_f32),
// whatever milan_set_precision says.  The split-f16 mode, its status word and its range
// guards were built for inference activations; gradients span many more decades and are
// not guarded, so training never uses them.
//
// The kernels read the caller's raw fp32 parameters, row-major in torch layout, on every
// call (the optimizer rewrites them after every step): the packed arena of
// milan_finalize_weights is neither needed nor touched.  No weight is transposed or
// packed either: the one GEMM kernel below (tgemm_kernel) reads both operands through
// strided views and stages either orientation into LDS, so X.W^T, dG^T.X and dG.W are the
// same kernel with different views.
//
// Determinism: every output element is reduced in a fixed order.  Split-K GEMMs write
// their partial sums to the workspace and a combine kernel adds them in split order; the
// column sums (bias gradients) and the embedding gradient are ordered loops; the loss
// reduction is one workgroup.  No float atomics: two calls with the same inputs and seed
// give identical bits.
#include "train_common.h"

namespace milan {
namespace lmt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// C(m, n) = sum_k A(m, k) B(k, n) [+ D(m, n)] [+ bias1[n]] [+ bias2[n]]
//   ta = 0: A(m, k) = a(m, k);  ta = 1: A(m, k) = a(k, m)
//   tb = 0: B(k, n) = b(k, n);  tb = 1: B(k, n) = b(n, k)
struct GemmArgs {
  View a, b, c, d;  // d.p == nullptr: no addend (d may alias c)
  int ta, tb;
  int M, N, K;
  int kchunk;   // K range of one split (multiple of BK)
  float* part;  // splits > 1: partial sums [split][M][N]
  const float* bias1;
  const float* bias2;
};

constexpr int BM = 64, BN = 64, BK = 32, LDP = 68;

// One K-tile of an operand, OP(x0 + xx, k0 + kk) for xx < 64, kk < BK, zero outside
// [0, xlim) x [k0, klim): fetched into 8 registers per lane, then stored to LDS as T[kk][xx].
// kmajor: OP(x, k) = v(k, x) (64 lanes walk x); else OP(x, k) = v(x, k) (32 lanes walk k).
__device__ __forceinline__ void fetch_tile(const View& v, int kmajor, int x0, int xlim, int k0,
                                           int klim, float (&r)[8], int tid) {
  if (kmajor) {
    const int x = x0 + (tid & 63);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + (tid >> 6) + 4 * j;
      r[j] = 0.f;
      if (x < xlim && k < klim) r[j] = v.p[voff(v, k) + x];
    }
  } else {
    const int k = k0 + (tid & 31);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int x = x0 + (tid >> 5) + 8 * j;
      r[j] = 0.f;
      if (x < xlim && k < klim) r[j] = v.p[voff(v, x) + k];
    }
  }
}
__device__ __forceinline__ void store_tile(int kmajor, const float (&r)[8], float (*T)[LDP],
                                           int tid) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (kmajor)
      T[(tid >> 6) + 4 * j][tid & 63] = r[j];
    else
      T[tid & 31][(tid >> 5) + 8 * j] = r[j];
  }
}

__device__ __forceinline__ float epilogue(const GemmArgs& g, int m, int n, float acc) {
  if (g.d.p) acc += g.d.p[voff(g.d, m) + n];
  if (g.bias1) acc += g.bias1[n];
  if (g.bias2) acc += g.bias2[n];
  return acc;
}

// 64 x 64 output tile per workgroup, four waves of 32 x 32 (2 x 2 MFMA 16x16x4 tiles).
__global__ __launch_bounds__(256) void tgemm_kernel(GemmArgs g) {
  __shared__ float As[BK][LDP], Bs[BK][LDP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = blockIdx.z * g.kchunk;
  const int ke = min(g.K, kb + g.kchunk);
  const int wm = (w & 1) * 32, wn = (w >> 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the next K-tile's global loads are in flight while this one's MFMAs run
  float ra[8], rb[8];
  fetch_tile(g.a, g.ta, m0, g.M, kb, ke, ra, tid);
  fetch_tile(g.b, !g.tb, n0, g.N, kb, ke, rb, tid);
  for (int k0 = kb; k0 < ke; k0 += BK) {
    store_tile(g.ta, ra, As, tid);
    store_tile(!g.tb, rb, Bs, tid);
    __syncthreads();
    if (k0 + BK < ke) {
      fetch_tile(g.a, g.ta, m0, g.M, k0 + BK, ke, ra, tid);
      fetch_tile(g.b, !g.tb, n0, g.N, k0 + BK, ke, rb, tid);
    }
#pragma unroll
    for (int ks = 0; ks < BK; ks += 4) {
      const float a0 = As[ks + lk][wm + lr], a1 = As[ks + lk][wm + 16 + lr];
      const float b0 = Bs[ks + lk][wn + lr], b1 = Bs[ks + lk][wn + 16 + lr];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D map of the 16x16 f32 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + lk * 4 + r, n = n0 + wn + 16 * j + lr;
        if (m >= g.M || n >= g.N) continue;
        if (g.part) {
          g.part[((long)blockIdx.z * g.M + m) * g.N + n] = acc[i][j][r];
        } else {
          float* c = const_cast<float*>(g.c.p);
          c[voff(g.c, m) + n] = epilogue(g, m, n, acc[i][j][r]);
        }
      }
}

// Split-K combine: the partial sums in split order, then the epilogue.
__global__ void combine_kernel(GemmArgs g, int splits) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)g.M * g.N) return;
  const int m = (int)(i / g.N), n = (int)(i % g.N);
  float s = g.part[i];
  for (int z = 1; z < splits; ++z) s += g.part[(long)z * g.M * g.N + i];
  float* c = const_cast<float*>(g.c.p);
  c[voff(g.c, m) + n] = epilogue(g, m, n, s);
}

// Splits of K: enough workgroups to cover the CUs, at least 128 of K per split.  A
// function of the shape alone, so the summation order is too.
static int plan_splits(int M, int N, int K, int* kchunk) {
  const long tiles = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int s = 1;
  while (s < 16 && tiles * s < 512 && K / (2 * s) >= 128) s *= 2;
  int kc = (K + s - 1) / s;
  kc = (kc + BK - 1) / BK * BK;
  if (kc == 0) kc = BK;
  *kchunk = kc;
  return (K + kc - 1) / kc > 0 ? (K + kc - 1) / kc : 1;
}

size_t split_scratch_floats(int M, int N, int K) {
  int kc;
  const int s = plan_splits(M, N, K, &kc);
  return s > 1 ? (size_t)s * M * N : 0;
}

// Splits of K as a function of K alone (at least 256 of K per split, at most 8 splits): the
// bits of an output row then depend on that row of A and on B, not on how many rows the
// call has.
static int plan_splits_rows(int K, int* kchunk) {
  int s = 1;
  while (s < 8 && K / (2 * s) >= 256) s *= 2;
  int kc = (K + s - 1) / s;
  kc = (kc + BK - 1) / BK * BK;
  if (kc == 0) kc = BK;
  *kchunk = kc;
  return (K + kc - 1) / kc > 0 ? (K + kc - 1) / kc : 1;
}

size_t rows_scratch_floats(int M, int N, int K) {
  int kc;
  const int s = plan_splits_rows(K, &kc);
  return s > 1 ? (size_t)s * M * N : 0;
}

static int gemm_planned(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                        const float* bias2, int M, int N, int K, bool by_rows, Scratch sc,
                        hipStream_t s);

int gemm(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                const float* bias2, int M, int N, int K, Scratch sc, hipStream_t s) {
  return gemm_planned(a, ta, b, tb, c, d, bias1, bias2, M, N, K, false, sc, s);
}

int gemm_rows(View a, int ta, View b, int tb, View c, View d, const float* bias1,
              const float* bias2, int M, int N, int K, Scratch sc, hipStream_t s) {
  return gemm_planned(a, ta, b, tb, c, d, bias1, bias2, M, N, K, true, sc, s);
}

static int gemm_planned(View a, int ta, View b, int tb, View c, View d, const float* bias1,
                        const float* bias2, int M, int N, int K, bool by_rows, Scratch sc,
                        hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  GemmArgs g{a, b, c, d, ta, tb, M, N, K, 0, nullptr, bias1, bias2};
  const int splits = K <= 0 ? 1
                            : (by_rows ? plan_splits_rows(K, &g.kchunk)
                                       : plan_splits(M, N, K, &g.kchunk));
  if (K <= 0) g.kchunk = BK;
  if (splits > 1) {
    MILAN_REQUIRE((size_t)splits * M * N <= sc.floats, MILAN_ERR_WORKSPACE,
                  "lm train: split-K scratch too small (%d x %d x %d)", splits, M, N);
    g.part = sc.p;
  }
  dim3 grid((N + BN - 1) / BN, (M + BM - 1) / BM, splits);
  hipLaunchKernelGGL(tgemm_kernel, grid, dim3(256), 0, s, g);
  MILAN_CHECK_HIP(hipGetLastError());
  if (splits > 1) {
    const long total = (long)M * N;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       g, splits);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// ---- dropout mask: a pure function of (seed, layer, row, t, unit) ------------------------
// keep  <=>  (mix64(seed ^ mix64(key)) >> 40) >= thr,   thr = (uint32)(p * 2^24),
// key = layer << 56 | row << 32 | t << 16 | unit  (splitmix64 finaliser; restated on the
// host by milan_amd.lms.dropout_mask).
__device__ __forceinline__ bool keep(uint64_t seed, int layer, int row, int t, int unit,
                                     uint32_t thr) {
  const uint64_t key = (uint64_t)layer << 56 | (uint64_t)row << 32 | (uint64_t)t << 16 |
                       (uint64_t)unit;
  return (uint32_t)(mix64(seed ^ mix64(key)) >> 40) >= thr;
}

__device__ __forceinline__ int clamp_id(int64_t id, int V) {
  return id < 0 ? 0 : (id >= V ? V - 1 : (int)id);
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// X0[n][e] = embedding[inputs[n]][e]  (ids clamped into [0, V): memory safety only, the
// Python side validates them)
__global__ void embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb,
                             float* __restrict__ x, int N, int E, int V) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)N * E) return;
  const int n = (int)(i / E), e = (int)(i % E);
  x[i] = emb[(long)clamp_id(ids[n], V) * E + e];
}

// One LSTM cell step t (torch gate order i, f, g, o).  G: pre-activations of step t in,
// activated gates out; C: c_t [rows][L][H]; Hs: h_t at slot t + 1 of [rows][L + 1][H].
__global__ void cell_fwd_kernel(float* __restrict__ G, float* __restrict__ C,
                                float* __restrict__ Hs, int rows, int L, int H, int t) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const int b = (int)(i / H), j = (int)(i % H);
  float* g = G + ((long)b * L + t) * 4 * H;
  const float ig = sigm(g[j]), fg = sigm(g[H + j]), gg = tanhf(g[2 * H + j]),
              og = sigm(g[3 * H + j]);
  const float cp = t ? C[((long)b * L + t - 1) * H + j] : 0.f;
  const float c = fg * cp + ig * gg;
  g[j] = ig;
  g[H + j] = fg;
  g[2 * H + j] = gg;
  g[3 * H + j] = og;
  C[((long)b * L + t) * H + j] = c;
  Hs[((long)b * (L + 1) + t + 1) * H + j] = og * tanhf(c);
}

// Input of layer + 1 = dropout(h of `layer`): X[b][t][j] = h * mask * scale (p == 0: copy).
__global__ void dropout_fwd_kernel(const float* __restrict__ Hs, float* __restrict__ X,
                                   int rows, int L, int H, int layer, uint64_t seed,
                                   uint32_t thr, float scale) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * L * H) return;
  const int j = (int)(i % H);
  const long bt = i / H;
  const int t = (int)(bt % L), b = (int)(bt / L);
  float h = Hs[((long)b * (L + 1) + t + 1) * H + j];
  if (thr) h = keep(seed, layer, b, t, j, thr) ? h * scale : 0.f;
  X[i] = h;
}

// dY[b][t][j] *= mask * scale (the same mask as dropout_fwd_kernel)
__global__ void dropout_bwd_kernel(float* __restrict__ dY, int rows, int L, int H, int layer,
                                   uint64_t seed, uint32_t thr, float scale) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * L * H) return;
  const int j = (int)(i % H);
  const long bt = i / H;
  const int t = (int)(bt % L), b = (int)(bt / L);
  dY[i] = keep(seed, layer, b, t, j, thr) ? dY[i] * scale : 0.f;
}

// Deterministic block reductions (fixed tree over 256 threads).
__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, u) : v + u;
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
  return r;
}

// Per position: lse of the logits row, -log p(target) (0 for pad targets), valid flag.
__global__ __launch_bounds__(256) void nll_rows_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ tgt, int V,
                                                       int pad, float* __restrict__ lse,
                                                       float* __restrict__ term,
                                                       float* __restrict__ valid) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const float* x = logits + (long)n * V;
  float m = -INFINITY;
  for (int v = threadIdx.x; v < V; v += blockDim.x) m = fmaxf(m, x[v]);
  m = block_reduce(m, red, true);
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += blockDim.x) s += expf(x[v] - m);
  s = block_reduce(s, red, false);
  if (threadIdx.x == 0) {
    const float l = m + logf(s);
    const int64_t t = tgt[n];
    const bool ok = t != pad && t >= 0 && t < V;
    lse[n] = l;
    term[n] = ok ? l - x[t] : 0.f;
    valid[n] = ok ? 1.f : 0.f;
  }
}

// out[0] = sum of terms, out[1] = number of valid targets (one workgroup, fixed order)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ term,
                                                          const float* __restrict__ valid,
                                                          int N, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f, c = 0.f;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    s += term[n];
    c += valid[n];
  }
  s = block_reduce(s, red, false);
  c = block_reduce(c, red, false);
  if (threadIdx.x == 0) {
    out[0] = s;
    out[1] = c;
  }
}

// dlogits = (softmax - onehot(target)) * valid / n_valid, in place over the logits
__global__ __launch_bounds__(256) void dlogits_kernel(float* __restrict__ logits,
                                                      const int64_t* __restrict__ tgt,
                                                      const float* __restrict__ lse,
                                                      const float* __restrict__ valid,
                                                      const float* __restrict__ loss, int V) {
  const int n = blockIdx.x;
  float* x = logits + (long)n * V;
  const bool ok = valid[n] != 0.f;
  const float inv = ok ? 1.f / loss[1] : 0.f;
  const float l = lse[n];
  const int64_t t = tgt[n];
  for (int v = threadIdx.x; v < V; v += blockDim.x)
    x[v] = ok ? (expf(x[v] - l) - (v == t ? 1.f : 0.f)) * inv : 0.f;
}

// ---- the autograd pair (milan_lm_forward_train / milan_lm_backward) ------------------------
// out[n][v] = logits[n][v] - lse[n]
__global__ void lm_logprobs_kernel(const float* __restrict__ logits,
                                   const float* __restrict__ lse, float* __restrict__ out, int N,
                                   int V) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)N * V) return;
  out[i] = logits[i] - lse[i / V];
}

// picked[n] = logits[n][tgt[n]] - lse[n]: the log-prob of one token per position, without
// the [N][V] log-probs ever being written
__global__ void lm_picked_kernel(const float* __restrict__ logits,
                                 const int64_t* __restrict__ tgt, const float* __restrict__ lse,
                                 float* __restrict__ picked, int N, int V) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  picked[n] = logits[(long)n * V + clamp_id(tgt[n], V)] - lse[n];
}

// Log-softmax backward from upstream gradients of the log-probs, G [N][V], and of the picked
// log-probs, gp [N] (either null: zero), one workgroup per position:
//   g_v = G[n][v] + (v == tgt[n] ? gp[n] : 0)
//   logits[n][v] <- g_v - exp(logits[n][v] - lse[n]) * sum_v g_v
// in place, where backward() expects dlogits.  The row sum has one order whatever V is:
// thread i adds its elements v = i, i + 256, ... in increasing v, the 64 lanes of a wave by
// xor butterfly, the 4 waves in order.
__global__ __launch_bounds__(256) void lm_log_softmax_bwd_kernel(
    const float* __restrict__ G, const float* __restrict__ gp, const int64_t* __restrict__ tgt,
    float* __restrict__ logits, const float* __restrict__ lse, int V) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  float* x = logits + (long)n * V;
  const float* g = G ? G + (long)n * V : nullptr;
  const int t = gp ? clamp_id(tgt[n], V) : -1;
  const float dp = gp ? gp[n] : 0.f;
  float s = 0.f;
  if (g) {
    for (int v = tid; v < V; v += 256) s += v == t ? g[v] + dp : g[v];
  } else if (t >= 0 && (t & 255) == tid) {
    s = dp;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float sum = ((red[0] + red[1]) + red[2]) + red[3];
  const float l = lse[n];
  for (int v = tid; v < V; v += 256) {
    float gv = g ? g[v] : 0.f;
    if (v == t) gv += dp;
    x[v] = gv - expf(x[v] - l) * sum;
  }
}

// Column sums of X [R][N], stage 1: part[c][n] = sum over the rows of chunk c, in order.
__global__ void colsum_part_kernel(const float* __restrict__ X, int R, int N, int rchunk,
                                   float* __restrict__ part) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int r0 = blockIdx.y * rchunk, r1 = min(R, r0 + rchunk);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += X[(long)r * N + n];
  part[(long)blockIdx.y * N + n] = s;
}
// stage 2: out1[n] (= out2[n] when given) = sum of the chunks in order
__global__ void colsum_final_kernel(const float* __restrict__ part, int chunks, int N,
                                    float* __restrict__ out1, float* __restrict__ out2) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[(long)c * N + n];
  out1[n] = s;
  if (out2) out2[n] = s;
}

int colsum_chunks(int R) {
  const int c = (R + 63) / 64;
  return c < 1 ? 1 : (c > 64 ? 64 : c);
}

int colsum(const float* X, int R, int N, float* out1, float* out2, Scratch sc,
                  hipStream_t s) {
  const int chunks = colsum_chunks(R), rchunk = (R + chunks - 1) / chunks;
  MILAN_REQUIRE((size_t)chunks * N <= sc.floats, MILAN_ERR_WORKSPACE,
                "lm train: column-sum scratch too small");
  hipLaunchKernelGGL(colsum_part_kernel, dim3((N + 255) / 256, chunks), dim3(256), 0, s, X, R,
                     N, rchunk, sc.p);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, s, sc.p, chunks,
                     N, out1, out2);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Backward of cell step t.  dh: dL/dh_t (row stride dh_rs); G: activated gates of step t
// in, d(pre-activation) out; dc: dL/dc_t in (ignored at t = L - 1), dL/dc_{t-1} out.
__global__ void cell_bwd_kernel(const float* __restrict__ dh, long dh_rs, float* __restrict__ G,
                                const float* __restrict__ C, float* __restrict__ dc, int rows,
                                int L, int H, int t) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const int b = (int)(i / H), j = (int)(i % H);
  float* g = G + ((long)b * L + t) * 4 * H;
  const float ig = g[j], fg = g[H + j], gg = g[2 * H + j], og = g[3 * H + j];
  const float c = C[((long)b * L + t) * H + j];
  const float cp = t ? C[((long)b * L + t - 1) * H + j] : 0.f;
  const float d_h = dh[(long)b * dh_rs + j];
  const float tc = tanhf(c);
  const float dcur = d_h * og * (1.f - tc * tc) + (t == L - 1 ? 0.f : dc[i]);
  dc[i] = dcur * fg;
  g[j] = dcur * gg * ig * (1.f - ig);
  g[H + j] = dcur * cp * fg * (1.f - fg);
  g[2 * H + j] = dcur * ig * (1.f - gg * gg);
  g[3 * H + j] = d_h * tc * og * (1.f - og);
}

// dEmbedding[v] = sum over positions n with inputs[n] == v of dX0[n], in position order;
// the padding row is exactly zero.  One workgroup per token id: each pass compacts the
// matching positions of 256 ids into LDS (wave ballots, order kept), then every lane adds
// its column of those rows.
__global__ __launch_bounds__(256) void embed_grad_kernel(const int64_t* __restrict__ ids,
                                                         const float* __restrict__ dX, int N,
                                                         int E, int V, int pad,
                                                         float* __restrict__ dEmb) {
  __shared__ int list[256];
  __shared__ int wave_count[4];
  const int v = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int e0 = 0; e0 < E; e0 += blockDim.x) {
    const int e = e0 + threadIdx.x;
    float s = 0.f;
    for (int n0 = 0; n0 < N && v != pad; n0 += 256) {
      const int n = n0 + threadIdx.x;
      const bool hit = n < N && clamp_id(ids[n], V) == v;
      const uint64_t mask = __ballot(hit);
      if (lane == 0) wave_count[w] = __popcll(mask);
      __syncthreads();
      int base = 0, total = 0;
      for (int k = 0; k < 4; ++k) {
        base += k < w ? wave_count[k] : 0;
        total += wave_count[k];
      }
      if (hit) list[base + __popcll(mask & ((1ull << lane) - 1))] = n;
      __syncthreads();
      if (e < E)
        for (int k = 0; k < total; ++k) s += dX[(long)list[k] * E + e];
      __syncthreads();
    }
    if (e < E) dEmb[(long)v * E + e] = s;
  }
}

static unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

// ---- workspace layout -------------------------------------------------------------------
struct Plan {
  int V, E, H, NL, pad, rows, L, N;
  size_t x0, xin[8], gates[8], cst[8], hs[8];  // per-layer float offsets
  size_t logits, lse, term, valid, dy, dhrec, dc, scratch, scratch_floats, total;
  size_t terms, grad_total;  // after `total`: what the autograd pair adds
};

static int make_plan(const milan_ctx* c, int rows, int L, Plan* p) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "lm train: null ctx");
  const milan_dims& d = c->d;
  MILAN_REQUIRE(d.has_lm, MILAN_ERR_NO_LM, "lm train: the context has no language model");
  MILAN_REQUIRE(d.lm_layers >= 1 && d.lm_layers <= 8, MILAN_ERR_SHAPE,
                "lm train: 1..8 layers supported, got %d", d.lm_layers);
  MILAN_REQUIRE(rows > 0 && L > 0 && rows < (1 << 24) && L < (1 << 16), MILAN_ERR_SHAPE,
                "lm train: need 0 < rows < 2^24 and 0 < L < 2^16 (rows %d, L %d)", rows, L);
  MILAN_REQUIRE((long)rows * L < (1L << 30), MILAN_ERR_SHAPE, "lm train: batch too large");
  MILAN_REQUIRE(d.lm_hidden_size < (1 << 14), MILAN_ERR_SHAPE, "lm train: hidden size too large");
  p->V = d.vocab_size;
  p->E = d.lm_embedding_size;
  p->H = d.lm_hidden_size;
  p->NL = d.lm_layers;
  p->pad = d.pad_index;
  p->rows = rows;
  p->L = L;
  const int N = p->N = rows * L, H = p->H, E = p->E, V = p->V;
  size_t off = 0;
  auto take = [&](size_t floats) {
    const size_t at = off;
    off += (floats + 63) / 64 * 64;
    return at;
  };
  p->x0 = take((size_t)N * E);
  for (int l = 0; l < p->NL; ++l) {
    p->xin[l] = l ? take((size_t)N * H) : p->x0;
    p->gates[l] = take((size_t)N * 4 * H);
    p->cst[l] = take((size_t)N * H);
    p->hs[l] = take((size_t)rows * (L + 1) * H);
  }
  p->logits = take((size_t)N * V);
  p->lse = take(N);
  p->term = take(N);
  p->valid = take(N);
  p->dy = take((size_t)N * (H > E ? H : E));
  p->dhrec = take((size_t)rows * H);
  p->dc = take((size_t)rows * H);
  size_t sc = 0;
  auto need = [&](size_t f) { sc = f > sc ? f : sc; };
  need((size_t)colsum_chunks(N) * (V > 4 * H ? V : 4 * H));
  need(split_scratch_floats(N, V, H));      // logits
  need(split_scratch_floats(V, H, N));      // dW_out
  need(split_scratch_floats(N, H, V));      // dH of the top layer
  for (int l = 0; l < p->NL; ++l) {
    const int in = l ? H : E;
    need(split_scratch_floats(N, 4 * H, in));    // input projection
    need(split_scratch_floats(rows, 4 * H, H));  // recurrent step
    need(split_scratch_floats(rows, H, 4 * H));  // dh_{t-1}
    need(split_scratch_floats(4 * H, H, N));     // dW_hh
    need(split_scratch_floats(4 * H, in, N));    // dW_ih
    need(split_scratch_floats(N, in, 4 * H));    // dX
  }
  p->scratch = take(sc);
  p->scratch_floats = sc;
  p->total = off * sizeof(float);
  // after `total`, what the autograd pair (milan_lm_forward_train / _backward) adds: the
  // forward's loss terms, which nobody reads (the backward overwrites activations in place
  // and needs no buffer of its own)
  p->terms = take(2);
  p->grad_total = off * sizeof(float);
  return 0;
}

struct Params {
  const float *emb, *w_ih[8], *w_hh[8], *b_ih[8], *b_hh[8], *w_out, *b_out;
};

static int unpack(const Plan& p, const float* const* params, int n, Params* o) {
  MILAN_REQUIRE(params, MILAN_ERR_ARG, "lm train: null parameter list");
  MILAN_REQUIRE(n == 3 + 4 * p.NL, MILAN_ERR_ARG,
                "lm train: %d parameter pointers given, LanguageModel.state_dict() of %d layers "
                "has %d", n, p.NL, 3 + 4 * p.NL);
  for (int i = 0; i < n; ++i)
    MILAN_REQUIRE(params[i], MILAN_ERR_ARG, "lm train: parameter %d is null", i);
  o->emb = params[0];
  for (int l = 0; l < p.NL; ++l) {
    o->w_ih[l] = params[1 + 4 * l];
    o->w_hh[l] = params[2 + 4 * l];
    o->b_ih[l] = params[3 + 4 * l];
    o->b_hh[l] = params[4 + 4 * l];
  }
  o->w_out = params[1 + 4 * p.NL];
  o->b_out = params[2 + 4 * p.NL];
  return 0;
}

static uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 16777216.0); }

// Forward (+ loss).  train: dropout between layers with (p, seed).
static int forward(const Plan& p, const Params& w, float* ws, const int64_t* inputs,
                   const int64_t* targets, float p_drop, uint64_t seed, float* loss,
                   hipStream_t s) {
  const int N = p.N, H = p.H, E = p.E, V = p.V, rows = p.rows, L = p.L;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  const uint32_t thr = drop_threshold(p_drop);
  const float scale = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  hipLaunchKernelGGL(embed_kernel, dim3(blocks_for((long)N * E)), dim3(256), 0, s, inputs, w.emb,
                     ws + p.x0, N, E, V);
  for (int l = 0; l < p.NL; ++l) {
    const int in = l ? H : E;
    float* G = ws + p.gates[l];
    float* C = ws + p.cst[l];
    float* Hs = ws + p.hs[l];
    MILAN_CHECK_HIP(hipMemsetAsync(Hs, 0, sizeof(float) * rows * (L + 1) * H, s));
    if (l) {
      hipLaunchKernelGGL(dropout_fwd_kernel, dim3(blocks_for((long)N * H)), dim3(256), 0, s,
                         ws + p.hs[l - 1], ws + p.xin[l], rows, L, H, l - 1, seed, thr, scale);
    }
    // pre-activations of every position: X . W_ih^T + b_ih + b_hh
    MILAN_TRY(gemm(view(ws + p.xin[l], in), 0, view(w.w_ih[l], in), 1, view(G, 4 * H), none,
                   w.b_ih[l], w.b_hh[l], N, 4 * H, in, sc, s));
    for (int t = 0; t < L; ++t) {
      if (t) {  // += h_{t-1} . W_hh^T  (h_{t-1} = slot t of Hs)
        const View g = view(G + (size_t)t * 4 * H, (long)L * 4 * H);
        MILAN_TRY(gemm(view(Hs + (size_t)t * H, (long)(L + 1) * H), 0, view(w.w_hh[l], H), 1, g,
                       g, nullptr, nullptr, rows, 4 * H, H, sc, s));
      }
      hipLaunchKernelGGL(cell_fwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, G,
                         C, Hs, rows, L, H, t);
    }
  }
  // logits of every position (top layer, no dropout on its output)
  const View htop = view(ws + p.hs[p.NL - 1] + H, H, L, (long)(L + 1) * H);
  MILAN_TRY(gemm(htop, 0, view(w.w_out, H), 1, view(ws + p.logits, V), none, w.b_out, nullptr,
                 N, V, H, sc, s));
  hipLaunchKernelGGL(nll_rows_kernel, dim3(N), dim3(256), 0, s, ws + p.logits, targets, V, p.pad,
                     ws + p.lse, ws + p.term, ws + p.valid);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, ws + p.term, ws + p.valid, N,
                     loss);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

struct Grads {
  float *emb, *w_ih[8], *w_hh[8], *b_ih[8], *b_hh[8], *w_out, *b_out;
};

static int unpack_grads(const Plan& p, float* const* grads, int n, Grads* g) {
  Params gp;
  MILAN_TRY(unpack(p, (const float* const*)grads, n, &gp));
  g->emb = const_cast<float*>(gp.emb);
  for (int l = 0; l < p.NL; ++l) {
    g->w_ih[l] = const_cast<float*>(gp.w_ih[l]);
    g->w_hh[l] = const_cast<float*>(gp.w_hh[l]);
    g->b_ih[l] = const_cast<float*>(gp.b_ih[l]);
    g->b_hh[l] = const_cast<float*>(gp.b_hh[l]);
  }
  g->w_out = const_cast<float*>(gp.w_out);
  g->b_out = const_cast<float*>(gp.b_out);
  return 0;
}

static int backward(const Plan& p, const Params& w, const Grads& gr, float* ws,
                    const int64_t* inputs, const int64_t* targets, float p_drop, uint64_t seed,
                    const float* loss, hipStream_t s) {
  const int N = p.N, H = p.H, E = p.E, V = p.V, rows = p.rows, L = p.L;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  const uint32_t thr = drop_threshold(p_drop);
  const float scale = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  float* dlog = ws + p.logits;
  if (loss)  // (null: the logits buffer already holds dlogits, milan_lm_backward)
    hipLaunchKernelGGL(dlogits_kernel, dim3(N), dim3(256), 0, s, dlog, targets, ws + p.lse,
                       ws + p.valid, loss, V);
  const View htop = view(ws + p.hs[p.NL - 1] + H, H, L, (long)(L + 1) * H);
  // dW_out = dlogits^T . H,  db_out = sum dlogits,  dH = dlogits . W_out
  MILAN_TRY(gemm(view(dlog, V), 1, htop, 0, view(gr.w_out, H), none, nullptr, nullptr, V, H, N,
                 sc, s));
  MILAN_TRY(colsum(dlog, N, V, gr.b_out, nullptr, sc, s));
  float* dY = ws + p.dy;
  MILAN_TRY(gemm(view(dlog, V), 0, view(w.w_out, H), 0, view(dY, H), none, nullptr, nullptr, N,
                 H, V, sc, s));
  float* dh = ws + p.dhrec;
  float* dc = ws + p.dc;
  for (int l = p.NL - 1; l >= 0; --l) {
    const int in = l ? H : E;
    float* G = ws + p.gates[l];
    const float* C = ws + p.cst[l];
    const float* Hs = ws + p.hs[l];
    for (int t = L - 1; t >= 0; --t) {
      const float* dht = t == L - 1 ? dY + (size_t)t * H : dh;
      const long rs = t == L - 1 ? (long)L * H : H;
      hipLaunchKernelGGL(cell_bwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, dht,
                         rs, G, C, dc, rows, L, H, t);
      if (t) {  // dL/dh_{t-1} = dY[:, t-1] + dG_t . W_hh
        MILAN_TRY(gemm(view(G + (size_t)t * 4 * H, (long)L * 4 * H), 0, view(w.w_hh[l], H), 0,
                       view(dh, H), view(dY + (size_t)(t - 1) * H, (long)L * H), nullptr,
                       nullptr, rows, H, 4 * H, sc, s));
      }
    }
    // dW_hh = sum_t dG_t^T h_{t-1} (h_{-1} = 0 in slot 0), dW_ih = dG^T X, biases, dX
    MILAN_TRY(gemm(view(G, 4 * H), 1, view(Hs, H, L, (long)(L + 1) * H), 0, view(gr.w_hh[l], H),
                   none, nullptr, nullptr, 4 * H, H, N, sc, s));
    MILAN_TRY(gemm(view(G, 4 * H), 1, view(ws + p.xin[l], in), 0, view(gr.w_ih[l], in), none,
                   nullptr, nullptr, 4 * H, in, N, sc, s));
    MILAN_TRY(colsum(G, N, 4 * H, gr.b_ih[l], gr.b_hh[l], sc, s));
    MILAN_TRY(gemm(view(G, 4 * H), 0, view(w.w_ih[l], in), 0, view(dY, in), none, nullptr,
                   nullptr, N, in, 4 * H, sc, s));
    if (l && thr)
      hipLaunchKernelGGL(dropout_bwd_kernel, dim3(blocks_for((long)N * H)), dim3(256), 0, s, dY,
                         rows, L, H, l - 1, seed, thr, scale);
  }
  hipLaunchKernelGGL(embed_grad_kernel, dim3(V), dim3(256), 0, s, inputs, dY, N, E, V, p.pad,
                     gr.emb);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// host launchers of the kernels above, for decoder_train.hip (train_common.h)
void launch_nll_rows(const float* logits, const int64_t* tgt, int N, int V, int pad, float* lse,
                     float* term, float* valid, hipStream_t s) {
  hipLaunchKernelGGL(nll_rows_kernel, dim3(N), dim3(256), 0, s, logits, tgt, V, pad, lse, term,
                     valid);
}
void launch_loss_reduce(const float* term, const float* valid, int N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, term, valid, N, out);
}
void launch_dlogits(float* logits, const int64_t* tgt, const float* lse, const float* valid,
                    const float* loss, int N, int V, hipStream_t s) {
  hipLaunchKernelGGL(dlogits_kernel, dim3(N), dim3(256), 0, s, logits, tgt, lse, valid, loss, V);
}
void launch_embed_grad(const int64_t* ids, const float* dX, int N, int E, int V, int pad,
                       float* dEmb, hipStream_t s) {
  hipLaunchKernelGGL(embed_grad_kernel, dim3(V), dim3(256), 0, s, ids, dX, N, E, V, pad, dEmb);
}

}  // namespace lmt
}  // namespace milan

using namespace milan;
using namespace milan::lmt;

extern "C" {

size_t milan_lm_train_workspace_bytes(const milan_ctx* c, int rows, int L) {
  Plan p;
  if (make_plan(c, rows, L, &p) != 0) return 0;
  return p.total;
}

int milan_lm_nll(milan_ctx* c, const float* const* params, int n_params, const int64_t* inputs,
                 const int64_t* targets, int rows, int L, float* loss_sum_and_count, void* ws,
                 size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(inputs && targets && loss_sum_and_count && ws, MILAN_ERR_ARG,
                "milan_lm_nll: null argument");
  Plan p;
  MILAN_TRY(make_plan(c, rows, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.total, MILAN_ERR_WORKSPACE,
                "milan_lm_nll: workspace %zu < %zu bytes", ws_bytes, p.total);
  Params w;
  MILAN_TRY(unpack(p, params, n_params, &w));
  return forward(p, w, (float*)ws, inputs, targets, 0.f, 0, loss_sum_and_count,
                 (hipStream_t)stream);
}

int milan_lm_train_step(milan_ctx* c, const float* const* params, float* const* grads,
                        int n_params, const int64_t* inputs, const int64_t* targets, int rows,
                        int L, float dropout, uint64_t seed, float* loss_sum_and_count, void* ws,
                        size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(grads && inputs && targets && loss_sum_and_count && ws, MILAN_ERR_ARG,
                "milan_lm_train_step: null argument");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_lm_train_step: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.total, MILAN_ERR_WORKSPACE,
                "milan_lm_train_step: workspace %zu < %zu bytes", ws_bytes, p.total);
  Params w;
  MILAN_TRY(unpack(p, params, n_params, &w));
  Grads g;
  MILAN_TRY(unpack_grads(p, grads, n_params, &g));
  const hipStream_t s = (hipStream_t)stream;
  MILAN_TRY(forward(p, w, (float*)ws, inputs, targets, dropout, seed, loss_sum_and_count, s));
  return backward(p, w, g, (float*)ws, inputs, targets, dropout, seed, loss_sum_and_count, s);
}

size_t milan_lm_grad_workspace_bytes(const milan_ctx* c, int rows, int L) {
  Plan p;
  if (make_plan(c, rows, L, &p) != 0) return 0;
  return p.grad_total;
}

int milan_lm_forward_train(milan_ctx* c, const float* const* params, int n_params,
                           const int64_t* inputs, int rows, int L, float dropout, uint64_t seed,
                           float* logprobs_out, float* picked_out, const int64_t* targets,
                           void* ws, size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(inputs && ws, MILAN_ERR_ARG, "milan_lm_forward_train: null argument");
  MILAN_REQUIRE((picked_out != nullptr) == (targets != nullptr), MILAN_ERR_ARG,
                "milan_lm_forward_train: targets go with picked_out, and only with it");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_lm_forward_train: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.grad_total, MILAN_ERR_WORKSPACE,
                "milan_lm_forward_train: workspace %zu < %zu bytes", ws_bytes, p.grad_total);
  Params w;
  MILAN_TRY(unpack(p, params, n_params, &w));
  const hipStream_t s = (hipStream_t)stream;
  float* f = (float*)ws;
  // the forward of the train step; its loss terms (of `targets`, or of the inputs read as
  // targets when there are none: any ids do) land behind the plan and are not used
  MILAN_TRY(forward(p, w, f, inputs, targets ? targets : inputs, dropout, seed, f + p.terms, s));
  if (logprobs_out)
    hipLaunchKernelGGL(lm_logprobs_kernel, dim3(blocks_for((long)p.N * p.V)), dim3(256), 0, s,
                       f + p.logits, f + p.lse, logprobs_out, p.N, p.V);
  if (picked_out)
    hipLaunchKernelGGL(lm_picked_kernel, dim3(blocks_for(p.N)), dim3(256), 0, s, f + p.logits,
                       targets, f + p.lse, picked_out, p.N, p.V);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int milan_lm_backward(milan_ctx* c, const float* const* params, float* const* grads,
                      int n_params, const int64_t* inputs, int rows, int L, float dropout,
                      uint64_t seed, const float* dlogprobs, const float* dpicked,
                      const int64_t* targets, void* ws, size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(grads && inputs && ws, MILAN_ERR_ARG, "milan_lm_backward: null argument");
  MILAN_REQUIRE(dlogprobs || dpicked, MILAN_ERR_ARG,
                "milan_lm_backward: neither dlogprobs nor dpicked given");
  MILAN_REQUIRE(!dpicked || targets, MILAN_ERR_ARG,
                "milan_lm_backward: dpicked needs the targets of the forward");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_lm_backward: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.grad_total, MILAN_ERR_WORKSPACE,
                "milan_lm_backward: workspace %zu < %zu bytes", ws_bytes, p.grad_total);
  Params w;
  MILAN_TRY(unpack(p, params, n_params, &w));
  Grads g;
  MILAN_TRY(unpack_grads(p, grads, n_params, &g));
  const hipStream_t s = (hipStream_t)stream;
  float* f = (float*)ws;
  // dlogits into the logits buffer, where backward() expects them
  hipLaunchKernelGGL(lm_log_softmax_bwd_kernel, dim3(p.N), dim3(256), 0, s, dlogprobs, dpicked,
                     targets, f + p.logits, f + p.lse, p.V);
  MILAN_CHECK_HIP(hipGetLastError());
  return backward(p, w, g, f, inputs, nullptr, dropout, seed, nullptr, s);
}

}  // extern "C"
