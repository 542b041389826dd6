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
// packed either: the one GEMM (tgemm.h) reads both operands through strided views, so
// X.W^T, dG^T.X and dG.W are the same kernel with different views.
//
// Determinism: every output element is reduced in a fixed order.  Split-K GEMMs add their
// partial sums in split order; the column sums (bias gradients) and the embedding gradient
// are ordered loops; the loss reduction is one workgroup.  No float atomics: two calls with
// the same inputs and seed give identical bits.
//
// This file also defines, in namespace train, the kernels that decoder_train.hip runs as
// well (train_common.h declares their launchers).
#include "train_common.h"

namespace milan {
namespace train {

// (what each kernel computes is said at its launcher in train_common.h)
__global__ void embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb,
                             float* __restrict__ x, int N, int E, long x_rs, int V) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)N * E) return;
  const int n = (int)(i / E), e = (int)(i % E);
  x[n * x_rs + e] = emb[(long)clamp_id(ids[n], V) * E + e];
}

__global__ void cell_fwd_kernel(float* __restrict__ G, const float* __restrict__ cprev,
                                float* __restrict__ cout, long c_rs, float* __restrict__ Hs,
                                int rows, int L, int H, int t) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const int b = (int)(i / H), j = (int)(i % H);
  float* g = G + ((long)b * L + t) * 4 * H;
  const float ig = sigm(g[j]), fg = sigm(g[H + j]), gg = tanhf(g[2 * H + j]),
              og = sigm(g[3 * H + j]);
  const float cp = cprev ? cprev[b * c_rs + j] : 0.f;
  const float c = fg * cp + ig * gg;
  g[j] = ig;
  g[H + j] = fg;
  g[2 * H + j] = gg;
  g[3 * H + j] = og;
  cout[b * c_rs + j] = c;
  Hs[((long)b * (L + 1) + t + 1) * H + j] = og * tanhf(c);
}

__global__ void dropout_fwd_kernel(const float* __restrict__ Hs, float* __restrict__ X,
                                   int rows, int L, int H, int tag, uint64_t seed,
                                   uint32_t thr, float scale) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * L * H) return;
  const int j = (int)(i % H);
  const long bt = i / H;
  const int t = (int)(bt % L), b = (int)(bt / L);
  float h = Hs[((long)b * (L + 1) + t + 1) * H + j];
  if (thr) h = keep(seed, tag, b, t, j, thr) ? h * scale : 0.f;
  X[i] = h;
}

__global__ void dropout_bwd_kernel(float* __restrict__ dY, int rows, int L, int H, int tag,
                                   uint64_t seed, uint32_t thr, float scale) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * L * H) return;
  const int j = (int)(i % H);
  const long bt = i / H;
  const int t = (int)(bt % L), b = (int)(bt / L);
  dY[i] = keep(seed, tag, b, t, j, thr) ? dY[i] * scale : 0.f;
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

// (dhrec is added by a branch, not as a zero addend when absent: -0 + 0 is not -0)
__global__ void cell_bwd_kernel(const float* __restrict__ dh, long dh_rs,
                                const float* __restrict__ dhrec, float* __restrict__ G,
                                const float* __restrict__ ccur, const float* __restrict__ cprev,
                                long c_rs, float* __restrict__ dc, int rows, int L, int H,
                                int t) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const int b = (int)(i / H), j = (int)(i % H);
  const bool last = t == L - 1;
  float* g = G + ((long)b * L + t) * 4 * H;
  const float ig = g[j], fg = g[H + j], gg = g[2 * H + j], og = g[3 * H + j];
  const float c = ccur[b * c_rs + j];
  const float cp = cprev ? cprev[b * c_rs + j] : 0.f;
  float d_h = dh[(long)b * dh_rs + j];
  if (dhrec) d_h = d_h + (last ? 0.f : dhrec[i]);
  const float tc = tanhf(c);
  const float dcur = d_h * og * (1.f - tc * tc) + (last ? 0.f : dc[i]);
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

// ---- host launchers (train_common.h) --------------------------------------------------------
void launch_embed(const int64_t* ids, const float* emb, float* x, int N, int E, long x_rs, int V,
                  hipStream_t s) {
  hipLaunchKernelGGL(embed_kernel, dim3(blocks_for((long)N * E)), dim3(256), 0, s, ids, emb, x, N,
                     E, x_rs, V);
}
void launch_embed_grad(const int64_t* ids, const float* dX, int N, int E, int V, int pad,
                       float* dEmb, hipStream_t s) {
  hipLaunchKernelGGL(embed_grad_kernel, dim3(V), dim3(256), 0, s, ids, dX, N, E, V, pad, dEmb);
}
void launch_dropout_fwd(const float* Hs, float* X, int rows, int L, int H, int tag, uint64_t seed,
                        uint32_t thr, float scale, hipStream_t s) {
  hipLaunchKernelGGL(dropout_fwd_kernel, dim3(blocks_for((long)rows * L * H)), dim3(256), 0, s,
                     Hs, X, rows, L, H, tag, seed, thr, scale);
}
void launch_dropout_bwd(float* dY, int rows, int L, int H, int tag, uint64_t seed, uint32_t thr,
                        float scale, hipStream_t s) {
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3(blocks_for((long)rows * L * H)), dim3(256), 0, s,
                     dY, rows, L, H, tag, seed, thr, scale);
}
void launch_cell_fwd(float* G, const float* cprev, float* cout, long c_rs, float* Hs, int rows,
                     int L, int H, int t, hipStream_t s) {
  hipLaunchKernelGGL(cell_fwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, G, cprev,
                     cout, c_rs, Hs, rows, L, H, t);
}
void launch_cell_bwd(const float* dh, long dh_rs, const float* dhrec, float* G, const float* ccur,
                     const float* cprev, long c_rs, float* dc, int rows, int L, int H, int t,
                     hipStream_t s) {
  hipLaunchKernelGGL(cell_bwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, dh, dh_rs,
                     dhrec, G, ccur, cprev, c_rs, dc, rows, L, H, t);
}
void launch_logprobs(const float* logits, const float* lse, float* out, int N, int V,
                     hipStream_t s) {
  hipLaunchKernelGGL(lm_logprobs_kernel, dim3(blocks_for((long)N * V)), dim3(256), 0, s, logits,
                     lse, out, N, V);
}
void launch_log_softmax_bwd(const float* G, const float* gp, const int64_t* tgt, float* logits,
                            const float* lse, int N, int V, hipStream_t s) {
  hipLaunchKernelGGL(lm_log_softmax_bwd_kernel, dim3(N), dim3(256), 0, s, G, gp, tgt, logits, lse,
                     V);
}

int output_forward(const OutLayer& o, View h_out, const float* w_out, const float* b_out,
                   const int64_t* targets, float* loss, Scratch sc, hipStream_t s) {
  MILAN_TRY(gemm(h_out, 0, view(w_out, o.H), 1, view(o.logits, o.V), view(nullptr, 0), b_out,
                 nullptr, o.N, o.V, o.H, sc, s));
  hipLaunchKernelGGL(nll_rows_kernel, dim3(o.N), dim3(256), 0, s, o.logits, targets, o.V, o.pad,
                     o.lse, o.term, o.valid);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, o.term, o.valid, o.N, loss);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int output_backward(const OutLayer& o, View h_out, const float* w_out, const int64_t* targets,
                    const float* loss, float* dw_out, float* db_out, float* dY, Scratch sc,
                    hipStream_t s) {
  const View none = view(nullptr, 0), dlog = view(o.logits, o.V);
  if (loss)
    hipLaunchKernelGGL(dlogits_kernel, dim3(o.N), dim3(256), 0, s, o.logits, targets, o.lse,
                       o.valid, loss, o.V);
  MILAN_TRY(gemm(dlog, 1, h_out, 0, view(dw_out, o.H), none, nullptr, nullptr, o.V, o.H, o.N, sc,
                 s));
  MILAN_TRY(colsum(o.logits, o.N, o.V, db_out, nullptr, sc, s));
  return gemm(dlog, 0, view(w_out, o.H), 0, view(dY, o.H), none, nullptr, nullptr, o.N, o.H, o.V,
              sc, s);
}

}  // namespace train

namespace lmt {
using namespace train;

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
  Layout w;
  p->x0 = w.take((size_t)N * E);
  for (int l = 0; l < p->NL; ++l) {
    p->xin[l] = l ? w.take((size_t)N * H) : p->x0;
    p->gates[l] = w.take((size_t)N * 4 * H);
    p->cst[l] = w.take((size_t)N * H);
    p->hs[l] = w.take((size_t)rows * (L + 1) * H);
  }
  p->logits = w.take((size_t)N * V);
  p->lse = w.take(N);
  p->term = w.take(N);
  p->valid = w.take(N);
  p->dy = w.take((size_t)N * (H > E ? H : E));
  p->dhrec = w.take((size_t)rows * H);
  p->dc = w.take((size_t)rows * H);
  w.need((size_t)colsum_chunks(N) * (V > 4 * H ? V : 4 * H));
  w.need(split_scratch_floats(N, V, H));      // logits
  w.need(split_scratch_floats(V, H, N));      // dW_out
  w.need(split_scratch_floats(N, H, V));      // dH of the top layer
  for (int l = 0; l < p->NL; ++l) {
    const int in = l ? H : E;
    w.need(split_scratch_floats(N, 4 * H, in));    // input projection
    w.need(split_scratch_floats(rows, 4 * H, H));  // recurrent step
    w.need(split_scratch_floats(rows, H, 4 * H));  // dh_{t-1}
    w.need(split_scratch_floats(4 * H, H, N));     // dW_hh
    w.need(split_scratch_floats(4 * H, in, N));    // dW_ih
    w.need(split_scratch_floats(N, in, 4 * H));    // dX
  }
  p->scratch = w.take(w.scratch);
  p->scratch_floats = w.scratch;
  p->total = w.off * sizeof(float);
  // after `total`, what the autograd pair (milan_lm_forward_train / _backward) adds: the
  // forward's loss terms, which nobody reads (the backward overwrites activations in place
  // and needs no buffer of its own)
  p->terms = w.take(2);
  p->grad_total = w.off * sizeof(float);
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

// Forward (+ loss).  train: dropout between layers with (p, seed).
static int forward(const Plan& p, const Params& w, float* ws, const int64_t* inputs,
                   const int64_t* targets, float p_drop, uint64_t seed, float* loss,
                   hipStream_t s) {
  const int N = p.N, H = p.H, E = p.E, rows = p.rows, L = p.L;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  launch_embed(inputs, w.emb, ws + p.x0, N, E, E, p.V, s);
  for (int l = 0; l < p.NL; ++l) {
    const int in = l ? H : E;
    float* G = ws + p.gates[l];
    float* C = ws + p.cst[l];  // c_t [rows][L][H]
    float* Hs = ws + p.hs[l];
    MILAN_CHECK_HIP(hipMemsetAsync(Hs, 0, sizeof(float) * rows * (L + 1) * H, s));
    if (l)  // input of layer l = dropout(h of layer l - 1), tagged with that layer
      launch_dropout_fwd(ws + p.hs[l - 1], ws + p.xin[l], rows, L, H, l - 1, seed,
                         drop_threshold(p_drop), drop_scale(p_drop), s);
    // pre-activations of every position: X . W_ih^T + b_ih + b_hh
    MILAN_TRY(gemm(view(ws + p.xin[l], in), 0, view(w.w_ih[l], in), 1, view(G, 4 * H), none,
                   w.b_ih[l], w.b_hh[l], N, 4 * H, in, sc, s));
    for (int t = 0; t < L; ++t) {
      if (t) {  // += h_{t-1} . W_hh^T  (h_{t-1} = slot t of Hs)
        const View g = view(G + (size_t)t * 4 * H, (long)L * 4 * H);
        MILAN_TRY(gemm(view(Hs + (size_t)t * H, (long)(L + 1) * H), 0, view(w.w_hh[l], H), 1, g,
                       g, nullptr, nullptr, rows, 4 * H, H, sc, s));
      }
      launch_cell_fwd(G, t ? C + (size_t)(t - 1) * H : nullptr, C + (size_t)t * H, (long)L * H, Hs,
                      rows, L, H, t, s);
    }
  }
  // logits of every position (top layer, no dropout on its output)
  const View htop = view(ws + p.hs[p.NL - 1] + H, H, L, (long)(L + 1) * H);
  return output_forward(out_layer(p, ws), htop, w.w_out, w.b_out, targets, loss, sc, s);
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
  const int N = p.N, H = p.H, E = p.E, rows = p.rows, L = p.L;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  const uint32_t thr = drop_threshold(p_drop);
  const View htop = view(ws + p.hs[p.NL - 1] + H, H, L, (long)(L + 1) * H);
  float* dY = ws + p.dy;
  // (loss null: the logits buffer already holds dlogits, milan_lm_backward)
  MILAN_TRY(output_backward(out_layer(p, ws), htop, w.w_out, targets, loss, gr.w_out, gr.b_out,
                            dY, sc, s));
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
      launch_cell_bwd(dht, rs, nullptr, G, C + (size_t)t * H, t ? C + (size_t)(t - 1) * H : nullptr,
                      (long)L * H, dc, rows, L, H, t, s);
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
    if (l && thr) launch_dropout_bwd(dY, rows, L, H, l - 1, seed, thr, drop_scale(p_drop), s);
  }
  launch_embed_grad(inputs, dY, N, E, p.V, p.pad, gr.emb, s);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
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
  if (logprobs_out) launch_logprobs(f + p.logits, f + p.lse, logprobs_out, p.N, p.V, s);
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
  launch_log_softmax_bwd(dlogprobs, dpicked, targets, f + p.logits, f + p.lse, p.N, p.V, s);
  MILAN_CHECK_HIP(hipGetLastError());
  return backward(p, w, g, f, inputs, nullptr, dropout, seed, nullptr, s);
}

}  // extern "C"
