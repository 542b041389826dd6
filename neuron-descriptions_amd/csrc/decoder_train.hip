// Decoder training (src/milan/decoders.py:873-1070): the loss, forward and backward of the
// teacher-forced attention LSTM, Decoder.forward(features, strategy=targets, mi=False) in
// training mode (decoders.py:431-463, 576-634), over a padded (rows, L) batch of targets
// with k visual features per row.
//
//   h_0 = tanh(W_h mean_k f + b_h),  c_0 = tanh(W_c mean_k f + b_c)
//   per step t (input x_t = <start> at t = 0, targets[:, t-1] after):
//     q = W_q h_t + b_q;  u_k = tanh(q + W_k f_k + b_k);  s_k = w_o . u_k + b_o
//     alpha = softmax_k(s);  ctx = sum_k alpha_k f_k;  z = ctx * sigmoid(W_g h_t + b_g)
//     (h_{t+1}, c_{t+1}) = LSTMCell([emb(x_t) ; z], (h_t, c_t))
//     log p_t = log_softmax(W_out dropout(h_{t+1}) + b_out)
//   loss = NLL(ignore pad) mean + w * mean_{row, k} (1 - sum_t alpha_{t,k})^2
//
// As in lm_train.hip: exact fp32 MFMA whatever milan_set_precision says, raw torch-layout
// parameters read on every call through the strided GEMM of tgemm.h, fixed reduction orders
// and no float atomics (equal inputs and seed give equal bits).  The embedding gather and
// gradient, the dropout, the LSTM cell, the log-softmax and the output layer are the LM
// trainer's (train_common.h); the attention and the init_h / init_c kernels are defined here.
//
// Layout.  Hoisted before the time loop: the feature mean and the
// init_h / init_c GEMMs, the attention keys W_k f + b_k of all rows * k features, and the
// embedding columns of W_ih for all rows * L inputs (teacher forcing knows every input up
// front).  Per step: the query and gate GEMMs, one attention kernel (scores, softmax,
// context, gate), the context columns of W_ih and W_hh accumulated into the step's gates,
// the cell.  After the loop: one vocabulary GEMM, the NLL rows and the regulariser.
// Backward per step, in reverse time: cell, dz = dG . W_ih[:, E:], one attention-backward
// kernel (gate, context, softmax and tanh backward into dq and the per-feature dK, which is
// accumulated in fixed t order), dh_t = dq . W_q + dgate . W_g + dG . W_hh.  The weight
// gradients are grouped GEMMs over all steps after the loop.
#include "train_common.h"

namespace milan {
namespace dect {
using namespace train;

constexpr int kMaxK = 64;  // features per row (the attention kernels keep k scores in LDS)

// Teacher-forced inputs: in[b][0] = start, in[b][t] = targets[b][t - 1].
__global__ void inputs_kernel(const int64_t* __restrict__ tgt, int64_t* __restrict__ in, int rows,
                              int L, int start) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * L) return;
  const int t = (int)(i % L);
  in[i] = t ? tgt[i - 1] : (int64_t)start;
}

// pooled[b][f] = (sum over k of feat[b][k][f], in k order) / k
__global__ void pool_kernel(const float* __restrict__ feat, float* __restrict__ pooled, int rows,
                            int k, int F) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * F) return;
  const int b = (int)(i / F), f = (int)(i % F);
  float s = 0.f;
  for (int j = 0; j < k; ++j) s += feat[((long)b * k + j) * F + f];
  pooled[i] = s / (float)k;
}

// slot 0 of Hs and C: tanh of the init_h / init_c pre-activations written there
__global__ void init_fwd_kernel(float* __restrict__ Hs, float* __restrict__ C, int rows, int L,
                                int H) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const long o = (i / H) * (L + 1) * H + i % H;
  Hs[o] = tanhf(Hs[o]);
  C[o] = tanhf(C[o]);
}

// Attention of step t, one workgroup per row b.  Q: queries [rows * L][A]; Kh: keys
// [rows * k][A]; GT: gate pre-activations in, sigmoid out [rows * L][F].  Writes U (the tanh
// hidden, [rows * L * k][A]), ALPHA [rows * L][k], CTX [rows * L][F] and z = ctx * gate into
// the context columns of X.
__global__ __launch_bounds__(256) void attend_fwd_kernel(
    const float* __restrict__ Q, const float* __restrict__ Kh, const float* __restrict__ feat,
    const float* __restrict__ w_o, const float* __restrict__ b_o, float* __restrict__ GT,
    float* __restrict__ CTX, float* __restrict__ X, float* __restrict__ ALPHA,
    float* __restrict__ U, int L, int k, int A, int F, int E, int t) {
  __shared__ float sc[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long n = (long)b * L + t;
  const float* q = Q + n * A;
  for (int j = w; j < k; j += 4) {
    const float* kh = Kh + ((long)b * k + j) * A;
    float* u = U + (n * k + j) * A;
    float s = 0.f;
    for (int a = lane; a < A; a += 64) {
      const float v = tanhf(q[a] + kh[a]);
      u[a] = v;
      s += v * w_o[a];
    }
    s = wave_sum(s);
    if (lane == 0) sc[j] = s + b_o[0];
  }
  __syncthreads();
  if (tid == 0) {
    float m = -INFINITY;
    for (int j = 0; j < k; ++j) m = fmaxf(m, sc[j]);
    float sum = 0.f;
    for (int j = 0; j < k; ++j) {
      sc[j] = expf(sc[j] - m);
      sum += sc[j];
    }
    for (int j = 0; j < k; ++j) {
      sc[j] = sc[j] / sum;
      ALPHA[n * k + j] = sc[j];
    }
  }
  __syncthreads();
  const float* fb = feat + (long)b * k * F;
  for (int f = tid; f < F; f += blockDim.x) {
    float c = 0.f;
    for (int j = 0; j < k; ++j) c += sc[j] * fb[(long)j * F + f];
    const float g = sigm(GT[n * F + f]);
    GT[n * F + f] = g;
    CTX[n * F + f] = c;
    X[n * (E + F) + E + f] = c * g;
  }
}

// S[b][j] = sum over t (in order) of alpha[b][t][j]
__global__ void attn_sum_kernel(const float* __restrict__ ALPHA, float* __restrict__ S, int rows,
                                int L, int k) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * k) return;
  const int b = (int)(i / k), j = (int)(i % k);
  float s = 0.f;
  for (int t = 0; t < L; ++t) s += ALPHA[((long)b * L + t) * k + j];
  S[i] = s;
}

// out[0] = sum over rows * k of (1 - S)^2 (one workgroup, fixed order)
__global__ __launch_bounds__(256) void reg_reduce_kernel(const float* __restrict__ S, long n,
                                                         float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += blockDim.x) {
    const float d = 1.f - S[i];
    s += d * d;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

// Attention backward of step t, one workgroup per row b.  dZ: dL/dz of the step [rows][F].
// Writes DGP (d gate pre-activation, [rows * L][F]), DS (d score, [rows * L][k]), DQ (d query,
// [rows * L][A]) and accumulates dKh [rows * k][A] (overwritten at t = L - 1, then added to
// in decreasing t).  reg = 2 w / (rows * k): the regulariser adds -reg (1 - S) to d alpha.
__global__ __launch_bounds__(256) void attend_bwd_kernel(
    const float* __restrict__ dZ, const float* __restrict__ GT, const float* __restrict__ CTX,
    const float* __restrict__ feat, const float* __restrict__ ALPHA, const float* __restrict__ U,
    const float* __restrict__ S, const float* __restrict__ w_o, float reg,
    float* __restrict__ DGP, float* __restrict__ DS, float* __restrict__ DQ,
    float* __restrict__ dKh, int L, int k, int A, int F, int t) {
  __shared__ float da[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long n = (long)b * L + t;
  const float* dz = dZ + (long)b * F;
  const float* gt = GT + n * F;
  const float* fb = feat + (long)b * k * F;
  for (int f = tid; f < F; f += blockDim.x) {
    const float g = gt[f];
    DGP[n * F + f] = dz[f] * CTX[n * F + f] * g * (1.f - g);
  }
  // d alpha_j = (dz * gate) . f_j - reg (1 - S_j)
  for (int j = w; j < k; j += 4) {
    const float* fj = fb + (long)j * F;
    float s = 0.f;
    for (int f = lane; f < F; f += 64) s += dz[f] * gt[f] * fj[f];
    s = wave_sum(s);
    if (lane == 0) da[j] = s - reg * (1.f - S[(long)b * k + j]);
  }
  __syncthreads();
  if (tid == 0) {
    float dot = 0.f;
    for (int j = 0; j < k; ++j) dot += ALPHA[n * k + j] * da[j];
    for (int j = 0; j < k; ++j) {
      da[j] = ALPHA[n * k + j] * (da[j] - dot);
      DS[n * k + j] = da[j];
    }
  }
  __syncthreads();
  for (int a = tid; a < A; a += blockDim.x) {
    const float wa = w_o[a];
    float dq = 0.f;
    for (int j = 0; j < k; ++j) {
      const float u = U[(n * k + j) * A + a];
      const float du = da[j] * wa * (1.f - u * u);
      dq += du;
      const long o = ((long)b * k + j) * A + a;
      dKh[o] = t == L - 1 ? du : dKh[o] + du;
    }
    DQ[n * A + a] = dq;
  }
}

// attend_bwd_kernel driven by an upstream gradient instead of the regulariser (the autograd
// backward, milan_decoder_backward): d alpha_j = (dz * gate) . f_j + dA[n][j] (dA null: zero),
// and DCTX [rows * L][F] (null: not stored) receives dctx = dz * gate, the context's share of
// the feature gradient.  A kernel of its own, so that attend_bwd_kernel, which
// milan_decoder_train_step runs, keeps its instruction stream.
__global__ __launch_bounds__(256) void attend_bwd_up_kernel(
    const float* __restrict__ dZ, const float* __restrict__ GT, const float* __restrict__ CTX,
    const float* __restrict__ feat, const float* __restrict__ ALPHA, const float* __restrict__ U,
    const float* __restrict__ dA, const float* __restrict__ w_o, float* __restrict__ DCTX,
    float* __restrict__ DGP, float* __restrict__ DS, float* __restrict__ DQ,
    float* __restrict__ dKh, int L, int k, int A, int F, int t) {
  __shared__ float da[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long n = (long)b * L + t;
  const float* dz = dZ + (long)b * F;
  const float* gt = GT + n * F;
  const float* fb = feat + (long)b * k * F;
  for (int f = tid; f < F; f += blockDim.x) {
    const float g = gt[f];
    DGP[n * F + f] = dz[f] * CTX[n * F + f] * g * (1.f - g);
    if (DCTX) DCTX[n * F + f] = dz[f] * g;
  }
  for (int j = w; j < k; j += 4) {
    const float* fj = fb + (long)j * F;
    float s = 0.f;
    for (int f = lane; f < F; f += 64) s += dz[f] * gt[f] * fj[f];
    s = wave_sum(s);
    if (lane == 0) da[j] = dA ? s + dA[n * k + j] : s;
  }
  __syncthreads();
  if (tid == 0) {
    float dot = 0.f;
    for (int j = 0; j < k; ++j) dot += ALPHA[n * k + j] * da[j];
    for (int j = 0; j < k; ++j) {
      da[j] = ALPHA[n * k + j] * (da[j] - dot);
      DS[n * k + j] = da[j];
    }
  }
  __syncthreads();
  for (int a = tid; a < A; a += blockDim.x) {
    const float wa = w_o[a];
    float dq = 0.f;
    for (int j = 0; j < k; ++j) {
      const float u = U[(n * k + j) * A + a];
      const float du = da[j] * wa * (1.f - u * u);
      dq += du;
      const long o = ((long)b * k + j) * A + a;
      dKh[o] = t == L - 1 ? du : dKh[o] + du;
    }
    DQ[n * A + a] = dq;
  }
}

// The context and mean-pool shares of the feature gradient, added to the key share that dF
// [rows][k][F] holds: dF[b][j][f] = (dF[b][j][f] + sum over t (increasing) of
// alpha[b][t][j] * dctx[b][t][f]) + dpool[b][f] / k.
__global__ void dfeat_kernel(const float* __restrict__ ALPHA, const float* __restrict__ DCTX,
                             const float* __restrict__ dpool, float* __restrict__ dF, int rows,
                             int L, int k, int F) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * k * F) return;
  const int f = (int)(i % F);
  const long bj = i / F;
  const int j = (int)(bj % k), b = (int)(bj / k);
  float s = 0.f;
  for (int t = 0; t < L; ++t) {
    const long n = (long)b * L + t;
    s += ALPHA[n * k + j] * DCTX[n * F + f];
  }
  dF[i] = (dF[i] + s) + dpool[(long)b * F + f] / (float)k;
}

// d pre-activations of init_h / init_c from dh_0 (dhrec) and dc_0 (dc)
__global__ void init_bwd_kernel(const float* __restrict__ Hs, const float* __restrict__ C,
                                const float* __restrict__ dhrec, const float* __restrict__ dc,
                                float* __restrict__ dph, float* __restrict__ dpc, int rows, int L,
                                int H) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)rows * H) return;
  const long o = (i / H) * (L + 1) * H + i % H;
  const float h = Hs[o], c = C[o];
  dph[i] = dhrec[i] * (1.f - h * h);
  dpc[i] = dc[i] * (1.f - c * c);
}

// ---- workspace layout -------------------------------------------------------------------
struct Plan {
  int V, E, H, A, F, pad, start, rows, k, L, N;
  size_t ids, pooled, kh, x, g, cst, hs, hd, q, gt, ctx, alpha, u, s, logits, lse, term, valid;
  size_t dy, dhrec, dc, dz, dgp, ds, dq, dkh, dxe, dph, dpc, scratch, scratch_floats, total;
  // after `total`, what the autograd pair (milan_decoder_forward_train / _backward) adds:
  // the loss terms the forward still computes, dctx_t = dz_t * gate_t of every step, the
  // pooled features' gradient and the scratch of the feature-gradient GEMMs
  size_t terms, dctx, dpool, gscratch, gscratch_floats, grad_total;
};

static int make_plan(const milan_ctx* c, int rows, int k, int L, Plan* p) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "decoder train: null ctx");
  const milan_dims& d = c->d;
  MILAN_REQUIRE(rows > 0 && L > 0 && rows < (1 << 24) && L < (1 << 16), MILAN_ERR_SHAPE,
                "decoder train: need 0 < rows < 2^24 and 0 < L < 2^16 (rows %d, L %d)", rows, L);
  MILAN_REQUIRE(k > 0 && k <= kMaxK, MILAN_ERR_SHAPE,
                "decoder train: need 0 < k <= %d features per row, got %d", kMaxK, k);
  MILAN_REQUIRE((long)rows * L * k < (1L << 30), MILAN_ERR_SHAPE, "decoder train: batch too large");
  MILAN_REQUIRE(d.hidden_size > 0 && d.hidden_size < (1 << 14) && d.embedding_size > 0 &&
                    d.attention_size > 0 && d.feature_size > 0 && d.vocab_size > 0,
                MILAN_ERR_SHAPE, "decoder train: the context has no decoder dims");
  p->V = d.vocab_size;
  p->E = d.embedding_size;
  p->H = d.hidden_size;
  p->A = d.attention_size;
  p->F = d.feature_size;
  p->pad = d.pad_index;
  p->start = d.start_index;
  p->rows = rows;
  p->k = k;
  p->L = L;
  const int N = p->N = rows * L, H = p->H, E = p->E, V = p->V, A = p->A, F = p->F;
  const long BK = (long)rows * k;
  Layout w;
  p->ids = w.take((size_t)N * 2);  // int64
  p->pooled = w.take((size_t)rows * F);
  p->kh = w.take((size_t)BK * A);
  p->x = w.take((size_t)N * (E + F));
  p->g = w.take((size_t)N * 4 * H);
  p->cst = w.take((size_t)rows * (L + 1) * H);
  p->hs = w.take((size_t)rows * (L + 1) * H);
  p->hd = w.take((size_t)N * H);
  p->q = w.take((size_t)N * A);
  p->gt = w.take((size_t)N * F);
  p->ctx = w.take((size_t)N * F);
  p->alpha = w.take((size_t)N * k);
  p->u = w.take((size_t)N * k * A);
  p->s = w.take((size_t)BK);
  p->logits = w.take((size_t)N * V);
  p->lse = w.take(N);
  p->term = w.take(N);
  p->valid = w.take(N);
  p->dy = w.take((size_t)N * H);
  p->dhrec = w.take((size_t)rows * H);
  p->dc = w.take((size_t)rows * H);
  p->dz = w.take((size_t)rows * F);
  p->dgp = w.take((size_t)N * F);
  p->ds = w.take((size_t)N * k);
  p->dq = w.take((size_t)N * A);
  p->dkh = w.take((size_t)BK * A);
  p->dxe = w.take((size_t)N * E);
  p->dph = w.take((size_t)rows * H);
  p->dpc = w.take((size_t)rows * H);
  auto cs = [&](long R, long cols) { w.need((size_t)colsum_chunks((int)R) * cols); };
  cs(N, V);
  cs(N, 4 * H);
  cs(N, A);
  cs(N, F);
  cs(BK, A);
  cs((long)N * k, 1);
  cs(rows, H);
  const int KK = (int)((long)N * k);
  const int shapes[][3] = {
      {rows, H, F},  {(int)BK, A, F}, {N, 4 * H, E},  {rows, A, H},     {rows, F, H},
      {rows, 4 * H, F}, {rows, 4 * H, H}, {N, V, H},  {V, H, N},        {N, H, V},
      {rows, F, 4 * H}, {rows, H, A}, {rows, H, 4 * H}, {4 * H, E + F, N}, {4 * H, H, N}, {A, H, N},
      {F, H, N},     {A, F, (int)BK}, {1, A, KK},     {N, E, 4 * H},    {H, F, rows}};
  for (const auto& s : shapes) w.need(split_scratch_floats(s[0], s[1], s[2]));
  p->scratch = w.take(w.scratch);
  p->scratch_floats = w.scratch;
  p->total = w.off * sizeof(float);
  p->terms = w.take(4);
  p->dctx = w.take((size_t)N * F);
  p->dpool = w.take((size_t)rows * F);
  const size_t gk = split_scratch_floats((int)BK, F, A), gp = split_scratch_floats(rows, F, H);
  const size_t gsc = gk > gp ? gk : gp;  // dKh . W_k, then dph . W_init_h + dpc . W_init_c
  p->gscratch = w.take(gsc);
  p->gscratch_floats = gsc;
  p->grad_total = w.off * sizeof(float);
  return 0;
}

// the 19 tensors of the decoder's own state dict, in the reference's order
enum {
  P_INIT_H_W, P_INIT_H_B, P_INIT_C_W, P_INIT_C_B, P_EMB, P_Q_W, P_Q_B, P_K_W, P_K_B, P_O_W,
  P_O_B, P_GATE_W, P_GATE_B, P_W_IH, P_W_HH, P_B_IH, P_B_HH, P_OUT_W, P_OUT_B, N_PARAMS
};

static int check_params(const void* const* params, int n, const char* what) {
  MILAN_REQUIRE(params, MILAN_ERR_ARG, "decoder train: null %s list", what);
  MILAN_REQUIRE(n == N_PARAMS, MILAN_ERR_ARG,
                "decoder train: %d %s pointers given, the decoder's state dict has %d", n, what,
                (int)N_PARAMS);
  for (int i = 0; i < n; ++i)
    MILAN_REQUIRE(params[i], MILAN_ERR_ARG, "decoder train: %s %d is null", what, i);
  return 0;
}

// Forward, loss terms [nll sum, valid count, sum (1 - S)^2].  thr > 0: dropout on h.
static int forward(const Plan& p, const float* const* w, float* ws, const float* feat,
                   const int64_t* targets, uint32_t thr, float scale, uint64_t seed, float* loss,
                   hipStream_t s) {
  const int N = p.N, H = p.H, E = p.E, V = p.V, A = p.A, F = p.F, rows = p.rows, k = p.k,
            L = p.L;
  const int BK = rows * k;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  int64_t* ids = (int64_t*)(ws + p.ids);
  float *X = ws + p.x, *G = ws + p.g, *C = ws + p.cst, *Hs = ws + p.hs, *Q = ws + p.q,
        *GT = ws + p.gt, *Kh = ws + p.kh;
  hipLaunchKernelGGL(inputs_kernel, dim3(blocks_for(N)), dim3(256), 0, s, targets, ids, rows, L,
                     p.start);
  launch_embed(ids, w[P_EMB], X, N, E, E + F, V, s);  // (the context columns follow)
  hipLaunchKernelGGL(pool_kernel, dim3(blocks_for((long)rows * F)), dim3(256), 0, s, feat,
                     ws + p.pooled, rows, k, F);
  MILAN_CHECK_HIP(hipGetLastError());
  // h_0, c_0 into slot 0 of Hs / C
  const View slot0h = view(Hs, (long)(L + 1) * H), slot0c = view(C, (long)(L + 1) * H);
  MILAN_TRY(gemm(view(ws + p.pooled, F), 0, view(w[P_INIT_H_W], F), 1, slot0h, none,
                 w[P_INIT_H_B], nullptr, rows, H, F, sc, s));
  MILAN_TRY(gemm(view(ws + p.pooled, F), 0, view(w[P_INIT_C_W], F), 1, slot0c, none,
                 w[P_INIT_C_B], nullptr, rows, H, F, sc, s));
  hipLaunchKernelGGL(init_fwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, Hs, C,
                     rows, L, H);
  // attention keys of every feature, embedding part of every step's gates
  MILAN_TRY(gemm(view(feat, F), 0, view(w[P_K_W], F), 1, view(Kh, A), none, w[P_K_B], nullptr,
                 BK, A, F, sc, s));
  MILAN_TRY(gemm(view(X, E + F), 0, view(w[P_W_IH], E + F), 1, view(G, 4 * H), none, w[P_B_IH],
                 w[P_B_HH], N, 4 * H, E, sc, s));
  for (int t = 0; t < L; ++t) {
    const View ht = view(Hs + (size_t)t * H, (long)(L + 1) * H);
    MILAN_TRY(gemm(ht, 0, view(w[P_Q_W], H), 1, view(Q + (size_t)t * A, (long)L * A), none,
                   w[P_Q_B], nullptr, rows, A, H, sc, s));
    MILAN_TRY(gemm(ht, 0, view(w[P_GATE_W], H), 1, view(GT + (size_t)t * F, (long)L * F), none,
                   w[P_GATE_B], nullptr, rows, F, H, sc, s));
    hipLaunchKernelGGL(attend_fwd_kernel, dim3(rows), dim3(256), 0, s, Q, Kh, feat, w[P_O_W],
                       w[P_O_B], GT, ws + p.ctx, X, ws + p.alpha, ws + p.u, L, k, A, F, E, t);
    MILAN_CHECK_HIP(hipGetLastError());
    const View gt = view(G + (size_t)t * 4 * H, (long)L * 4 * H);
    MILAN_TRY(gemm(view(X + (size_t)t * (E + F) + E, (long)L * (E + F)), 0,
                   view(w[P_W_IH] + E, E + F), 1, gt, gt, nullptr, nullptr, rows, 4 * H, F, sc,
                   s));
    MILAN_TRY(gemm(ht, 0, view(w[P_W_HH], H), 1, gt, gt, nullptr, nullptr, rows, 4 * H, H, sc, s));
    // c_t, h_t: slot t of C, Hs [rows][L + 1][H] in, slot t + 1 out
    launch_cell_fwd(G, C + (size_t)t * H, C + (size_t)(t + 1) * H, (long)(L + 1) * H, Hs, rows, L,
                    H, t, s);
  }
  // logits of every position from (dropped-out) h_{t+1}
  View hout = view(Hs + H, H, L, (long)(L + 1) * H);
  if (thr) {
    launch_dropout_fwd(Hs, ws + p.hd, rows, L, H, kDecoderDropoutTag, seed, thr, scale, s);
    hout = view(ws + p.hd, H);
  }
  MILAN_TRY(output_forward(out_layer(p, ws), hout, w[P_OUT_W], w[P_OUT_B], targets, loss, sc, s));
  hipLaunchKernelGGL(attn_sum_kernel, dim3(blocks_for(BK)), dim3(256), 0, s, ws + p.alpha,
                     ws + p.s, rows, L, k);
  hipLaunchKernelGGL(reg_reduce_kernel, dim3(1), dim3(256), 0, s, ws + p.s, (long)BK, loss + 2);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Upstream gradients of the autograd backward (milan_decoder_backward): the logits buffer
// already holds dlogits; dattn [rows * L][k] is dL/d alpha (null: zero); dctx [rows * L][F]
// receives dz * gate per step (null: not stored).
struct Upstream {
  const float* dattn;
  float* dctx;
};

// Backward of the training loss (up == nullptr: dlogits from the loss terms `loss`, the
// regulariser with `reg_weight`) or of upstream gradients (up != nullptr).
static int backward(const Plan& p, const float* const* w, float* const* gr, float* ws,
                    const float* feat, const int64_t* targets, uint32_t thr, float scale,
                    uint64_t seed, float reg_weight, const float* loss, const Upstream* up,
                    hipStream_t s) {
  const int N = p.N, H = p.H, E = p.E, V = p.V, A = p.A, F = p.F, rows = p.rows, k = p.k,
            L = p.L;
  const int BK = rows * k;
  const Scratch sc{ws + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  const int64_t* ids = (const int64_t*)(ws + p.ids);
  float *X = ws + p.x, *G = ws + p.g, *Hs = ws + p.hs, *dY = ws + p.dy, *dh = ws + p.dhrec,
        *dc = ws + p.dc, *dZ = ws + p.dz, *DGP = ws + p.dgp, *DQ = ws + p.dq, *DS = ws + p.ds,
        *dKh = ws + p.dkh;
  const View hout = thr ? view(ws + p.hd, H) : view(Hs + H, H, L, (long)(L + 1) * H);
  // (loss is null exactly when up is given: the logits buffer then holds dlogits)
  MILAN_TRY(output_backward(out_layer(p, ws), hout, w[P_OUT_W], targets, loss, gr[P_OUT_W],
                            gr[P_OUT_B], dY, sc, s));
  if (thr) launch_dropout_bwd(dY, rows, L, H, kDecoderDropoutTag, seed, thr, scale, s);
  const float reg = 2.f * reg_weight / (float)BK;
  const float* C = ws + p.cst;
  for (int t = L - 1; t >= 0; --t) {
    // dL/dh_{t+1} = dY[:, t] + dh through step t + 1 (absent at t = L - 1)
    launch_cell_bwd(dY + (size_t)t * H, (long)L * H, dh, G, C + (size_t)(t + 1) * H,
                    C + (size_t)t * H, (long)(L + 1) * H, dc, rows, L, H, t, s);
    const View dgt = view(G + (size_t)t * 4 * H, (long)L * 4 * H);
    // dz = dG_t . W_ih[:, E:]
    MILAN_TRY(gemm(dgt, 0, view(w[P_W_IH] + E, E + F), 0, view(dZ, F), none, nullptr, nullptr,
                   rows, F, 4 * H, sc, s));
    if (up)
      hipLaunchKernelGGL(attend_bwd_up_kernel, dim3(rows), dim3(256), 0, s, dZ, ws + p.gt,
                         ws + p.ctx, feat, ws + p.alpha, ws + p.u, up->dattn, w[P_O_W], up->dctx,
                         DGP, DS, DQ, dKh, L, k, A, F, t);
    else
      hipLaunchKernelGGL(attend_bwd_kernel, dim3(rows), dim3(256), 0, s, dZ, ws + p.gt,
                         ws + p.ctx, feat, ws + p.alpha, ws + p.u, ws + p.s, w[P_O_W], reg, DGP,
                         DS, DQ, dKh, L, k, A, F, t);
    MILAN_CHECK_HIP(hipGetLastError());
    // dL/dh_t through step t = dq . W_q + dgate . W_g + dG . W_hh
    const View dhv = view(dh, H);
    MILAN_TRY(gemm(view(DQ + (size_t)t * A, (long)L * A), 0, view(w[P_Q_W], H), 0, dhv, none,
                   nullptr, nullptr, rows, H, A, sc, s));
    MILAN_TRY(gemm(view(DGP + (size_t)t * F, (long)L * F), 0, view(w[P_GATE_W], H), 0, dhv, dhv,
                   nullptr, nullptr, rows, H, F, sc, s));
    MILAN_TRY(gemm(dgt, 0, view(w[P_W_HH], H), 0, dhv, dhv, nullptr, nullptr, rows, H, 4 * H, sc,
                   s));
  }
  // weight gradients, grouped over all steps (h_t = slot t of Hs)
  const View hprev = view(Hs, H, L, (long)(L + 1) * H);
  MILAN_TRY(gemm(view(G, 4 * H), 1, view(X, E + F), 0, view(gr[P_W_IH], E + F), none, nullptr,
                 nullptr, 4 * H, E + F, N, sc, s));
  MILAN_TRY(gemm(view(G, 4 * H), 1, hprev, 0, view(gr[P_W_HH], H), none, nullptr, nullptr, 4 * H,
                 H, N, sc, s));
  MILAN_TRY(colsum(G, N, 4 * H, gr[P_B_IH], gr[P_B_HH], sc, s));
  MILAN_TRY(gemm(view(DQ, A), 1, hprev, 0, view(gr[P_Q_W], H), none, nullptr, nullptr, A, H, N,
                 sc, s));
  MILAN_TRY(colsum(DQ, N, A, gr[P_Q_B], nullptr, sc, s));
  MILAN_TRY(gemm(view(DGP, F), 1, hprev, 0, view(gr[P_GATE_W], H), none, nullptr, nullptr, F, H,
                 N, sc, s));
  MILAN_TRY(colsum(DGP, N, F, gr[P_GATE_B], nullptr, sc, s));
  MILAN_TRY(gemm(view(dKh, A), 1, view(feat, F), 0, view(gr[P_K_W], F), none, nullptr, nullptr,
                 A, F, BK, sc, s));
  MILAN_TRY(colsum(dKh, BK, A, gr[P_K_B], nullptr, sc, s));
  const int NK = N * k;
  MILAN_TRY(gemm(view(DS, 1), 1, view(ws + p.u, A), 0, view(gr[P_O_W], A), none, nullptr,
                 nullptr, 1, A, NK, sc, s));
  MILAN_TRY(colsum(DS, NK, 1, gr[P_O_B], nullptr, sc, s));
  // embedding: dX_emb = dG . W_ih[:, :E], summed by token id (no padding row)
  MILAN_TRY(gemm(view(G, 4 * H), 0, view(w[P_W_IH], E + F), 0, view(ws + p.dxe, E), none,
                 nullptr, nullptr, N, E, 4 * H, sc, s));
  launch_embed_grad(ids, ws + p.dxe, N, E, V, -1, gr[P_EMB], s);
  // init_h / init_c from dh_0 / dc_0
  hipLaunchKernelGGL(init_bwd_kernel, dim3(blocks_for((long)rows * H)), dim3(256), 0, s, Hs,
                     ws + p.cst, dh, dc, ws + p.dph, ws + p.dpc, rows, L, H);
  MILAN_TRY(gemm(view(ws + p.dph, H), 1, view(ws + p.pooled, F), 0, view(gr[P_INIT_H_W], F),
                 none, nullptr, nullptr, H, F, rows, sc, s));
  MILAN_TRY(colsum(ws + p.dph, rows, H, gr[P_INIT_H_B], nullptr, sc, s));
  MILAN_TRY(gemm(view(ws + p.dpc, H), 1, view(ws + p.pooled, F), 0, view(gr[P_INIT_C_W], F),
                 none, nullptr, nullptr, H, F, rows, sc, s));
  MILAN_TRY(colsum(ws + p.dpc, rows, H, gr[P_INIT_C_B], nullptr, sc, s));
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace dect
}  // namespace milan

using namespace milan;
using namespace milan::dect;

extern "C" {

size_t milan_decoder_train_workspace_bytes(const milan_ctx* c, int rows, int k, int L) {
  Plan p;
  if (make_plan(c, rows, k, L, &p) != 0) return 0;
  return p.total;
}

int milan_decoder_nll(milan_ctx* c, const float* const* params, int n_params,
                      const float* features, const int64_t* targets, int rows, int k, int L,
                      float* loss_terms, void* ws, size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(features && targets && loss_terms && ws, MILAN_ERR_ARG,
                "milan_decoder_nll: null argument");
  Plan p;
  MILAN_TRY(make_plan(c, rows, k, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.total, MILAN_ERR_WORKSPACE,
                "milan_decoder_nll: workspace %zu < %zu bytes", ws_bytes, p.total);
  MILAN_TRY(check_params((const void* const*)params, n_params, "parameter"));
  return forward(p, params, (float*)ws, features, targets, 0, 1.f, 0, loss_terms,
                 (hipStream_t)stream);
}

int milan_decoder_train_step(milan_ctx* c, const float* const* params, float* const* grads,
                             int n_params, const float* features, const int64_t* targets,
                             int rows, int k, int L, float dropout, uint64_t seed,
                             float regularization_weight, float* loss_terms, void* ws,
                             size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(features && targets && loss_terms && ws, MILAN_ERR_ARG,
                "milan_decoder_train_step: null argument");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_decoder_train_step: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, k, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.total, MILAN_ERR_WORKSPACE,
                "milan_decoder_train_step: workspace %zu < %zu bytes", ws_bytes, p.total);
  MILAN_TRY(check_params((const void* const*)params, n_params, "parameter"));
  MILAN_TRY(check_params((const void* const*)grads, n_params, "gradient"));
  const uint32_t thr = drop_threshold(dropout);
  const float scale = drop_scale(dropout);
  const hipStream_t s = (hipStream_t)stream;
  MILAN_TRY(forward(p, params, (float*)ws, features, targets, thr, scale, seed, loss_terms, s));
  return backward(p, params, grads, (float*)ws, features, targets, thr, scale, seed,
                  regularization_weight, loss_terms, nullptr, s);
}

size_t milan_decoder_grad_workspace_bytes(const milan_ctx* c, int rows, int k, int L) {
  Plan p;
  if (make_plan(c, rows, k, L, &p) != 0) return 0;
  return p.grad_total;
}

int milan_decoder_forward_train(milan_ctx* c, const float* const* params, int n_params,
                                const float* features, const int64_t* targets, int rows, int k,
                                int L, float dropout, uint64_t seed, float* logprobs_out,
                                float* attentions_out, void* ws, size_t ws_bytes,
                                milan_stream stream) {
  MILAN_REQUIRE(features && targets && logprobs_out && attentions_out && ws, MILAN_ERR_ARG,
                "milan_decoder_forward_train: null argument");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_decoder_forward_train: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, k, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.grad_total, MILAN_ERR_WORKSPACE,
                "milan_decoder_forward_train: workspace %zu < %zu bytes", ws_bytes, p.grad_total);
  MILAN_TRY(check_params((const void* const*)params, n_params, "parameter"));
  const uint32_t thr = drop_threshold(dropout);
  const float scale = drop_scale(dropout);
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  MILAN_TRY(forward(p, params, w, features, targets, thr, scale, seed, w + p.terms, s));
  launch_logprobs(w + p.logits, w + p.lse, logprobs_out, p.N, p.V, s);
  MILAN_CHECK_HIP(hipGetLastError());
  MILAN_CHECK_HIP(hipMemcpyAsync(attentions_out, w + p.alpha, (size_t)p.N * k * sizeof(float),
                                 hipMemcpyDeviceToDevice, s));
  return 0;
}

int milan_decoder_backward(milan_ctx* c, const float* const* params, float* const* grads,
                           int n_params, const float* features, const int64_t* targets, int rows,
                           int k, int L, float dropout, uint64_t seed, const float* dlogprobs,
                           const float* dattentions, float* dfeatures, void* ws, size_t ws_bytes,
                           milan_stream stream) {
  MILAN_REQUIRE(features && targets && ws, MILAN_ERR_ARG, "milan_decoder_backward: null argument");
  MILAN_REQUIRE(dropout >= 0.f && dropout < 1.f, MILAN_ERR_ARG,
                "milan_decoder_backward: dropout %g not in [0, 1)", (double)dropout);
  Plan p;
  MILAN_TRY(make_plan(c, rows, k, L, &p));
  MILAN_REQUIRE(ws_bytes >= p.grad_total, MILAN_ERR_WORKSPACE,
                "milan_decoder_backward: workspace %zu < %zu bytes", ws_bytes, p.grad_total);
  MILAN_TRY(check_params((const void* const*)params, n_params, "parameter"));
  MILAN_TRY(check_params((const void* const*)grads, n_params, "gradient"));
  const uint32_t thr = drop_threshold(dropout);
  const float scale = drop_scale(dropout);
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  // dlogits into the logits buffer, where backward() expects them
  launch_log_softmax_bwd(dlogprobs, nullptr, nullptr, w + p.logits, w + p.lse, p.N, p.V, s);
  MILAN_CHECK_HIP(hipGetLastError());
  const Upstream up{dattentions, dfeatures ? w + p.dctx : nullptr};
  MILAN_TRY(backward(p, params, grads, w, features, targets, thr, scale, seed, 0.f, nullptr, &up,
                     s));
  if (!dfeatures) return 0;
  // dF = (dKh . W_k + sum_t alpha_t dctx_t) + (dph . W_init_h + dpc . W_init_c) / k
  const Scratch gsc{w + p.gscratch, p.gscratch_floats};
  const View none = view(nullptr, 0), dpool = view(w + p.dpool, p.F);
  MILAN_TRY(gemm(view(w + p.dkh, p.A), 0, view(params[P_K_W], p.F), 0, view(dfeatures, p.F), none,
                 nullptr, nullptr, rows * k, p.F, p.A, gsc, s));
  MILAN_TRY(gemm(view(w + p.dph, p.H), 0, view(params[P_INIT_H_W], p.F), 0, dpool, none, nullptr,
                 nullptr, rows, p.F, p.H, gsc, s));
  MILAN_TRY(gemm(view(w + p.dpc, p.H), 0, view(params[P_INIT_C_W], p.F), 0, dpool, dpool, nullptr,
                 nullptr, rows, p.F, p.H, gsc, s));
  hipLaunchKernelGGL(dfeat_kernel, dim3(blocks_for((long)rows * k * p.F)), dim3(256), 0, s,
                     w + p.alpha, w + p.dctx, w + p.dpool, dfeatures, rows, L, k, p.F);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
