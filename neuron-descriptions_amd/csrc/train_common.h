// What lm_train.hip (LanguageModel.fit, LanguageModel.forward in training mode) and
// decoder_train.hip (Decoder.fit, Decoder.forward in training mode) share: the dropout hash,
// the small device and host inlines, the workspace-offset helper, and host launchers of the
// kernels both run (embedding gather and gradient, dropout, the LSTM cell, log-softmax) with
// the output layer as two host helpers.  The kernels are defined once, in lm_train.hip.  The
// contraction is the strided exact-fp32 GEMM of tgemm.h.
#pragma once
#include "tgemm.h"
#include "wave.h"

namespace milan {
namespace train {

using tgemm::colsum;
using tgemm::colsum_chunks;
using tgemm::gemm;
using tgemm::Scratch;
using tgemm::split_scratch_floats;
using tgemm::View;
using tgemm::view;
using wave::wave_sum;

// ---- dropout mask: a pure function of (seed, tag, row, t, unit) ----------------------------
// keep  <=>  (mix64(seed ^ mix64(key)) >> 40) >= thr,   thr = (uint32)(p * 2^24),
// key = tag << 56 | row << 32 | t << 16 | unit  (splitmix64 finaliser; restated on the host
// by milan_amd.lms.tagged_dropout_mask).  The LM's tag is the layer whose output is dropped,
// the decoder's is kDecoderDropoutTag, above every LM layer.
constexpr int kDecoderDropoutTag = 0xDC;
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ bool keep(uint64_t seed, int tag, int row, int t, int unit,
                                     uint32_t thr) {
  const uint64_t key = (uint64_t)tag << 56 | (uint64_t)row << 32 | (uint64_t)t << 16 |
                       (uint64_t)unit;
  return (uint32_t)(mix64(seed ^ mix64(key)) >> 40) >= thr;
}
static inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 16777216.0); }
static inline float drop_scale(float p) { return p > 0.f ? 1.f / (1.f - p) : 1.f; }

__device__ __forceinline__ int clamp_id(int64_t id, int V) {
  return id < 0 ? 0 : (id >= V ? V - 1 : (int)id);
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

static inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

// Workspace offsets in floats: take() gives the next 64-float-aligned block, need() keeps the
// largest scratch any one GEMM or column sum asks for.
struct Layout {
  size_t off = 0, scratch = 0;
  size_t take(size_t floats) {
    const size_t at = off;
    off += (floats + 63) / 64 * 64;
    return at;
  }
  void need(size_t floats) { scratch = floats > scratch ? floats : scratch; }
};

// ---- kernels both trainers run ---------------------------------------------------------------
// x[n * x_rs + e] = embedding[ids[n]][e] for e < E  (ids clamped into [0, V): memory safety
// only, the Python side validates them)
void launch_embed(const int64_t* ids, const float* emb, float* x, int N, int E, long x_rs, int V,
                  hipStream_t s);
// dEmb[v] = sum over positions n with ids[n] == v of dX[n] (row stride E), in position order;
// row `pad` is exactly zero (pad < 0: no such row)
void launch_embed_grad(const int64_t* ids, const float* dX, int N, int E, int V, int pad,
                       float* dEmb, hipStream_t s);

// X[b][t][j] = dropout(h_{t+1}), h_{t+1} = slot t + 1 of Hs [rows][L + 1][H]: h * mask * scale
// (thr == 0: a copy)
void launch_dropout_fwd(const float* Hs, float* X, int rows, int L, int H, int tag, uint64_t seed,
                        uint32_t thr, float scale, hipStream_t s);
// dY[b][t][j] *= mask * scale (the same mask)
void launch_dropout_bwd(float* dY, int rows, int L, int H, int tag, uint64_t seed, uint32_t thr,
                        float scale, hipStream_t s);

// One LSTM cell step t (torch gate order i, f, g, o).  G [rows * L][4H]: pre-activations of
// step t in, activated gates out.  c_{t-1} is cprev[b * c_rs + j] (cprev null: zero), c_t goes
// to cout[b * c_rs + j], h_t to slot t + 1 of Hs [rows][L + 1][H].
void launch_cell_fwd(float* G, const float* cprev, float* cout, long c_rs, float* Hs, int rows,
                     int L, int H, int t, hipStream_t s);
// Backward of cell step t.  dL/dh_t = dh[b * dh_rs + j], plus dhrec[b * H + j] when dhrec is
// given and t < L - 1 (dhrec null: dh is already the sum).  G: activated gates in,
// d(pre-activation) out.  ccur / cprev as in the forward.  dc [rows][H]: dL/dc_t in (ignored
// at t = L - 1), dL/dc_{t-1} out.
void launch_cell_bwd(const float* dh, long dh_rs, const float* dhrec, float* G, const float* ccur,
                     const float* cprev, long c_rs, float* dc, int rows, int L, int H, int t,
                     hipStream_t s);

// out[n][v] = logits[n][v] - lse[n]
void launch_logprobs(const float* logits, const float* lse, float* out, int N, int V,
                     hipStream_t s);
// Log-softmax backward in place over the logits, from upstream gradients of the log-probs,
// G [N][V], and of the picked log-probs, gp [N] with their targets (either null: zero)
void launch_log_softmax_bwd(const float* G, const float* gp, const int64_t* tgt, float* logits,
                            const float* lse, int N, int V, hipStream_t s);

// ---- the output layer: Linear(H, V) -> LogSoftmax -> NLLLoss(ignore_index = pad) -----------
struct OutLayer {
  int N, V, H, pad;
  float *logits, *lse, *term, *valid;  // [N][V], [N], [N], [N] of the workspace
};
template <typename Plan>  // (either trainer's plan: it names these dims and offsets alike)
static inline OutLayer out_layer(const Plan& p, float* ws) {
  return {p.N, p.V, p.H, p.pad, ws + p.logits, ws + p.lse, ws + p.term, ws + p.valid};
}
// logits = h_out . W_out^T + b_out; per row the lse, -log p(target) (0 for pad) and the valid
// flag; loss[0] = sum of the terms, loss[1] = number of valid targets (one workgroup)
int output_forward(const OutLayer& o, View h_out, const float* w_out, const float* b_out,
                   const int64_t* targets, float* loss, Scratch sc, hipStream_t s);
// loss given: logits <- (softmax - onehot(target)) * valid / loss[1] first (loss null: the
// logits buffer already holds dlogits).  Then dW_out = dlogits^T . h_out, db_out = the column
// sums of dlogits, dY [N][H] = dlogits . W_out.
int output_backward(const OutLayer& o, View h_out, const float* w_out, const int64_t* targets,
                    const float* loss, float* dw_out, float* db_out, float* dY, Scratch sc,
                    hipStream_t s);

}  // namespace train
}  // namespace milan
