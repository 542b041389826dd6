// What the transformer towers share (clip.hip, bert.hip, vit.hip): the wave reductions and
// the LayerNorm row as device inlines, the row kernels and the LDS attention kernel behind
// host launchers, and the weight store of a tower context.  Kernels and the store are defined
// once, in tower.hip.  Each tower keeps its own block walk and workspace plan.  The towers'
// contraction is the strided exact-fp32 GEMM of tgemm.h; the wave reductions are wave.h's.
#pragma once
#include "tgemm.h"
#include "wave.h"

namespace milan {
namespace tower {

// ---- device inlines ---------------------------------------------------------------------------
using wave::wave_max;
using wave::wave_sum;

// Two-pass LayerNorm of one row held by one wave (mean, then the centred second moment, as
// torch's CPU kernel); `in(j)` gives element j.
template <typename In>
__device__ __forceinline__ void ln_row(In in, int W, float eps, const float* w, const float* b,
                                       float* dst, int lane) {
  float s = 0.f;
  for (int j = lane; j < W; j += 64) s += in(j);
  const float mean = wave_sum(s) / (float)W;
  float q = 0.f;
  for (int j = lane; j < W; j += 64) {
    const float d = in(j) - mean;
    q += d * d;
  }
  const float rstd = 1.f / sqrtf(wave_sum(q) / (float)W + eps);
  for (int j = lane; j < W; j += 64) dst[j] = (in(j) - mean) * rstd * w[j] + b[j];
}

// ---- host inlines -----------------------------------------------------------------------------
static inline unsigned blocks_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
static inline size_t up64(size_t v) { return (v + 63) / 64 * 64; }

// ---- row kernels ------------------------------------------------------------------------------
// The stride-P patches of n (3, R, R) images as the rows of conv1's im2col:
// A[(img * G + gy) * G + gx][(c * P + py) * P + px], G = R / P.  renorm_mul_add (HOST, 6
// floats: mul[3], add[3]) or nullptr: x * mul[c] + add[c] first.
int launch_patch_gather(const float* images, float* A, long n, int R, int P,
                        const float* renorm_mul_add, hipStream_t s);

// dst[r][:] = LayerNorm(src[r * stride .. + W]; w, b, eps), biased variance, one wave per row.
int launch_layernorm_rows(const float* src, long stride, float* dst, int rows, int W,
                          const float* w, const float* b, float eps, hipStream_t s);

// x <- x * 0.5 * (1 + erf(x / sqrt(2))), in place.
int launch_gelu_erf(float* x, long total, hipStream_t s);

// y[r] = normalize ? x[r] / ||x[r]|| : x[r], rows of W floats, one wave per row.
int launch_l2norm(const float* x, float* y, int rows, int W, int normalize, hipStream_t s);

// ---- attention with a whole head in LDS -------------------------------------------------------
// softmax(q k^T / sqrt(hd)) v, one workgroup per (sequence, head).
// qkv: [rows][3 W] (q | k | v, heads contiguous inside each), out: [rows][W].
// Ragged sequences are bidirectional and unedited: `offsets` with `causal` or `cls_mask` is
// MILAN_ERR_ARG.
struct LdsAttention {
  const float* qkv;
  float* out;
  const int32_t* offsets;  // ragged: sequence s is rows offsets[s] .. offsets[s + 1]; or nullptr:
  int T;                   // uniform: sequence s is rows s * T .. (s + 1) * T
  int max_len;             // the longest sequence (T when uniform): sizes the LDS
  int W, hd;
  int causal;              // keys j > i are excluded (the text tower's additive -inf mask)
  // After the softmax, P[0][j] *= cls_mask[s % n_img][j - 1] for j >= 1, for sequences s <
  // n_masked only; not renormalised (rerankers.py:203-214).  nullptr: no edit.
  const float* cls_mask;
  int n_img, n_masked;
};
constexpr size_t LDS_LIMIT = 64 * 1024;
static inline size_t lds_attention_bytes(int T, int hd) {
  return sizeof(float) * (3 * (size_t)T * (hd + 1) + 4 * (size_t)T);
}
static inline bool lds_attention_fits(int T, int hd) {
  return lds_attention_bytes(T, hd) <= LDS_LIMIT;
}
int launch_lds_attention(const LdsAttention& a, long seqs, int heads, hipStream_t s);

// ---- weights ----------------------------------------------------------------------------------
// The tensors of a state dict, by name, until finalize() copies the wanted ones into one device
// arena (in the order of `wants`, each at a 64-float boundary).  `what` ("clip", "bert",
// "vit") names the tower in the error texts.
struct Want {
  std::string name;
  size_t count;
  const float** dst;
};
struct Weights {
  int device = 0;
  bool finalized = false;
  std::map<std::string, Tensor> raw;
  float* arena = nullptr;

  int set(const char* what, const char* name, const float* data, const int64_t* shape, int ndim);
  int finalize(const char* what, const std::vector<Want>& wants, hipStream_t s);
  void release();
};

}  // namespace tower
}  // namespace milan
