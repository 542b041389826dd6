// The parts the transformer towers share (tower_common.h): the row kernels, the attention
// kernel that holds a whole head in LDS, and the weight store.
//
// Precision: exact fp32.  Determinism: fixed reduction orders, no float atomics.
#include "tower_common.h"

#include <string.h>

namespace milan {
namespace tower {

constexpr int ATT_THREADS = 256;

// Renormalise (x * mul[c] + add[c], the reference's Renormalizer) and gather the stride-P
// patches: A[(img * G + gy) * G + gx][(c * P + py) * P + px], the im2col of conv1.
__global__ void patch_gather_kernel(const float* __restrict__ images, float* __restrict__ A,
                                    long total, int R, int P, int G, float m0, float m1,
                                    float m2, float a0, float a1, float a2, int renorm) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int kk = 3 * P * P;
  const int col = (int)(i % kk);
  const long row = i / kk;
  const int px = col % P, py = (col / P) % P, c = col / (P * P);
  const int gx = (int)(row % G), gy = (int)((row / G) % G);
  const long img = row / ((long)G * G);
  float v = images[((img * 3 + c) * R + (gy * P + py)) * (long)R + gx * P + px];
  if (renorm) {
    const float mul = c == 0 ? m0 : (c == 1 ? m1 : m2);
    const float add = c == 0 ? a0 : (c == 1 ? a1 : a2);
    v = v * mul + add;
  }
  A[i] = v;
}

// dst[r] = LayerNorm(src[r * stride .. + W]); one wave per row.
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ src,
                                                         long stride, float* __restrict__ dst,
                                                         int rows, int W,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ b, float eps) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* row = src + (long)r * stride;
  ln_row([&](int j) { return row[j]; }, W, eps, w, b, dst + (long)r * W, lane);
}

// x <- x * 0.5 * (1 + erf(x / sqrt(2)))
__global__ void gelu_erf_kernel(float* __restrict__ x, long total) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float v = x[i];
  x[i] = v * 0.5f * (1.f + erff(v * 0.70710678118654752440f));
}

// y[r] = normalize ? x[r] / ||x[r]|| : x[r]   (one wave per row)
__global__ __launch_bounds__(256) void l2norm_kernel(const float* __restrict__ x,
                                                      float* __restrict__ y, int rows, int W,
                                                      int normalize) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* row = x + (long)r * W;
  float nrm = 1.f;
  if (normalize) {
    float q = 0.f;
    for (int j = lane; j < W; j += 64) q += row[j] * row[j];
    nrm = sqrtf(wave_sum(q));
  }
  for (int j = lane; j < W; j += 64) y[(long)r * W + j] = row[j] / nrm;
}

// One workgroup per (sequence, head).  Q / sqrt(hd), K, V of the head live in LDS (rows padded
// to hd + 1 floats: lanes that walk the keys hit distinct banks); wave w owns query rows w,
// w + 4, ...: lanes walk the keys for the scores and the softmax, then the head's columns for
// P V.  The sequence's rows and length come from `offsets` (RAGGED) or from the uniform T.
// One body behind two entry points, below, each with the arguments its tower had before the
// body was shared: what an entry passes as a constant folds away.
template <bool RAGGED>
__device__ __forceinline__ void lds_attention(
    const float* __restrict__ qkv, const int32_t* __restrict__ offsets, float* __restrict__ out,
    int T, int W, int hd, int max_len, int causal, const float* __restrict__ cls_mask, int n_img,
    int n_masked) {
  extern __shared__ float lds[];
  const int seq = blockIdx.x, head = blockIdx.y;
  size_t row0 = (size_t)seq * T;
  if (RAGGED) {
    row0 = offsets[seq];
    T = offsets[seq + 1] - offsets[seq];
    T = T < 0 ? 0 : (T > max_len ? max_len : T);  // memory safety only; the host validates
  }
  const int ldh = hd + 1;
  float* Q = lds;
  float* K = Q + (size_t)T * ldh;
  float* V = K + (size_t)T * ldh;
  float* P = V + (size_t)T * ldh;  // [4][T]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* base = qkv + row0 * 3 * W + (size_t)head * hd;
  const float qs = sqrtf((float)hd);
  for (int i = tid; i < T * hd; i += ATT_THREADS) {
    const int t = i / hd, d = i % hd;
    const float* p = base + (size_t)t * 3 * W + d;
    Q[t * ldh + d] = p[0] / qs;
    K[t * ldh + d] = p[W];
    V[t * ldh + d] = p[2 * W];
  }
  __syncthreads();
  const float* cm = (cls_mask && seq < n_masked)
                        ? cls_mask + (size_t)(seq % n_img) * (T - 1)
                        : nullptr;
  float* Pw = P + (size_t)w * T;
  for (int i = w; i < T; i += 4) {
    const int nk = causal ? i + 1 : T;
    const float* q = Q + i * ldh;
    float mx = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
      const float* k = K + j * ldh;
      float sc = 0.f;
      for (int d = 0; d < hd; ++d) sc += q[d] * k[d];
      Pw[j] = sc;
      mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
      const float e = expf(Pw[j] - mx);
      Pw[j] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    for (int j = lane; j < nk; j += 64) {
      float p = Pw[j] / sum;
      if (cm && i == 0 && j >= 1) p *= cm[j - 1];
      Pw[j] = p;
    }
    // (the lanes of one wave wrote Pw; the wave reads it back below)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int d = lane; d < hd; d += 64) {
      float o = 0.f;
      for (int j = 0; j < nk; ++j) o += Pw[j] * V[j * ldh + d];
      out[(row0 + i) * W + (size_t)head * hd + d] = o;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
}

// Ragged, bidirectional, no mask edit (BERT).
__global__ __launch_bounds__(ATT_THREADS) void lds_attention_ragged_kernel(
    const float* __restrict__ qkv, const int32_t* __restrict__ offsets, float* __restrict__ out,
    int W, int hd, int max_len) {
  lds_attention<true>(qkv, offsets, out, 0, W, hd, max_len, 0, nullptr, 1, 0);
}

// Uniform T, with the causal flag and the CLS-row edit (CLIP).
__global__ __launch_bounds__(ATT_THREADS) void lds_attention_kernel(
    const float* __restrict__ qkv, float* __restrict__ out, int T, int W, int hd, int causal,
    const float* __restrict__ cls_mask, int n_img, int n_masked) {
  lds_attention<false>(qkv, nullptr, out, T, W, hd, T, causal, cls_mask, n_img, n_masked);
}

// ---- host side ------------------------------------------------------------------------------
int launch_patch_gather(const float* images, float* A, long n, int R, int P,
                        const float* renorm_mul_add, hipStream_t s) {
  const int G = R / P;
  const long total = n * G * G * 3 * P * P;
  if (total <= 0) return 0;
  float ma[6] = {1.f, 1.f, 1.f, 0.f, 0.f, 0.f};
  if (renorm_mul_add) memcpy(ma, renorm_mul_add, sizeof(ma));  // HOST floats
  hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks_for(total)), dim3(256), 0, s, images, A,
                     total, R, P, G, ma[0], ma[1], ma[2], ma[3], ma[4], ma[5],
                     renorm_mul_add ? 1 : 0);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_layernorm_rows(const float* src, long stride, float* dst, int rows, int W,
                          const float* w, const float* b, float eps, hipStream_t s) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(layernorm_kernel, dim3(blocks_for(rows, 4)), dim3(256), 0, s, src, stride,
                     dst, rows, W, w, b, eps);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_gelu_erf(float* x, long total, hipStream_t s) {
  if (total <= 0) return 0;
  hipLaunchKernelGGL(gelu_erf_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, total);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int launch_l2norm(const float* x, float* y, int rows, int W, int normalize, hipStream_t s) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(l2norm_kernel, dim3(blocks_for(rows, 4)), dim3(256), 0, s, x, y, rows, W,
                     normalize);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// (ensure_lds_attr only ever raises a kernel's limit, so callers with different lengths may
// come in any order)
int launch_lds_attention(const LdsAttention& a, long seqs, int heads, hipStream_t s) {
  MILAN_REQUIRE(!a.offsets || (!a.causal && !a.cls_mask), MILAN_ERR_ARG,
                "lds attention: ragged sequences have no causal or mask-edit form");
  const size_t lds = lds_attention_bytes(a.max_len, a.hd);
  const dim3 grid((unsigned)seqs, heads);
  if (a.offsets) {
    MILAN_TRY(ensure_lds_attr((const void*)lds_attention_ragged_kernel, (int)lds));
    hipLaunchKernelGGL(lds_attention_ragged_kernel, grid, dim3(ATT_THREADS), lds, s, a.qkv,
                       a.offsets, a.out, a.W, a.hd, a.max_len);
  } else {
    MILAN_TRY(ensure_lds_attr((const void*)lds_attention_kernel, (int)lds));
    hipLaunchKernelGGL(lds_attention_kernel, grid, dim3(ATT_THREADS), lds, s, a.qkv, a.out, a.T,
                       a.W, a.hd, a.causal, a.cls_mask, a.n_img, a.n_masked);
  }
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- weights ----------------------------------------------------------------------------------
int Weights::set(const char* what, const char* name, const float* data, const int64_t* shape,
                 int ndim) {
  MILAN_REQUIRE(name && data && (shape || ndim == 0) && ndim >= 0 && ndim <= 8, MILAN_ERR_ARG,
                "milan_%s_set_weight: bad argument", what);
  MILAN_REQUIRE(!finalized, MILAN_ERR_STATE,
                "milan_%s_set_weight after milan_%s_finalize_weights", what, what);
  Tensor t;
  t.shape.assign(shape, shape + ndim);
  t.dev = data;
  raw[name] = t;
  return 0;
}

// The uploaded tensor `name` of `count` elements, or nullptr with the error set.
static const float* find(const char* what, const std::map<std::string, Tensor>& raw,
                         const std::string& name, size_t count) {
  auto it = raw.find(name);
  if (it == raw.end()) {
    set_error("%s: weight %s was not uploaded", what, name.c_str());
    return nullptr;
  }
  size_t n = 1;
  for (int64_t v : it->second.shape) n *= (size_t)v;
  if (n != count) {
    set_error("%s: weight %s has %zu elements, the dims need %zu", what, name.c_str(), n, count);
    return nullptr;
  }
  return (const float*)it->second.dev;
}

int Weights::finalize(const char* what, const std::vector<Want>& wants, hipStream_t s) {
  MILAN_REQUIRE(!finalized, MILAN_ERR_STATE, "%s weights already finalized", what);
  MILAN_CHECK_HIP(hipSetDevice(device));
  size_t total = 0;
  for (auto& w : wants) {
    if (!find(what, raw, w.name, w.count)) return MILAN_ERR_STATE;
    total += up64(w.count);
  }
  MILAN_CHECK_HIP(hipMalloc((void**)&arena, total * sizeof(float)));
  size_t o = 0;
  for (auto& w : wants) {
    MILAN_CHECK_HIP(hipMemcpyAsync(arena + o, find(what, raw, w.name, w.count),
                                   w.count * sizeof(float), hipMemcpyDeviceToDevice, s));
    *w.dst = arena + o;
    o += up64(w.count);
  }
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  raw.clear();
  finalized = true;
  return 0;
}

void Weights::release() {
  (void)hipSetDevice(device);
  if (arena) (void)hipFree(arena);
  arena = nullptr;
}

}  // namespace tower
}  // namespace milan
