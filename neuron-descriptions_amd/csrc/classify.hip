// Unit ablation, classification and activation taps on the ResNet trunks (milan_set_ablation,
// milan_classify, milan_classify_sweep, milan_activations): the reference's
// src/utils/ablations.py on torchvision's ResNet._forward_impl, eval mode.
//
// The forward is a plain walker of its own: stem conv, bn1 + ReLU + maxpool, every block's convs
// through launch_gemm with the epilogues the encoder uses, then the head.  It materialises the
// five tensors an edit must see -- the raw conv1 output (level 0: nethook edits the module's
// output, before bn1) and the post-ReLU output of every stage (levels 1..4) -- and multiplies
// each by the context's 0/1 channel mask before anything reads it.  None of the encoder's fused
// launches (chain, fused stem, conv-front, row lists) is used: those are the paths that never
// write such a tensor.
//
// Head: pooled[c] = (sum over pixels p = 0 .. h*w-1, ascending, one fp32 add
// each) / (h*w); logit[j] = bias[j] + sum_k pooled[k] * W[j][k] with lane l of one wavefront
// accumulating k = l, l + 64, ... by fmaf and the 64 partial sums folded by a butterfly
// (lane ^ 32, 16, 8, 4, 2, 1).  Neither depends on the batch size or on the grid.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace milan {

typedef float cf32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned cu32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 cf16x8_t __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__global__ void fill_ones_kernel(float* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.f;
}

// y = x * mask[channel], NHWC fp32, one float4 (4 channels) per lane; `extra` >= 0 zeroes that
// channel as well (the sweep's copy-and-mask: x = the held tensor, y = the working tensor).
// x == y is the in-place form.  The product is the reference's `features * mask`.
__global__ void channel_mask_f32_kernel(const cf32x4_t* x, cf32x4_t* y, long total4, int C4,
                                        const cf32x4_t* __restrict__ mask, int extra) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total4;
       i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    cf32x4_t m = mask[c4];
    if ((extra >> 2) == c4 && extra >= 0) m[extra & 3] = 0.f;
    y[i] = x[i] * m;
  }
}

// the same on the split (hi, lo) format: one 8-channel group [hi x8 | lo x8] per lane, two
// 16-byte loads and stores; a masked channel's two f16 halves become +0 (split values are
// finite and, after a ReLU, non-negative: the product with 0 is +0 as well)
__global__ void channel_mask_split_kernel(const float* x, float* y, long groups, int G,
                                          const float* __restrict__ mask, int extra) {
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < groups;
       q += (long)gridDim.x * blockDim.x) {
    const int g = (int)(q % G);
    const cf32x4_t m0 = *reinterpret_cast<const cf32x4_t*>(mask + g * 8);
    const cf32x4_t m1 = *reinterpret_cast<const cf32x4_t*>(mask + g * 8 + 4);
    cu32x4_t keep;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int e0 = 2 * d, e1 = 2 * d + 1;
      const float k0 = e0 < 4 ? m0[e0] : m1[e0 - 4], k1 = e1 < 4 ? m0[e1] : m1[e1 - 4];
      const bool on0 = k0 != 0.f && g * 8 + e0 != extra, on1 = k1 != 0.f && g * 8 + e1 != extra;
      keep[d] = (on0 ? 0x0000ffffu : 0u) | (on1 ? 0xffff0000u : 0u);
    }
    const cu32x4_t hi = *reinterpret_cast<const cu32x4_t*>(x + q * 8);
    const cu32x4_t lo = *reinterpret_cast<const cu32x4_t*>(x + q * 8 + 4);
    *reinterpret_cast<cu32x4_t*>(y + q * 8) = hi & keep;
    *reinterpret_cast<cu32x4_t*>(y + q * 8 + 4) = lo & keep;
  }
}

// global average pool (n, P, C) -> (n, C): a thread per (image, channel), pixels in ascending
// order, then one division.  SPLIT: the value is (float(hi) + float(lo)) * inv_scale, the
// activation scale (a power of two) removed exactly before the sum.
template <bool SPLIT>
__global__ __launch_bounds__(256) void avgpool_kernel(const float* __restrict__ x, int P, int C,
                                                      float inv_scale, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const long img = blockIdx.y;
  if (c >= C) return;
  float sum = 0.f;
  for (int p = 0; p < P; ++p) {
    const float* row = x + (img * P + p) * C;
    float v;
    if constexpr (SPLIT) {
      const _Float16* g = reinterpret_cast<const _Float16*>(row + (c >> 3) * 8);
      v = ((float)g[c & 7] + (float)g[8 + (c & 7)]) * inv_scale;
    } else {
      v = row[c];
    }
    sum += v;
  }
  out[img * C + c] = sum / (float)P;
}

// Activation tap (milan_activations): a level tensor (n, P, C) in the trunk's layout -> fp32
// (n, C, P), the NCHW tensor the exemplar kernels read.  One workgroup moves a tile of
// TAP_P pixels x TAP_C channels through LDS: the global reads are 16-byte pieces contiguous
// along C (one float4, or one [hi x8 | lo x8] group = two pieces), the global writes run
// along P, one wavefront per 256-byte run.  LDS rows are pixels, padded by one dword: the
// writes of a 32-lane half (c-piece fastest, then pixel) and the column reads (lane = pixel)
// both land on 32 distinct banks.  fp32: a copy of the value, except that -0 becomes +0.
// SPLIT: the value is (float(hi) + float(lo)) * inv_scale, avgpool_kernel's decode.  Both
// tile edges are guarded (P is anything >= 1, C a multiple of 8).
// grid (ceil(P / TAP_P), ceil(C / TAP_C), n).
constexpr int TAP_P = 64, TAP_C = 32, TAP_LD = TAP_C + 1;
template <bool SPLIT>
__global__ __launch_bounds__(256) void tap_nchw_kernel(const float* __restrict__ x, int P, int C,
                                                       float inv_scale, float* __restrict__ out) {
  __shared__ float tile[TAP_P * TAP_LD];
  const int t = threadIdx.x;
  const int p0 = blockIdx.x * TAP_P, c0 = blockIdx.y * TAP_C;
  const size_t img = blockIdx.z;
  const float* src = x + img * (size_t)P * C;
  if constexpr (SPLIT) {
    // 4 groups of 8 channels per pixel: one group per thread
    const int g = t & 3, p = t >> 2;
    const int c = c0 + g * 8;
    if (p0 + p < P && c < C) {
      const float* q = src + (size_t)(p0 + p) * C + c;
      const cf16x8_t hi = *reinterpret_cast<const cf16x8_t*>(q);
      const cf16x8_t lo = *reinterpret_cast<const cf16x8_t*>(q + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        tile[p * TAP_LD + g * 8 + e] = ((float)hi[e] + (float)lo[e]) * inv_scale;
    }
  } else {
    // 8 float4 per pixel: 32 pixels per pass, two passes.  A zero leaves as +0: the raw conv1
    // tensor has negative values, and the mask's product with one of them is -0.
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int c4 = t & 7, p = (t >> 3) + r * 32;
      const int c = c0 + c4 * 4;
      if (p0 + p < P && c < C) {
        const cf32x4_t v = *reinterpret_cast<const cf32x4_t*>(src + (size_t)(p0 + p) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[p * TAP_LD + c4 * 4 + e] = v[e] == 0.f ? 0.f : v[e];
      }
    }
  }
  __syncthreads();
  // wavefront w writes channels w*8 .. w*8+7, lane = pixel
  const int lane = t & 63, wv = t >> 6;
  if (p0 + lane < P) {
    float* dst = out + img * (size_t)C * P + (size_t)p0 + lane;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cc = wv * 8 + k;
      if (c0 + cc < C) dst[(size_t)(c0 + cc) * P] = tile[lane * TAP_LD + cc];
    }
  }
}

// logits[img][j] = bias[j] + pooled[img] . W[j], exact fp32, one wavefront per output (see the
// file comment for the order); 4 outputs per workgroup, grid (ceil(classes / 4), n)
__global__ __launch_bounds__(256) void fc_kernel(const float* __restrict__ pooled,
                                                 const float* __restrict__ W,
                                                 const float* __restrict__ bias, int K,
                                                 int classes, float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const long img = blockIdx.y;
  if (j >= classes) return;   // (whole wavefronts leave: the shuffles below stay converged)
  const float* p = pooled + img * K;
  const float* w = W + (long)j * K;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = __fmaf_rn(p[k], w[k], acc);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) logits[img * classes + j] = acc + (bias ? bias[j] : 0.f);
}

// torch.argmax's rule: a NaN counts as the maximum, the lowest index among equals wins
__device__ __forceinline__ bool argmax_better(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a > b || (a == b && ia < ib);
}
__global__ __launch_bounds__(64) void row_argmax_kernel(const float* __restrict__ logits,
                                                        int classes, long long* __restrict__ out) {
  const long row = blockIdx.x;
  const float* x = logits + row * classes;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = threadIdx.x; j < classes; j += 64)
    if (argmax_better(x[j], j, best, bi)) { best = x[j]; bi = j; }
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (argmax_better(ob, oi, best, bi)) { best = ob; bi = oi; }
  }
  if (threadIdx.x == 0) out[row] = bi;
}

// correct[j] = #{i : predictions[j][i] == targets[i]}: one workgroup per swept unit, integer
// partial counts folded in a fixed order, one plain vector store
__global__ __launch_bounds__(256) void correct_count_kernel(const long long* __restrict__ pred,
                                                            const long long* __restrict__ targets,
                                                            int n, int* __restrict__ correct) {
  __shared__ int part[4];
  const long long* row = pred + (long)blockIdx.x * n;
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += 256) cnt += row[i] == targets[i];
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) correct[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// ---------------------------------------------------------------------------
// weights and the ablation set
// ---------------------------------------------------------------------------
static bool resnet_trunk(const milan_ctx* c) {
  return c->d.trunk_kind == MILAN_TRUNK_BOTTLENECK || c->d.trunk_kind == MILAN_TRUNK_BASIC;
}
static int level_channels(const milan_ctx* c, int level) {
  const int wd = c->d.trunk_width;
  if (level == 0) return wd;
  return (c->d.trunk_kind == MILAN_TRUNK_BASIC ? wd : wd * 4) << (level - 1);
}

// called from milan_finalize_weights after encoder_finalize: keeps fc.weight / fc.bias when the
// state dict has them (a context without them runs everything but the classify calls)
int classify_finalize(milan_ctx* c, hipStream_t s) {
  if (!resnet_trunk(c) || c->stem.w == nullptr) return 0;
  int total = 0;
  for (int l = 0; l < 5; ++l) {
    c->abl_ch[l] = level_channels(c, l);
    c->abl_off[l] = total;
    total += c->abl_ch[l];
    c->abl_count[l] = 0;
  }
  MILAN_TRY(dev_alloc(c, (void**)&c->abl_mask, sizeof(float) * total));
  hipLaunchKernelGGL(fill_ones_kernel, dim3((total + 255) / 256), dim3(256), 0, s, c->abl_mask,
                     total);
  MILAN_CHECK_HIP(hipGetLastError());
  const std::string p = "encoder.encoder.model.";
  auto w = c->raw.find(p + "fc.weight");
  if (w == c->raw.end()) return 0;
  const Tensor& tw = w->second;
  MILAN_REQUIRE(tw.shape.size() == 2 && tw.shape[0] >= 1 && tw.shape[1] == c->abl_ch[4],
                MILAN_ERR_SHAPE, "fc.weight must be (classes, %d)", c->abl_ch[4]);
  c->fc_classes = (int)tw.shape[0];
  c->fc_in = (int)tw.shape[1];
  MILAN_TRY(dev_alloc(c, (void**)&c->fc_w, sizeof(float) * (size_t)tw.numel()));
  MILAN_CHECK_HIP(hipMemcpyAsync(c->fc_w, tw.dev, sizeof(float) * (size_t)tw.numel(),
                                 hipMemcpyDeviceToDevice, s));
  auto b = c->raw.find(p + "fc.bias");
  if (b != c->raw.end()) {
    MILAN_REQUIRE(b->second.numel() == c->fc_classes, MILAN_ERR_SHAPE,
                  "fc.bias must have %d entries", c->fc_classes);
    MILAN_TRY(dev_alloc(c, (void**)&c->fc_b, sizeof(float) * (size_t)c->fc_classes));
    MILAN_CHECK_HIP(hipMemcpyAsync(c->fc_b, b->second.dev, sizeof(float) * (size_t)c->fc_classes,
                                   hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

static int check_units(const milan_ctx* c, const int32_t* levels, const int32_t* units, int count,
                       const char* what) {
  for (int i = 0; i < count; ++i) {
    MILAN_REQUIRE(levels[i] >= 0 && levels[i] <= 4, MILAN_ERR_ARG,
                  "%s: level %d is not one of 0..4 (conv1, layer1..layer4)", what, levels[i]);
    MILAN_REQUIRE(units[i] >= 0 && units[i] < c->abl_ch[levels[i]], MILAN_ERR_INDEX,
                  "%s: index %d is out of bounds for level %d with %d units", what, units[i],
                  levels[i], c->abl_ch[levels[i]]);
  }
  return 0;
}

int classify_set_ablation(milan_ctx* c, const int32_t* levels, const int32_t* units, int count,
                          hipStream_t s) {
  MILAN_REQUIRE(resnet_trunk(c), MILAN_ERR_ARG, "unit ablation needs a ResNet trunk");
  MILAN_REQUIRE(c->abl_mask != nullptr, MILAN_ERR_STATE, "encoder weights were not uploaded");
  MILAN_TRY(check_units(c, levels, units, count, "milan_set_ablation"));
  const int total = c->abl_off[4] + c->abl_ch[4];
  std::vector<float> host((size_t)total, 1.f);
  int cnt[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < count; ++i) {
    float& m = host[(size_t)c->abl_off[levels[i]] + units[i]];
    if (m != 0.f) { m = 0.f; ++cnt[levels[i]]; }
  }
  // (the one call of this family that synchronises: `host` must outlive the copy)
  MILAN_CHECK_HIP(hipMemcpyAsync(c->abl_mask, host.data(), sizeof(float) * (size_t)total,
                                 hipMemcpyHostToDevice, s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  for (int l = 0; l < 5; ++l) c->abl_count[l] = cnt[l];
  return 0;
}

// ---------------------------------------------------------------------------
// driver
// ---------------------------------------------------------------------------
struct ClsPlan {
  int h[5], w[5];   // level 0 = conv1 output, 1 = after the maxpool / layer1, 2..4 = layer2..4
  size_t lvl_sz[5]; // floats per image of the level's tensor (split format takes the same room)
  float *in4, *raw, *x0, *x1, *ds, *t1, *t2, *hold, *work, *pooled, *logits;
  long long* preds;
};

static int cls_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

static void cls_plan(const milan_ctx* c, int n, int H, int W, int sweep_units, int n_total,
                     Arena& a, ClsPlan* pl) {
  const int wd = c->d.trunk_width;
  pl->h[0] = cls_out(H, 7, 2, 3); pl->w[0] = cls_out(W, 7, 2, 3);
  for (int l = 1; l < 5; ++l) {
    pl->h[l] = cls_out(pl->h[l - 1], 3, 2, 1);
    pl->w[l] = cls_out(pl->w[l - 1], 3, 2, 1);
  }
  // (levels 1: the maxpool's and layer1's output have the same extent)
  const int exp = c->d.trunk_kind == MILAN_TRUNK_BASIC ? 1 : 4;
  size_t x_sz = (size_t)pl->h[1] * pl->w[1] * wd, t1_sz = 0, t2_sz = 0, lvl_max = 0;
  for (int li = 0; li < 4; ++li) {
    const size_t planes = (size_t)wd << li;
    const size_t in_px = (size_t)pl->h[li == 0 ? 1 : li] * pl->w[li == 0 ? 1 : li];
    const size_t out_px = (size_t)pl->h[li + 1] * pl->w[li + 1];
    x_sz = std::max(x_sz, out_px * planes * exp);
    t1_sz = std::max(t1_sz, in_px * planes);
    t2_sz = std::max(t2_sz, out_px * planes);
  }
  for (int l = 0; l < 5; ++l) {
    pl->lvl_sz[l] = (size_t)pl->h[l] * pl->w[l] * level_channels(c, l);
    lvl_max = std::max(lvl_max, pl->lvl_sz[l]);
  }
  // (first, so that its address does not depend on the pass's image count)
  pl->preds = sweep_units > 0 ? a.get<long long>((size_t)sweep_units * n_total) : nullptr;
  pl->in4 = a.get<float>((size_t)n * H * (W + 2) * 4);
  pl->raw = a.get<float>((size_t)n * pl->lvl_sz[0]);
  pl->x0 = a.get<float>((size_t)n * x_sz);
  pl->x1 = a.get<float>((size_t)n * x_sz);
  pl->ds = a.get<float>((size_t)n * x_sz);
  pl->t1 = a.get<float>((size_t)n * t1_sz);
  pl->t2 = a.get<float>((size_t)n * t2_sz);
  pl->pooled = a.get<float>((size_t)n * level_channels(c, 4));
  pl->logits = a.get<float>((size_t)n * (c->fc_classes > 0 ? c->fc_classes : 1));
  pl->hold = pl->work = nullptr;
  if (sweep_units > 0) {
    pl->hold = a.get<float>((size_t)n * lvl_max);
    pl->work = a.get<float>((size_t)n * lvl_max);
  }
}

size_t classify_workspace(const milan_ctx* c, int n_images, int H, int W, int sweep_units) {
  if (!resnet_trunk(c) || n_images <= 0 || H < 1 || W < 1) return 0;
  Arena a; a.dry = true;
  const int sub = encoder_sub_batch_size();
  ClsPlan pl;
  cls_plan(c, n_images < sub ? n_images : sub, H, W, sweep_units < 0 ? 0 : sweep_units, n_images,
           a, &pl);
  return a.off;
}

static int grid_for(long items) {
  const long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b < 16384 ? b : 16384));
}

struct Walker {
  milan_ctx* c;
  const ClsPlan& pl;
  int n;
  bool split;
  hipStream_t s;

  // level tensor `x` -> `y` (x == y: in place), times the context's mask of that level and with
  // unit `extra` (>= 0) zeroed too
  int mask(int level, const float* x, float* y, int extra) const {
    const int C = c->abl_ch[level];
    const long px = (long)n * pl.h[level] * pl.w[level];
    const float* m = c->abl_mask + c->abl_off[level];
    if (split && level > 0) {
      const long groups = px * (C / 8);
      hipLaunchKernelGGL(channel_mask_split_kernel, dim3(grid_for(groups)), dim3(256), 0, s, x, y,
                         groups, C / 8, m, extra);
    } else {
      const long total4 = px * (C / 4);
      hipLaunchKernelGGL(channel_mask_f32_kernel, dim3(grid_for(total4)), dim3(256), 0, s,
                         (const cf32x4_t*)x, (cf32x4_t*)y, total4, C / 4, (const cf32x4_t*)m,
                         extra);
    }
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }

  // the masked level tensor `x` -> tap[level] as fp32 NCHW (milan_activations).  Level 0 is
  // the raw conv1 output: fp32 without any scale in both modes (the pair stem's weight scale
  // leaves in the GEMM's acc_scale, the activation scale enters only with bn1_scale_s).
  int emit(int level, const float* x) const {
    const int C = c->abl_ch[level], P = pl.h[level] * pl.w[level];
    const dim3 grid((P + TAP_P - 1) / TAP_P, (C + TAP_C - 1) / TAP_C, n);
    if (split && level > 0)
      hipLaunchKernelGGL(tap_nchw_kernel<true>, grid, dim3(256), 0, s, x, P, C,
                         1.f / c->act_scale, tap[level]);
    else
      hipLaunchKernelGGL(tap_nchw_kernel<false>, grid, dim3(256), 0, s, x, P, C, 1.f,
                         tap[level]);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }

  // Runs the forward from level `from` (-1: from `src` = the images; otherwise `src` is the
  // level's tensor with its mask already applied) up to and including level `to`, applying the
  // context's masks to every level it produces.  *out = the level-`to` tensor.  Every level
  // it produces that has a tap[] pointer is also written there, after its mask.
  int walk(int from, int to, const float* src, const float** out) const {
    const float* x = src;
    if (from < 0) {
      const bool pair_stem = split && c->stem_pair.ws != nullptr;
      MILAN_TRY(launch_raw_input(src, n, hin, win, pair_stem, pl.in4, c->status, s));
      MILAN_TRY(launch_gemm(encoder_stem_args(c, pl.in4, n, hin, win, pl.raw, pair_stem), s));
      if (c->abl_count[0] > 0) MILAN_TRY(mask(0, pl.raw, pl.raw, -1));
      x = pl.raw;
      from = 0;
      if (tap[0]) MILAN_TRY(emit(0, x));
    }
    if (to == from) { *out = x; return 0; }
    float* y = pl.x0;
    if (from == 0) {
      MILAN_TRY(launch_stem_tail(c, x, n, pl.h[0], pl.w[0], pl.h[1], pl.w[1], split, pl.x0, s));
      x = pl.x0; y = pl.x1;
    }
    int h = pl.h[from == 0 ? 1 : from], w = pl.w[from == 0 ? 1 : from];
    for (int li = from == 0 ? 0 : from; li < 4 && li < to; ++li) {
      for (const Bottleneck& b : c->blocks[li]) {
        int h1, w1, h2, w2, h3, w3, hd, wdn;
        const float* identity = x;
        if (b.has_down) {
          MILAN_TRY(launch_gemm(encoder_conv_args(b.down, x, n, h, w, pl.ds, EPI_BIAS, nullptr,
                                                  c->zero, &hd, &wdn, split), s));
          identity = pl.ds;
        }
        MILAN_TRY(launch_gemm(encoder_conv_args(b.c1, x, n, h, w, pl.t1, EPI_BIAS_RELU, nullptr,
                                                c->zero, &h1, &w1, split), s));
        if (b.basic) {
          // BasicBlock: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity)
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c2, pl.t1, n, h1, w1, y, EPI_BIAS_RES_RELU,
                                                  identity, c->zero, &h3, &w3, split), s));
        } else {
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c2, pl.t1, n, h1, w1, pl.t2, EPI_BIAS_RELU,
                                                  nullptr, c->zero, &h2, &w2, split), s));
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c3, pl.t2, n, h2, w2, y, EPI_BIAS_RES_RELU,
                                                  identity, c->zero, &h3, &w3, split), s));
        }
        // the block's output becomes the next input; the other ping-pong buffer the next output
        // (an input that came from outside -- the sweep's working tensor -- is left alone)
        const float* nx = y;
        y = (x == pl.x0 || x == pl.x1) ? const_cast<float*>(x) : (y == pl.x0 ? pl.x1 : pl.x0);
        x = nx;
        h = h3; w = w3;
      }
      MILAN_REQUIRE(h == pl.h[li + 1] && w == pl.w[li + 1], MILAN_ERR_SHAPE,
                    "internal: stage %d geometry mismatch", li + 1);
      if (c->abl_count[li + 1] > 0)
        MILAN_TRY(mask(li + 1, x, const_cast<float*>(x), -1));
      if (tap[li + 1]) MILAN_TRY(emit(li + 1, x));
    }
    *out = x;
    return 0;
  }

  // avgpool + fc (+ argmax) of the masked level-4 tensor
  int head(const float* x4, float* logits, long long* preds) const {
    const int C = c->abl_ch[4], P = pl.h[4] * pl.w[4], K = c->fc_classes;
    if (split)
      hipLaunchKernelGGL(avgpool_kernel<true>, dim3((C + 255) / 256, n), dim3(256), 0, s, x4, P, C,
                         1.f / c->act_scale, pl.pooled);
    else
      hipLaunchKernelGGL(avgpool_kernel<false>, dim3((C + 255) / 256, n), dim3(256), 0, s, x4, P,
                         C, 1.f, pl.pooled);
    hipLaunchKernelGGL(fc_kernel, dim3((K + 3) / 4, n), dim3(256), 0, s, pl.pooled, c->fc_w,
                       c->fc_b, C, K, logits);
    if (preds)
      hipLaunchKernelGGL(row_argmax_kernel, dim3(n), dim3(64), 0, s, logits, K, preds);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }

  int hin = 0, win = 0;
  float* tap[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// `head`: the call runs avgpool + fc (milan_activations stops before them and does not)
static int classify_checks(milan_ctx* c, int n, int H, int W, bool* split, bool head = true) {
  MILAN_REQUIRE(resnet_trunk(c), MILAN_ERR_ARG,
                "classification needs a ResNet trunk (AlexNet's classifier is not built)");
  MILAN_REQUIRE(c->stem.w != nullptr && c->abl_mask != nullptr, MILAN_ERR_STATE,
                "encoder weights were not uploaded");
  MILAN_REQUIRE(!head || c->fc_w != nullptr, MILAN_ERR_STATE,
                "this context was created without fc.weight: it has no classifier head");
  MILAN_REQUIRE(!c->trunk_f16, MILAN_ERR_ARG,
                "classification runs in the f32 and split_f16 modes, not in the fast f16 mode");
  MILAN_REQUIRE(n > 0 && H >= 1 && W >= 1, MILAN_ERR_SHAPE,
                "classify: need n>0 and H,W>=1 (got n=%d H=%d W=%d)", n, H, W);
  bool sp = c->precision == MILAN_PRECISION_SPLIT_F16 && c->d.trunk_width % 8 == 0;
  for (int li = 0; li < 4 && sp; ++li)
    for (const Bottleneck& b : c->blocks[li])
      sp = sp && b.c1.ws && b.c2.ws && (b.basic || b.c3.ws) && (!b.has_down || b.down.ws);
  *split = sp;
  return 0;
}

int classify_run(milan_ctx* c, const float* images, int n, int H, int W, float* logits,
                 int64_t* predictions, Arena& ws, hipStream_t s) {
  bool split;
  MILAN_TRY(classify_checks(c, n, H, W, &split));
  const int sub = encoder_sub_batch_size();
  for (int lo = 0; lo < n; lo += sub) {
    const int cnt = n - lo < sub ? n - lo : sub;
    Arena a = ws;  // every pass reuses the same scratch
    ClsPlan pl;
    cls_plan(c, cnt, H, W, 0, 0, a, &pl);
    MILAN_REQUIRE(a.off <= a.size, MILAN_ERR_WORKSPACE,
                  "classify: workspace too small (%zu needed, %zu given)", a.off, a.size);
    Walker wk{c, pl, cnt, split, s};
    wk.hin = H; wk.win = W;
    const float* x4;
    MILAN_TRY(wk.walk(-1, 4, images + (size_t)lo * 3 * H * W, &x4));
    float* lg = logits ? logits + (size_t)lo * c->fc_classes : pl.logits;
    MILAN_TRY(wk.head(x4, lg, predictions ? (long long*)predictions + lo : nullptr));
  }
  return 0;
}

int classify_sweep(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                   const int32_t* units, int count, const int64_t* targets, int32_t* correct,
                   int64_t* predictions, Arena& ws, hipStream_t s) {
  bool split;
  MILAN_TRY(classify_checks(c, n, H, W, &split));
  MILAN_TRY(check_units(c, levels, units, count, "milan_classify_sweep"));
  if (count == 0) return 0;
  const int sub = encoder_sub_batch_size();
  long long* preds_all = (long long*)predictions;
  for (int lo = 0; lo < n; lo += sub) {
    const int cnt = n - lo < sub ? n - lo : sub;
    Arena a = ws;
    ClsPlan pl;
    cls_plan(c, cnt, H, W, count, n, a, &pl);
    MILAN_REQUIRE(a.off <= a.size, MILAN_ERR_WORKSPACE,
                  "classify_sweep: workspace too small (%zu needed, %zu given)", a.off, a.size);
    if (preds_all == nullptr) preds_all = pl.preds;   // (the same address in every pass)
    Walker wk{c, pl, cnt, split, s};
    wk.hin = H; wk.win = W;
    // units grouped by level: the forward up to and including the level runs once per pass with
    // the base set's masks and is held; every unit is one masked copy plus the suffix
    for (int level = 0; level < 5; ++level) {
      bool any = false;
      for (int j = 0; j < count && !any; ++j) any = levels[j] == level;
      if (!any) continue;
      const float* held;
      MILAN_TRY(wk.walk(-1, level, images + (size_t)lo * 3 * H * W, &held));
      if (level > 0) {
        // (levels >= 1 live in the ping-pong buffers the suffix overwrites; the raw conv1
        // tensor has a buffer of its own)
        MILAN_CHECK_HIP(hipMemcpyAsync(pl.hold, held, sizeof(float) * cnt * pl.lvl_sz[level],
                                       hipMemcpyDeviceToDevice, s));
        held = pl.hold;
      }
      for (int j = 0; j < count; ++j) {
        if (levels[j] != level) continue;
        MILAN_TRY(wk.mask(level, held, pl.work, units[j]));
        const float* x4;
        MILAN_TRY(wk.walk(level, 4, pl.work, &x4));
        MILAN_TRY(wk.head(x4, pl.logits, preds_all + (size_t)j * n + lo));
      }
    }
  }
  if (correct != nullptr) {
    hipLaunchKernelGGL(correct_count_kernel, dim3(count), dim3(256), 0, s, preds_all,
                       (const long long*)targets, n, correct);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// milan_activations: the walk of classify_run, once per sub-batch up to the highest requested
// level, each requested level converted to fp32 NCHW when it is produced; no head
size_t activations_workspace(const milan_ctx* c, int n_images, int H, int W) {
  return classify_workspace(c, n_images, H, W, 0);
}

int activations_run(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                    int count, float* const* outputs, Arena& ws, hipStream_t s) {
  bool split;
  MILAN_TRY(classify_checks(c, n, H, W, &split, false));
  int slot[5] = {-1, -1, -1, -1, -1}, top = -1;
  for (int i = 0; i < count; ++i) {
    MILAN_REQUIRE(levels[i] >= 0 && levels[i] <= 4, MILAN_ERR_ARG,
                  "milan_activations: level %d is not one of 0..4 (conv1, layer1..layer4)",
                  levels[i]);
    MILAN_REQUIRE(slot[levels[i]] < 0, MILAN_ERR_ARG,
                  "milan_activations: level %d is requested twice", levels[i]);
    MILAN_REQUIRE(outputs[i] != nullptr, MILAN_ERR_ARG,
                  "milan_activations: outputs[%d] is null", i);
    slot[levels[i]] = i;
    top = std::max(top, (int)levels[i]);
  }
  const int sub = encoder_sub_batch_size();
  for (int lo = 0; lo < n; lo += sub) {
    const int cnt = n - lo < sub ? n - lo : sub;
    Arena a = ws;  // every pass reuses the same scratch
    ClsPlan pl;
    cls_plan(c, cnt, H, W, 0, 0, a, &pl);
    MILAN_REQUIRE(a.off <= a.size, MILAN_ERR_WORKSPACE,
                  "activations: workspace too small (%zu needed, %zu given)", a.off, a.size);
    MILAN_REQUIRE(cnt <= 65535, MILAN_ERR_ARG, "activations: sub-batch of %d images", cnt);
    Walker wk{c, pl, cnt, split, s};
    wk.hin = H; wk.win = W;
    for (int l = 0; l < 5; ++l)
      if (slot[l] >= 0) wk.tap[l] = outputs[slot[l]] + (size_t)lo * pl.lvl_sz[l];
    const float* x;
    MILAN_TRY(wk.walk(-1, top, images + (size_t)lo * 3 * H * W, &x));
  }
  return 0;
}

}  // namespace milan
