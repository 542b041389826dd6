// Unit ablation, classification and activation taps on the ResNet trunks (milan_set_ablation,
// milan_classify, milan_classify_sweep, milan_activations): the reference's
// src/utils/ablations.py on torchvision's ResNet._forward_impl, eval mode.  The same calls on
// AlexNet (alexnet_seq: conv1..conv5, fc6, fc7, linear8) run through the same driver with a
// walk, a tail kernel and a Linear kernel of their own.
//
// The ResNet forward is a plain walker of its own: stem conv, bn1 + ReLU + maxpool, every
// block's convs through launch_gemm with the epilogues the encoder uses, then the head.  It
// materialises the five tensors an edit must see -- the raw conv1 output (level 0: nethook
// edits the module's output, before bn1) and the post-ReLU output of every stage (levels 1..4)
// -- and multiplies each by the context's 0/1 channel mask before anything reads it.  None of
// the encoder's fused launches (chain, fused stem, conv-front, row lists) is used: those are
// the paths that never write such a tensor.
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

// workgroups of 256 threads for a grid-stride loop over `items`
static int grid_for(long items) {
  const long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b < 16384 ? b : 16384));
}

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
// AlexNet: the tail of the trunk and the Linear layers
// ---------------------------------------------------------------------------
// pool5 + AdaptiveAvgPool2d((6, 6)) + flatten of the masked level-4 tensor (n, H, W, C), fp32 or
// split (avgpool_kernel<true>'s decode) -> fp32 (n, C * 36), column c * 36 + i * 6 + j.
// pool5 is the 3x3 / stride 2 max-pool without padding, (Hp, Wp) its extent; bin (i, j) covers
// pooled rows floor(i Hp / 6) .. ceil((i + 1) Hp / 6) - 1 and the columns likewise (torch's
// rule), added in ascending (row, column) order, then one division by the bin's size.
// A thread per (image, bin, channel), channels fastest.  grid (ceil(36 C / 256), n).
template <bool SPLIT>
__global__ __launch_bounds__(256) void alex_tail_kernel(const float* __restrict__ x, int H, int W,
                                                        int C, int Hp, int Wp, float inv_scale,
                                                        float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 36 * C) return;
  const int c = idx % C, bin = idx / C, bi = bin / 6, bj = bin % 6;
  const size_t img = blockIdx.y;
  const float* src = x + img * (size_t)H * W * C;
  const int r0 = (bi * Hp) / 6, r1 = ((bi + 1) * Hp + 5) / 6;
  const int q0 = (bj * Wp) / 6, q1 = ((bj + 1) * Wp + 5) / 6;
  float sum = 0.f;
  for (int r = r0; r < r1; ++r)
    for (int q = q0; q < q1; ++q) {
      float best = -INFINITY;
      for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
          const float* px = src + ((size_t)(2 * r + dy) * W + (2 * q + dx)) * C;
          float v;
          if constexpr (SPLIT) {
            const _Float16* g = reinterpret_cast<const _Float16*>(px + (c >> 3) * 8);
            v = ((float)g[c & 7] + (float)g[8 + (c & 7)]) * inv_scale;
          } else {
            v = px[c];
          }
          best = fmaxf(best, v);
        }
      sum += best;
    }
  out[img * (size_t)C * 36 + (size_t)c * 36 + bin] = sum / (float)((r1 - r0) * (q1 - q0));
}

// ---------------------------------------------------------------------------
// VGG: the first conv, the 2x2 pool and the tail of the trunk
// ---------------------------------------------------------------------------
// conv1_1's weight (cout, 3, 3, 3) OIHW -> (27, cout), row k = (kh * 3 + kw) * 3 + c
__global__ void vgg_pack_first_kernel(const float* __restrict__ w, int cout,
                                      float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 27 * cout) return;
  const int o = idx % cout, k = idx / cout;
  const int c = k % 3, t = k / 3;   // t = kh * 3 + kw
  out[idx] = w[(o * 3 + c) * 9 + t];
}

int vgg_pack_first(const float* w_oihw, int cout, float* w27, hipStream_t s) {
  hipLaunchKernelGGL(vgg_pack_first_kernel, dim3((27 * cout + 255) / 256), dim3(256), 0, s,
                     w_oihw, cout, w27);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// conv1_1 (3 -> C channels, 3x3, pad 1, stride 1) + bias + ReLU straight from the fp32 NCHW
// image (n, 3, H, W) to NHWC (n, H, W, C): fp32, or OUT_SPLIT split groups [hi x8 | lo x8] at
// scale 1.  A workgroup owns one output row of one image (grid = n H); a thread owns the
// 8-channel piece g of two horizontally adjacent pixels, pieces fastest: consecutive lanes write
// consecutive 32 bytes (two 16-byte stores per pixel) and read the same or neighbouring image
// words, the 3 x 4 x 3 input words of a pair once each.  The 27 x C weights and the bias sit
// in LDS (28 C floats); a lane reads its 8 weights of a tap as two 16-byte pieces, lanes of one
// piece the same address, and uses them for both pixels.  Per output: acc from zero, acc =
// fma(x, w, acc) over the taps in (kh, kw, c) ascending order -- a tap in the padding enters
// with x = 0, which leaves acc as it is; two channels share one packed fma, every lane of it a
// correctly rounded fma of its own -- then acc + bias, then max(., 0).  Neither the grid nor
// the batch enters, nor which pixel of its pair an output is.
// (The loop over kernel rows stays rolled: unrolled, the compiler issues all 54 weight reads of
// a piece up front, 272 VGPRs and one wave per SIMD, and the loads' latency shows; rolled it is
// 58 VGPRs.)
typedef float cf32x2_t __attribute__((ext_vector_type(2)));
template <bool OUT_SPLIT>
__global__ __launch_bounds__(256) void vgg_first_kernel(const float* __restrict__ img, int H,
                                                        int W, int C,
                                                        const float* __restrict__ w27,
                                                        const float* __restrict__ bias,
                                                        float* __restrict__ y,
                                                        unsigned* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float vgg_w[];   // [27][C] | bias [C]
  for (int i = threadIdx.x; i < 27 * C; i += blockDim.x) vgg_w[i] = w27[i];
  for (int i = threadIdx.x; i < C; i += blockDim.x) vgg_w[27 * C + i] = bias[i];
  __syncthreads();
  const int C8 = C >> 3, items = ((W + 1) >> 1) * C8;
  const size_t plane = (size_t)H * W;
  const size_t row = blockIdx.x;   // image * H + y0
  const int y0 = (int)(row % H);
  const float* src = img + (row / H) * 3 * plane;
  float* out_row = y + row * (size_t)W * C;
  float sat = 0.f;
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int g = i % C8, x0 = 2 * (i / C8);
    cf32x2_t acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[p][e] = cf32x2_t{0.f, 0.f};
#pragma unroll 1
    for (int kh = 0; kh < 3; ++kh) {
      const int iy = y0 + kh - 1;
      const bool row_in = iy >= 0 && iy < H;
      const float* line = src + (size_t)(row_in ? iy : y0) * W;
      // columns x0 - 1 .. x0 + 2 of the three channels: clamped addresses, zeros outside
      float v[3][4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int ix = x0 - 1 + d;
        const bool in = row_in && ix >= 0 && ix < W;
        const int ixc = ix < 0 ? 0 : (ix < W ? ix : W - 1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float t = line[ch * plane + ixc];
          v[ch][d] = in ? t : 0.f;
        }
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float* wk = vgg_w + ((kh * 3 + kw) * 3 + ch) * C + g * 8;
          const cf32x4_t w0 = *reinterpret_cast<const cf32x4_t*>(wk);
          const cf32x4_t w1 = *reinterpret_cast<const cf32x4_t*>(wk + 4);
          const cf32x2_t wp[4] = {{w0[0], w0[1]}, {w0[2], w0[3]}, {w1[0], w1[1]}, {w1[2], w1[3]}};
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const cf32x2_t xx = {v[ch][kw + p], v[ch][kw + p]};
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[p][e] = __builtin_elementwise_fma(xx, wp[e], acc[p][e]);
          }
        }
    }
    const float* bk = vgg_w + 27 * C + g * 8;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (x0 + p >= W) break;   // (the second pixel of the last pair of an odd row)
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = __fadd_rn(acc[p][e >> 1][e & 1], bk[e]);
      float* dst = out_row + (size_t)(x0 + p) * C + g * 8;
      if constexpr (OUT_SPLIT) {
        cf32x4_t hi4, lo4;
        split8_relu_rne(r, &hi4, &lo4, &sat);
        *reinterpret_cast<cf32x4_t*>(dst) = hi4;
        *reinterpret_cast<cf32x4_t*>(dst + 4) = lo4;
      } else {
        cf32x4_t o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o0[e] = r[e] > 0.f ? r[e] : 0.f;
          o1[e] = r[4 + e] > 0.f ? r[4 + e] : 0.f;
        }
        *reinterpret_cast<cf32x4_t*>(dst) = o0;
        *reinterpret_cast<cf32x4_t*>(dst + 4) = o1;
      }
    }
  }
  if constexpr (OUT_SPLIT) report_saturation(status, sat);
}

// 2x2 / stride 2 max-pool without padding over NHWC, (n, H, W, C) -> (n, Ho, Wo, C) with
// Ho = floor(H / 2), Wo = floor(W / 2): an odd last row or column is dropped, every window is
// whole.  A thread owns one output pixel's piece of 8 channels: two 16-byte loads per input
// pixel, two 16-byte stores.  fp32 -> fp32, fp32 -> split and split -> split at scale 1 (a
// split value is float(hi) + float(lo)); the maximum starts at -inf and fmaxf drops a NaN, as
// in the 3x3 / 2 pool of the AlexNets; saturation of the conversion goes to `status`.
template <bool IN_SPLIT, bool OUT_SPLIT>
__global__ __launch_bounds__(256) void maxpool2s2_kernel(const float* __restrict__ x, int H,
                                                         int W, int C8, int Ho, int Wo,
                                                         long total, float* __restrict__ y,
                                                         unsigned* __restrict__ status) {
  float sat = 0.f;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c8 = (int)(idx % C8);
    long t = idx / C8;
    const int wo = (int)(t % Wo); t /= Wo;
    const int ho = (int)(t % Ho);
    const size_t img = (size_t)(t / Ho);
    float best[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float* p =
            x + (((img * H + (size_t)(2 * ho + dy)) * W + (size_t)(2 * wo + dx)) * C8 + c8) * 8;
        const cf32x4_t a = *reinterpret_cast<const cf32x4_t*>(p);
        const cf32x4_t b = *reinterpret_cast<const cf32x4_t*>(p + 4);
        float v[8];
        if constexpr (IN_SPLIT) {
          join8_exact(a, b, v);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], v[e]);
      }
    float* d = y + idx * 8;
    if constexpr (OUT_SPLIT) {
      cf32x4_t hi4, lo4;
      split8_rne(best, &hi4, &lo4, &sat);
      *reinterpret_cast<cf32x4_t*>(d) = hi4;
      *reinterpret_cast<cf32x4_t*>(d + 4) = lo4;
    } else {
      const cf32x4_t o0 = {best[0], best[1], best[2], best[3]};
      const cf32x4_t o1 = {best[4], best[5], best[6], best[7]};
      *reinterpret_cast<cf32x4_t*>(d) = o0;
      *reinterpret_cast<cf32x4_t*>(d + 4) = o1;
    }
  }
  if constexpr (OUT_SPLIT) report_saturation(status, sat);
}

// pool5 (2x2 / 2) + AdaptiveAvgPool2d((7, 7)) + flatten of the masked level-4 tensor
// (n, H, W, C), fp32 or split at scale 1 -> fp32 (n, C * 49), column c * 49 + i * 7 + j.
// (Hp, Wp) = (floor(H / 2), floor(W / 2)) is pool5's extent; bin (i, j) covers pooled rows
// floor(i Hp / 7) .. ceil((i + 1) Hp / 7) - 1 and the columns likewise (torch's rule: a 1 x 1
// extent is replicated, a 7 x 7 one handed through), added from zero in ascending (row,
// column) order, then one division by the bin's size.  A thread per (image, bin, channel),
// channels fastest.  grid (ceil(49 C / 256), n).
template <bool SPLIT>
__global__ __launch_bounds__(256) void vgg_tail_kernel(const float* __restrict__ x, int H, int W,
                                                       int C, int Hp, int Wp,
                                                       float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 49 * C) return;
  const int c = idx % C, bin = idx / C, bi = bin / 7, bj = bin % 7;
  const size_t img = blockIdx.y;
  const float* src = x + img * (size_t)H * W * C;
  const int r0 = (bi * Hp) / 7, r1 = ((bi + 1) * Hp + 6) / 7;
  const int q0 = (bj * Wp) / 7, q1 = ((bj + 1) * Wp + 6) / 7;
  float sum = 0.f;
  for (int r = r0; r < r1; ++r)
    for (int q = q0; q < q1; ++q) {
      float best = -INFINITY;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const float* px = src + ((size_t)(2 * r + dy) * W + (2 * q + dx)) * C;
          float v;
          if constexpr (SPLIT) {
            const _Float16* g = reinterpret_cast<const _Float16*>(px + (c >> 3) * 8);
            v = (float)g[c & 7] + (float)g[8 + (c & 7)];
          } else {
            v = px[c];
          }
          best = fmaxf(best, v);
        }
      sum = __fadd_rn(sum, best);
    }
  out[img * (size_t)C * 49 + (size_t)c * 49 + bin] =
      __fdiv_rn(sum, (float)((r1 - r0) * (q1 - q0)));
}

static int launch_vgg_first(const float* images, int n, int H, int W, int C, const float* w27,
                     const float* bias, bool out_split, float* y, unsigned* status,
                     hipStream_t s) {
  MILAN_REQUIRE(images && w27 && bias && y && n >= 1 && H >= 1 && W >= 1 && C >= 8 &&
                    C % 8 == 0 && C <= 512,
                MILAN_ERR_ARG, "vgg first conv: bad argument (C = %d)", C);
  // (a workgroup per output row: the grid's x extent takes 2^31 - 1 of them)
  MILAN_REQUIRE((long)n * H <= 0x7fffffffL, MILAN_ERR_ARG, "vgg first conv: %d x %d rows", n, H);
  const dim3 grid((unsigned)((long)n * H));
  const size_t lds = sizeof(float) * 28 * (size_t)C;
  if (out_split)
    hipLaunchKernelGGL(vgg_first_kernel<true>, grid, dim3(256), lds, s, images, H, W, C, w27,
                       bias, y, status);
  else
    hipLaunchKernelGGL(vgg_first_kernel<false>, grid, dim3(256), lds, s, images, H, W, C, w27,
                       bias, y, status);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int launch_maxpool2s2(const float* x, int n, int H, int W, int C, bool in_split, bool out_split,
                      float* y, unsigned* status, hipStream_t s) {
  const int Ho = H / 2, Wo = W / 2;
  MILAN_REQUIRE(x && y && n >= 1 && Ho >= 1 && Wo >= 1 && C >= 8 && C % 8 == 0, MILAN_ERR_ARG,
                "maxpool 2x2: bad argument (%d x %d x %d)", H, W, C);
  MILAN_REQUIRE(out_split || !in_split, MILAN_ERR_STATE,
                "internal: there is no split -> fp32 2x2 pool");
  const long total = (long)n * Ho * Wo * (C / 8);
  const dim3 grid(grid_for(total));
  if (!out_split)
    hipLaunchKernelGGL((maxpool2s2_kernel<false, false>), grid, dim3(256), 0, s, x, H, W, C / 8,
                       Ho, Wo, total, y, status);
  else if (in_split)
    hipLaunchKernelGGL((maxpool2s2_kernel<true, true>), grid, dim3(256), 0, s, x, H, W, C / 8, Ho,
                       Wo, total, y, status);
  else
    hipLaunchKernelGGL((maxpool2s2_kernel<false, true>), grid, dim3(256), 0, s, x, H, W, C / 8,
                       Ho, Wo, total, y, status);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Across-channel local response normalisation of the Places365 AlexNet, over an
// NHWC tensor of `chunks` = pixels x C / 8 eight-channel pieces:
//   y[c] = x[c] / (1 + alpha * S[c] / n)^beta,  S[c] = sum of x[j]^2, |j - c| <= half, 0 <= j < C
// with n = 2 half + 1 whatever part of the window lies outside (torch's AvgPool3d with
// count_include_pad).  A thread owns one piece and reads its two neighbours (half <= 8): two
// 16-byte loads per piece, fp32 or split (hi x8 | lo x8) at scale 1, the channels of a pixel
// contiguous.  Per value: squares by one multiplication, S from zero in ascending j by plain
// additions, avg = S / n, d = fma(avg, alpha, 1), p = sqrt(d) * sqrt(sqrt(d)) for beta = 0.75
// (correctly rounded steps) or powf(d, beta), y = x / p.  HALF > 0 fixes the window at compile
// time; 0 reads `half` (<= 8).  x and y must not overlap.
template <bool SPLIT, int HALF>
__global__ __launch_bounds__(256) void lrn_kernel(const float* __restrict__ x, long chunks, int C8,
                                                  int half, float alpha, float beta,
                                                  float* __restrict__ y,
                                                  unsigned* __restrict__ status) {
  const float n = (float)(2 * (HALF > 0 ? HALF : half) + 1);
  const bool b34 = beta == 0.75f;
  float sat = 0.f;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < chunks;
       q += (long)gridDim.x * blockDim.x) {
    const int k = (int)(q % C8);
    float v[24];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int kk = k - 1 + t;
      if (kk >= 0 && kk < C8) {
        const float* px = x + (q + (t - 1)) * 8;
        const cf32x4_t a = *reinterpret_cast<const cf32x4_t*>(px);
        const cf32x4_t b = *reinterpret_cast<const cf32x4_t*>(px + 4);
        if constexpr (SPLIT) {
          join8_exact(a, b, v + t * 8);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[t * 8 + e] = a[e]; v[t * 8 + 4 + e] = b[e]; }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[t * 8 + e] = 0.f;
      }
    }
    float sq[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) sq[i] = __fmul_rn(v[i], v[i]);
    float out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float S = 0.f;
      if constexpr (HALF > 0) {
#pragma unroll
        for (int j = -HALF; j <= HALF; ++j) S = __fadd_rn(S, sq[8 + e + j]);
      } else {
#pragma unroll
        for (int j = -8; j <= 8; ++j)
          S = __fadd_rn(S, (j >= -half && j <= half) ? sq[8 + e + j] : 0.f);
      }
      const float d = __fmaf_rn(__fdiv_rn(S, n), alpha, 1.f);
      const float p = b34 ? __fmul_rn(__fsqrt_rn(d), __fsqrt_rn(__fsqrt_rn(d))) : powf(d, beta);
      out[e] = __fdiv_rn(v[8 + e], p);
    }
    float* dst = y + q * 8;
    if constexpr (SPLIT) {
      cf32x4_t hi4, lo4;
      split8_rne(out, &hi4, &lo4, &sat);
      *reinterpret_cast<cf32x4_t*>(dst) = hi4;
      *reinterpret_cast<cf32x4_t*>(dst + 4) = lo4;
    } else {
      const cf32x4_t o0 = {out[0], out[1], out[2], out[3]}, o1 = {out[4], out[5], out[6], out[7]};
      *reinterpret_cast<cf32x4_t*>(dst) = o0;
      *reinterpret_cast<cf32x4_t*>(dst + 4) = o1;
    }
  }
  if constexpr (SPLIT) report_saturation(status, sat);
}

int launch_lrn(const float* x, long long pixels, int C, bool split, int local_size, float alpha,
               float beta, float* y, unsigned* status, hipStream_t s) {
  MILAN_REQUIRE(x && y && pixels >= 1 && C >= 8 && C % 8 == 0, MILAN_ERR_ARG,
                "lrn: need a tensor of >= 1 pixels and a multiple of 8 channels (got %lld x %d)",
                pixels, C);
  MILAN_REQUIRE(local_size >= 1 && local_size % 2 == 1 && local_size <= 17, MILAN_ERR_ARG,
                "lrn: local_size %d is not an odd number in 1..17", local_size);
  const size_t bytes = (size_t)pixels * C * sizeof(float);
  MILAN_REQUIRE((const char*)x + bytes <= (const char*)y || (const char*)y + bytes <= (const char*)x,
                MILAN_ERR_ARG, "lrn: input and output overlap");
  MILAN_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, MILAN_ERR_ARG,
                "lrn: tensors must be 16-byte aligned");
  const long chunks = (long)pixels * (C / 8);
  const long b = (chunks + 255) / 256;
  const dim3 grid((int)(b < 16384 ? b : 16384));
  const int half = local_size / 2;
#define MILAN_LRN(SPLIT, HALF)                                                                 \
  hipLaunchKernelGGL((lrn_kernel<SPLIT, HALF>), grid, dim3(256), 0, s, x, chunks, C / 8, half, \
                     alpha, beta, y, status)
  if (split) {
    if (half == 2) MILAN_LRN(true, 2); else if (half == 1) MILAN_LRN(true, 1); else MILAN_LRN(true, 0);
  } else {
    if (half == 2) MILAN_LRN(false, 2); else if (half == 1) MILAN_LRN(false, 1); else MILAN_LRN(false, 0);
  }
#undef MILAN_LRN
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Linear layer y (M, N) = act(x (M, K) W^T + bias) on v_mfma_f32_32x32x2_f32: exact fp32, and
// per output a k-ordered fmaf chain.  The summation order of an output depends on K alone:
//   - K is padded with zeros to Kp (a multiple of 8) and cut into chunks of 256;
//   - a chunk is one chain from zero: acc = fmaf(x[k], w[k], acc), k ascending;
//   - wavefront v of the workgroup's four owns chunks v, v + 4, v + 8, ... and adds their sums
//     in that order to its total (from zero);
//   - the output is ((total0 + total1) + (total2 + total3)) + bias.
// Neither M, the grid nor a row's place in its tile enters: rows of the A operand are
// independent in the MFMA, so a batch gives the bits of its parts.
//
// A workgroup computes one tile of 32 rows of x by 32 rows of W, so W is streamed once per 32
// images.  W is packed once (linear_pack_kernel) into the order the B fragments are read: tile
// t = n / 32, then groups of 8 k, then lane l, then 4 floats = the lane's B operand of 4
// consecutive MFMAs, k = 8 g + 2 e + (l >> 5), n = 32 t + (l & 31); one 16-byte load per lane
// and 4 MFMAs, 1 KiB contiguous per wavefront.  x goes through LDS, 64 k at a time per
// wavefront: read along k (256-byte runs), stored k-major with rows padded to 33 dwords, so that
// the stores (bank 4 (l & 15) + (l >> 4) + const) and the per-MFMA reads (lane = row, two k)
// are free of bank conflicts but for one pair.
constexpr int LIN_SUB = 64, LIN_CHUNK = 256, LIN_LD = 33, LIN_WAVES = 4;
typedef float cf32x16_t __attribute__((ext_vector_type(16)));

__global__ void linear_pack_kernel(const float* __restrict__ W, int N, int K, int Kp, long total,
                                   float* __restrict__ out) {
  const int groups = Kp / 8;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 3), l = (int)((idx >> 2) & 63);
    const long tg = idx >> 8;
    const int g = (int)(tg % groups), t = (int)(tg / groups);
    const int n = t * 32 + (l & 31), k = g * 8 + 2 * e + (l >> 5);
    out[idx] = (n < N && k < K) ? W[(long)n * K + k] : 0.f;
  }
}

// VEC: K % 4 == 0, x rows are read as float4.  grid (ceil(N / 32), ceil(M / 32)).
template <bool VEC>
__global__ __launch_bounds__(256) void linear_mfma_kernel(const float* __restrict__ x,
                                                          const float* __restrict__ Wp,
                                                          const float* __restrict__ bias, int M,
                                                          int K, int Kp, int N, int relu,
                                                          float* __restrict__ y) {
  __shared__ float lds[LIN_WAVES * LIN_SUB * LIN_LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  float* xs = lds + wv * (LIN_SUB * LIN_LD);
  const int groups = Kp / 8;
  const cf32x4_t* wt =
      reinterpret_cast<const cf32x4_t*>(Wp) + (size_t)blockIdx.x * groups * 64 + lane;
  const int chunks = (Kp + LIN_CHUNK - 1) / LIN_CHUNK;
  const int rounds = (chunks + LIN_WAVES - 1) / LIN_WAVES;
  const int kq = lane & 15, rq = lane >> 4;   // staging: 16 lanes along k, 4 rows per pass
  cf32x16_t total;
#pragma unroll
  for (int i = 0; i < 16; ++i) total[i] = 0.f;
  // One step = 64 k of this wavefront's chunk: step t is sub-step t & 3 of the chunk of round
  // t >> 2.  The loads of step t + 1 (B operands and the x tile, in registers) are issued
  // before the MFMAs of step t and waited for after them.  A step at or past Kp loads nothing
  // and computes nothing (the same decision in all 64 lanes; every wavefront meets the barriers).
  constexpr int SUBS = LIN_CHUNK / LIN_SUB;
  const int steps = rounds * SUBS;
  cf32x4_t wn[LIN_SUB / 8], xn[8];
  auto fetch = [&](int t) {
    const int k0 = ((t / SUBS) * LIN_WAVES + wv) * LIN_CHUNK + (t % SUBS) * LIN_SUB;
    if (k0 >= Kp) return;
#pragma unroll
    for (int g = 0; g < LIN_SUB / 8; ++g) {
      const int gi = k0 / 8 + g;
      cf32x4_t w = {0.f, 0.f, 0.f, 0.f};
      if (gi < groups) w = wt[(size_t)gi * 64];
      wn[g] = w;
    }
    const int k = k0 + 4 * kq;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + rq + 4 * i;
      cf32x4_t v = {0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        const float* px = x + (size_t)m * K + k;
        if constexpr (VEC) {
          if (k < K) v = *reinterpret_cast<const cf32x4_t*>(px);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < K) v[e] = px[e];
        }
      }
      xn[i] = v;
    }
  };
  cf32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  fetch(0);
  for (int t = 0; t < steps; ++t) {
    const bool live = ((t / SUBS) * LIN_WAVES + wv) * LIN_CHUNK + (t % SUBS) * LIN_SUB < Kp;
    cf32x4_t wr[LIN_SUB / 8];
    if (live) {
#pragma unroll
      for (int g = 0; g < LIN_SUB / 8; ++g) wr[g] = wn[g];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) xs[(4 * kq + e) * LIN_LD + rq + 4 * i] = xn[i][e];
    }
    __syncthreads();
    if (t + 1 < steps) fetch(t + 1);
    if (live) {
#pragma unroll
      for (int p = 0; p < LIN_SUB / 2; ++p) {
        const float a = xs[(2 * p + (lane >> 5)) * LIN_LD + (lane & 31)];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wr[p >> 2][p & 3], acc, 0, 0, 0);
      }
    }
    __syncthreads();
    if (t % SUBS == SUBS - 1) {   // the chunk is complete: into the total, and from zero again
      total += acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    }
  }
  // the four totals through LDS ([wavefront][register][lane]); wavefront v finishes registers
  // 4 v .. 4 v + 3.  D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* red = lds;
#pragma unroll
  for (int i = 0; i < 16; ++i) red[(wv * 16 + i) * 64 + lane] = total[i];
  __syncthreads();
  const int n = n0 + (lane & 31);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = wv * 4 + q;
    const float s = (red[i * 64 + lane] + red[(16 + i) * 64 + lane]) +
                    (red[(32 + i) * 64 + lane] + red[(48 + i) * 64 + lane]);
    const int m = m0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (m < M && n < N) {
      float v = s + (bias ? bias[n] : 0.f);
      if (relu) v = v < 0.f ? 0.f : v;
      y[(size_t)m * N + n] = v;
    }
  }
}

size_t linear_packed_floats(int N, int K) {
  const size_t kp = ((size_t)K + 7) / 8 * 8;
  return ((size_t)N + 31) / 32 * 32 * kp;
}

int linear_pack(const float* W, int N, int K, float* packed, hipStream_t s) {
  MILAN_REQUIRE(W && packed && N >= 1 && K >= 1, MILAN_ERR_ARG, "linear_pack: bad argument");
  const long total = (long)linear_packed_floats(N, K);
  const long b = (total + 255) / 256;
  hipLaunchKernelGGL(linear_pack_kernel, dim3((int)(b < 8192 ? b : 8192)), dim3(256), 0, s, W, N,
                     K, (K + 7) / 8 * 8, total, packed);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

int linear_run(const float* x, const float* packed, const float* bias, int M, int K, int N,
               bool relu, float* y, hipStream_t s) {
  MILAN_REQUIRE(x && packed && y && M >= 1 && K >= 1 && N >= 1, MILAN_ERR_ARG,
                "linear: bad argument");
  const int mt = (M + 31) / 32;
  MILAN_REQUIRE(mt <= 65535, MILAN_ERR_ARG, "linear: %d rows in one call", M);
  const dim3 grid((N + 31) / 32, mt);
  const int Kp = (K + 7) / 8 * 8;
  if (K % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(linear_mfma_kernel<true>, grid, dim3(256), 0, s, x, packed, bias, M, K, Kp,
                       N, relu ? 1 : 0, y);
  else
    hipLaunchKernelGGL(linear_mfma_kernel<false>, grid, dim3(256), 0, s, x, packed, bias, M, K,
                       Kp, N, relu ? 1 : 0, y);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// weights and the ablation set
// ---------------------------------------------------------------------------
static bool resnet_trunk(const milan_ctx* c) {
  return c->d.trunk_kind == MILAN_TRUNK_BOTTLENECK || c->d.trunk_kind == MILAN_TRUNK_BASIC;
}
// an AlexNet context classifies once milan_set_alexnet_head has installed its three Linear
// layers; until then it is refused as before
static bool alex_trunk(const milan_ctx* c) {
  return c->d.trunk_kind == MILAN_TRUNK_ALEXNET && c->ahead.installed;
}
// the Places365 AlexNet taps and ablates without a head; classifying needs one
static bool places_trunk(const milan_ctx* c) {
  return c->d.trunk_kind == MILAN_TRUNK_ALEXNET_PLACES;
}
// VGG: like the Places net it taps and ablates without a head
static bool vgg_trunk(const milan_ctx* c) { return c->d.trunk_kind == MILAN_TRUNK_VGG; }
// the sequential nets: SeqTrunk walks them, seq_family has their row
static bool seq_trunk(const milan_ctx* c) {
  return alex_trunk(c) || places_trunk(c) || vgg_trunk(c);
}
static bool classifier_trunk(const milan_ctx* c) { return resnet_trunk(c) || seq_trunk(c); }
static const char* level_names(const milan_ctx* c) {
  return seq_trunk(c) ? seq_family(c->d.trunk_kind)->levels : "conv1, layer1..layer4";
}
// the width of level l of a sequential net
static int seq_channels(const milan_ctx* c, int l) {
  return vgg_trunk(c) ? c->vgg[l][0].cout : c->alex[l].cout;
}
static int level_channels(const milan_ctx* c, int level) {
  const int wd = c->d.trunk_width;
  if (level == 0) return wd;
  return (c->d.trunk_kind == MILAN_TRUNK_BASIC ? wd : wd * 4) << (level - 1);
}

// the context's mask table: `channels[l]` units on level l, none of them ablated
static int init_mask_table(milan_ctx* c, const int* channels, hipStream_t s) {
  int total = 0;
  for (int l = 0; l < 5; ++l) {
    c->abl_ch[l] = channels[l];
    c->abl_off[l] = total;
    total += channels[l];
    c->abl_count[l] = 0;
  }
  MILAN_TRY(dev_alloc(c, (void**)&c->abl_mask, sizeof(float) * total));
  hipLaunchKernelGGL(fill_ones_kernel, dim3((total + 255) / 256), dim3(256), 0, s, c->abl_mask,
                     total);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// called from milan_finalize_weights after encoder_finalize: keeps fc.weight / fc.bias when the
// state dict has them (a context without them runs everything but the classify calls)
int classify_finalize(milan_ctx* c, hipStream_t s) {
  const SeqFamily* fam = seq_family(c->d.trunk_kind);
  if ((fam == nullptr && !resnet_trunk(c)) || c->stem.w == nullptr) return 0;
  int channels[5];
  if (fam != nullptr) {
    // (torchvision's AlexNet gets its table with its head: until then it only encodes)
    if (fam->no_head == nullptr) return 0;
    // (vgg_first_kernel keeps 28 x width floats in LDS)
    MILAN_REQUIRE(!fam->vgg || c->d.trunk_width <= 512, MILAN_ERR_SHAPE,
                  "the VGG trunk takes widths up to 512 (got %d)", c->d.trunk_width);
    for (int l = 0; l < 5; ++l) channels[l] = seq_channels(c, l);
    return init_mask_table(c, channels, s);
  }
  for (int l = 0; l < 5; ++l) channels[l] = level_channels(c, l);
  MILAN_TRY(init_mask_table(c, channels, s));
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
                  "%s: level %d is not one of 0..4 (%s)", what, levels[i], level_names(c));
    MILAN_REQUIRE(units[i] >= 0 && units[i] < c->abl_ch[levels[i]], MILAN_ERR_INDEX,
                  "%s: index %d is out of bounds for level %d with %d units", what, units[i],
                  levels[i], c->abl_ch[levels[i]]);
  }
  return 0;
}

int classify_set_ablation(milan_ctx* c, const int32_t* levels, const int32_t* units, int count,
                          hipStream_t s) {
  MILAN_REQUIRE(classifier_trunk(c), MILAN_ERR_ARG,
                "unit ablation needs a ResNet trunk, a Places365 AlexNet trunk, or an AlexNet "
                "trunk whose head milan_set_alexnet_head has installed");
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
// driver: one pass loop, one sweep loop and one workspace dry run, written over
// a trunk.  A trunk (ResNetTrunk; SeqTrunk, which walks the AlexNets and the VGGs) is one
// pass's plan and walker: it derives from Trunk, fills h / w / lvl_sz and split_tap_scale when it is made, and
// supplies
//   carve(a)           its own buffers out of the arena, in its own order
//   carve_hold(a, f)   the sweep's room of `f` floats for a held level, if it needs one
//   check_geometry()   what it asks of the image extent
//   walk(from, to, src, &out)   the forward between two levels (see ResNetTrunk::walk)
//   head(x4, logits, preds)     from the masked level-4 tensor to logits (+ argmax)
//   hold_level(images, at, level, &held)   the sweep's step to the next level with units
// ---------------------------------------------------------------------------
struct Trunk {
  const milan_ctx* c;
  int n, hin, win;        // the pass's images and their extent
  bool split;
  hipStream_t s;
  float split_tap_scale;  // what a split level's stored value is multiplied by on its way out
  int h[5], w[5];         // extent of the five level tensors
  size_t lvl_sz[5];       // floats per image of a level's tensor (split takes the same room)
  long long* preds = nullptr;
  float *logits = nullptr, *work = nullptr;
  float* tap[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // whether a level's tensor is in split format (a trunk's constructor fills it: level 0 is
  // fp32 on the ResNets and the AlexNets, the Places365 AlexNet and the narrow VGGs have fp32
  // levels above it too)
  bool fmt[5] = {false, false, false, false, false};

  // level tensor `x` -> `y` (x == y: in place), times the context's mask of that level and with
  // unit `extra` (>= 0) zeroed too
  int mask(int level, const float* x, float* y, int extra) const {
    const int C = c->abl_ch[level];
    const long px = (long)n * h[level] * w[level];
    const float* m = c->abl_mask + c->abl_off[level];
    if (fmt[level]) {
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
  // fp32 without any scale in both modes on both trunks.
  int emit(int level, const float* x) const {
    const int C = c->abl_ch[level], P = h[level] * w[level];
    const dim3 grid((P + TAP_P - 1) / TAP_P, (C + TAP_C - 1) / TAP_C, n);
    if (fmt[level])
      hipLaunchKernelGGL(tap_nchw_kernel<true>, grid, dim3(256), 0, s, x, P, C, split_tap_scale,
                         tap[level]);
    else
      hipLaunchKernelGGL(tap_nchw_kernel<false>, grid, dim3(256), 0, s, x, P, C, 1.f,
                         tap[level]);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }
};

// `preds` comes first, so that its address does not depend on the pass's image count; then the
// trunk's buffers, the logits of one pass and the sweep's held and working tensors
template <class T>
static void carve(T& t, int sweep_units, int n_total, Arena& a) {
  const size_t lvl_max = *std::max_element(t.lvl_sz, t.lvl_sz + 5);
  t.preds = sweep_units > 0 ? a.get<long long>((size_t)sweep_units * n_total) : nullptr;
  t.carve(a);
  t.logits = a.get<float>((size_t)t.n * (t.c->fc_classes > 0 ? t.c->fc_classes : 1));
  if (sweep_units > 0) {
    t.carve_hold(a, (size_t)t.n * lvl_max);
    t.work = a.get<float>((size_t)t.n * lvl_max);
  }
}

// ResNet: level 0 is the raw conv1 output (fp32 in both modes: the pair stem's weight scale
// leaves in the GEMM's acc_scale, the activation scale enters only with bn1_scale_s), level 1
// the maxpool's and layer1's extent, levels 2..4 layer2..4.  Levels 1..4 live in two ping-pong
// buffers, split at the context's activation scale in the split mode.
struct ResNetTrunk : Trunk {
  float *in4, *raw, *x0, *x1, *ds, *t1, *t2, *hold = nullptr, *pooled;
  EncBuffers geo;  // the encoder pass's level extents and buffer sizes (enc_carve)

  ResNetTrunk(const milan_ctx* c, int n, int H, int W, bool split, hipStream_t s)
      : Trunk{c, n, H, W, split, s, 1.f / c->act_scale} {
    enc_carve(c->d.trunk_kind, c->d.trunk_width, n, H, W, nullptr, &geo);
    for (int l = 0; l < 5; ++l) {
      h[l] = geo.lv.h[l]; w[l] = geo.lv.w[l];
      lvl_sz[l] = (size_t)h[l] * w[l] * level_channels(c, l);
    }
    for (int l = 1; l < 5; ++l) fmt[l] = split;
  }

  void carve(Arena& a) {
    in4 = a.get<float>((size_t)n * hin * (win + 2) * 4);
    raw = a.get<float>((size_t)n * lvl_sz[0]);
    x0 = a.get<float>((size_t)n * geo.x_sz);
    x1 = a.get<float>((size_t)n * geo.x_sz);
    ds = a.get<float>((size_t)n * geo.x_sz);
    t1 = a.get<float>((size_t)n * geo.t1_sz);
    t2 = a.get<float>((size_t)n * geo.t2_sz);
    pooled = a.get<float>((size_t)n * level_channels(c, 4));
  }
  void carve_hold(Arena& a, size_t floats) { hold = a.get<float>(floats); }
  int check_geometry() const { return 0; }

  // Runs the forward from level `from` (-1: from `src` = the images; otherwise `src` is the
  // level's tensor with its mask already applied) up to and including level `to`, applying the
  // context's masks to every level it produces.  *out = the level-`to` tensor.  Every level
  // it produces that has a tap[] pointer is also written there, after its mask.
  int walk(int from, int to, const float* src, const float** out) const {
    const float* x = src;
    if (from < 0) {
      const bool pair_stem = split && c->stem_pair.ws != nullptr;
      MILAN_TRY(launch_raw_input(src, n, hin, win, pair_stem, in4, c->status, s));
      MILAN_TRY(launch_gemm(encoder_stem_args(c, in4, n, hin, win, raw, pair_stem), s));
      if (c->abl_count[0] > 0) MILAN_TRY(mask(0, raw, raw, -1));
      x = raw;
      from = 0;
      if (tap[0]) MILAN_TRY(emit(0, x));
    }
    if (to == from) { *out = x; return 0; }
    float* y = x0;
    if (from == 0) {
      MILAN_TRY(launch_stem_tail(c, x, n, h[0], w[0], h[1], w[1], split, x0, s));
      x = x0; y = x1;
    }
    int hh = h[from == 0 ? 1 : from], ww = w[from == 0 ? 1 : from];
    for (int li = from == 0 ? 0 : from; li < 4 && li < to; ++li) {
      for (const Bottleneck& b : c->blocks[li]) {
        int h1, w1, h2, w2, h3, w3, hd, wdn;
        const float* identity = x;
        if (b.has_down) {
          MILAN_TRY(launch_gemm(encoder_conv_args(b.down, x, n, hh, ww, ds, EPI_BIAS, nullptr,
                                                  c->zero, &hd, &wdn, split), s));
          identity = ds;
        }
        MILAN_TRY(launch_gemm(encoder_conv_args(b.c1, x, n, hh, ww, t1, EPI_BIAS_RELU, nullptr,
                                                c->zero, &h1, &w1, split), s));
        if (b.basic) {
          // BasicBlock: relu(bn2(conv2(relu(bn1(conv1(x))))) + identity)
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c2, t1, n, h1, w1, y, EPI_BIAS_RES_RELU,
                                                  identity, c->zero, &h3, &w3, split), s));
        } else {
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c2, t1, n, h1, w1, t2, EPI_BIAS_RELU,
                                                  nullptr, c->zero, &h2, &w2, split), s));
          MILAN_TRY(launch_gemm(encoder_conv_args(b.c3, t2, n, h2, w2, y, EPI_BIAS_RES_RELU,
                                                  identity, c->zero, &h3, &w3, split), s));
        }
        // the block's output becomes the next input; the other ping-pong buffer the next output
        // (an input that came from outside -- the sweep's working tensor -- is left alone)
        const float* nx = y;
        y = (x == x0 || x == x1) ? const_cast<float*>(x) : (y == x0 ? x1 : x0);
        x = nx;
        hh = h3; ww = w3;
      }
      MILAN_REQUIRE(hh == h[li + 1] && ww == w[li + 1], MILAN_ERR_SHAPE,
                    "internal: stage %d geometry mismatch", li + 1);
      if (c->abl_count[li + 1] > 0)
        MILAN_TRY(mask(li + 1, x, const_cast<float*>(x), -1));
      if (tap[li + 1]) MILAN_TRY(emit(li + 1, x));
    }
    *out = x;
    return 0;
  }

  // avgpool + fc (+ argmax) of the masked level-4 tensor
  int head(const float* x4, float* lg, long long* pr) const {
    const int C = c->abl_ch[4], P = h[4] * w[4], K = c->fc_classes;
    if (split)
      hipLaunchKernelGGL(avgpool_kernel<true>, dim3((C + 255) / 256, n), dim3(256), 0, s, x4, P, C,
                         1.f / c->act_scale, pooled);
    else
      hipLaunchKernelGGL(avgpool_kernel<false>, dim3((C + 255) / 256, n), dim3(256), 0, s, x4, P,
                         C, 1.f, pooled);
    hipLaunchKernelGGL(fc_kernel, dim3((K + 3) / 4, n), dim3(256), 0, s, pooled, c->fc_w,
                       c->fc_b, C, K, lg);
    if (pr) hipLaunchKernelGGL(row_argmax_kernel, dim3(n), dim3(64), 0, s, lg, K, pr);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }

  // The sweep's forward up to and including `level` starts from the images every time: levels
  // >= 1 live in the ping-pong buffers the suffix overwrites, so they are copied into `hold`
  // (the raw conv1 tensor has a buffer of its own).
  int hold_level(const float* images, int, int level, const float** held) const {
    MILAN_TRY(walk(-1, level, images, held));
    if (level > 0) {
      MILAN_CHECK_HIP(hipMemcpyAsync(hold, *held, sizeof(float) * n * lvl_sz[level],
                                     hipMemcpyDeviceToDevice, s));
      *held = hold;
    }
    return 0;
  }
};

// One step of a sequential net's pass.  A step reads what the step in front of it
// wrote (the first one of a walk: the walk's `src`).
struct SeqStep {
  // RAW: the image -> NHWC4 fp32 for an AlexNet's conv1; VGG_FIRST: the image -> relu(conv1_1 +
  // bias), vgg_first_kernel; POOL3 / POOL2: the 3x3 / 2 and 2x2 / 2 max-pools; CONV: relu(conv +
  // bias) on the GEMM tile
  enum Kind { RAW, VGG_FIRST, POOL3, POOL2, LRN, CONV } kind;
  const ConvW* cw;           // CONV, VGG_FIRST
  int hi, wi, ho, wo, C;     // extents of what it reads and writes, channels of what it writes
  bool in_split, out_split;  // the formats it reads and writes (SeqTrunk::formats)
  int dst;                   // the buffer it writes (SeqTrunk::buf)
  int level;                 // -1, or the level whose tensor it writes: mask and emit follow
  int slot;                  // its slot in milan_vgg_trace, or -1
};

// VGG: every pool halves (floor), so level l needs 2^l pixels each way; a walk asks before it
// launches anything, milan_activations per requested level.  (The AlexNets ask pass by pass and
// pool by pool: SeqTrunk::check_geometry, walk.)
static int seq_reach(const milan_ctx* c, int H, int W, int to) {
  MILAN_REQUIRE(!vgg_trunk(c) || to < 0 || ((H >> to) >= 1 && (W >> to) >= 1), MILAN_ERR_SHAPE,
                "classify: image %dx%d is too small for VGG level %d (%dx%d at least)", H, W, to,
                1 << (to < 0 ? 0 : to), 1 << (to < 0 ? 0 : to));
  return 0;
}

// The sequential nets in eval mode: torchvision's alexnet_seq (4.23), the
// Places365 AlexNet (4.27; the reference's src/deps/alexnet.py) and torchvision's VGG-11 / 13 /
// 16 / 19 without batch norm (4.30), each walked from a step plan that the constructor fills.
// A level's tensor is relu(conv + bias) * mask, the conv run with the encoder's bias + ReLU
// epilogue (no mask launch for a level without units).  Every level has a buffer of its own, so
// the sweep holds a level where it is.
//   AlexNets: levels 0..4 are conv1..conv5, shapes, paddings and groups in c->alex (AlexSpec,
//   DESIGN 4.28; a grouped conv is one launch, the group a grid dimension); pool1 and pool2,
//   each with the Places net's optional LRN behind it (c->lrn), sit in front of conv2 and conv3.
//   VGG: five blocks of 3x3 / pad 1 convs (c->vgg, as the uploaded keys gave them), a 2x2 / 2
//   pool in front of blocks 2..5; level l is the last conv of block l + 1.  The convs inside a
//   block and the pools write two scratch buffers in turn; conv1_1 reads the image itself.
// What the families differ in besides the plan is their row of SeqFamily (common.h).
struct SeqTrunk : Trunk {
  const SeqFamily& fam;
  SeqStep st[32];
  int ns = 0;
  int end[5] = {0, 0, 0, 0, 0};  // one past the step that writes level l
  size_t bsz[12];                // floats per image of buffer i, in carve order
  int nbuf = 0;
  float *buf[12], *flat, *f6, *f7;
  int th, tw;                    // pool5's extent, which the head's tail kernel reads
  int hh, ww;                    // (while the plan is made: the extent in flight)

  SeqTrunk(const milan_ctx* c, int n, int H, int W, bool split, hipStream_t s)
      : Trunk{c, n, H, W, split, s, 1.f}, fam(*seq_family(c->d.trunk_kind)), hh(H), ww(W) {
    if (fam.vgg) plan_vgg(); else plan_alexnet();
    formats();
  }

  int buffer(size_t floats) { bsz[nbuf] = floats; return nbuf++; }
  SeqStep& step(SeqStep::Kind kind, const ConvW* cw, int ho, int wo, int C, int dst,
                int level = -1, int slot = -1) {
    st[ns] = SeqStep{kind, cw, hh, ww, ho, wo, C, false, false, dst, level, slot};
    hh = ho; ww = wo;
    if (level >= 0) end[level] = ns + 1;
    return st[ns++];
  }

  // buffers: in4, a[0..4], then q[0], qn[0], q[1], qn[1] (the LRN's qn with c->lrn alone)
  void plan_alexnet() {
    int hq[3], wq[3], a[5], q[2], qn[2];
    alex_geometry(c, hin, win, h, w, hq, wq);
    // (an image too small for the trunk is refused before anything is used: check_geometry)
    for (int l = 0; l < 5; ++l)
      lvl_sz[l] = (size_t)std::max(h[l], 0) * std::max(w[l], 0) * c->abl_ch[l];
    th = hq[2]; tw = wq[2];
    const int in4 = buffer((size_t)hin * win * 4);
    for (int l = 0; l < 5; ++l) a[l] = buffer(lvl_sz[l]);
    for (int l = 0; l < 2; ++l) {
      const size_t sz = (size_t)std::max(hq[l], 0) * std::max(wq[l], 0) * c->abl_ch[l];
      q[l] = buffer(sz);
      qn[l] = c->lrn.size > 0 ? buffer(sz) : -1;
    }
    step(SeqStep::RAW, nullptr, hin, win, 4, in4);
    for (int l = 0; l < 5; ++l) {
      if (l == 1 || l == 2) {
        step(SeqStep::POOL3, nullptr, hq[l - 1], wq[l - 1], c->abl_ch[l - 1], q[l - 1]);
        if (qn[l - 1] >= 0) step(SeqStep::LRN, nullptr, hh, ww, c->abl_ch[l - 1], qn[l - 1]);
      }
      // (h[l] x w[l] is what the launch computes: alex_geometry reads the same ConvW)
      step(SeqStep::CONV, &c->alex[l], h[l], w[l], c->abl_ch[l], a[l], l);
    }
  }

  // buffers: lv[0..4], then the two scratch buffers, each as large as the largest level (a
  // pool's output is no larger than the level behind it, a conv's inside block b as large)
  void plan_vgg() {
    int lv[5], sc[2];
    h[0] = hin; w[0] = win;
    for (int l = 1; l < 5; ++l) { h[l] = h[l - 1] / 2; w[l] = w[l - 1] / 2; }
    for (int l = 0; l < 5; ++l) lvl_sz[l] = (size_t)h[l] * w[l] * c->abl_ch[l];
    th = h[4] / 2; tw = w[4] / 2;
    for (int l = 0; l < 5; ++l) lv[l] = buffer(lvl_sz[l]);
    for (int k = 0; k < 2; ++k) sc[k] = buffer(*std::max_element(lvl_sz, lvl_sz + 5));
    for (int b = 0; b < 5; ++b) {
      const int nb = c->vgg_n[b];
      if (b > 0) step(SeqStep::POOL2, nullptr, h[b], w[b], c->abl_ch[b - 1], sc[0]);
      for (int j = 0; j < nb; ++j) {
        // (the level's buffer, or the scratch buffer that the input is not in)
        const int dst = j == nb - 1 ? lv[b] : (ns > 0 && st[ns - 1].dst == sc[0] ? sc[1] : sc[0]);
        const int level = j == nb - 1 ? b : -1;
        if (b > 0 || j > 0) {
          step(SeqStep::CONV, &c->vgg[b][j], h[b], w[b], c->abl_ch[b], dst, level, 4 * b + j);
          continue;
        }
        // vgg_first_kernel writes the format that the second conv of the net can take, also
        // across a pool (vgg11: level 0 is then a split tensor and pool1 reads one)
        const ConvW& second = nb > 1 ? c->vgg[0][1] : c->vgg[1][0];
        step(SeqStep::VGG_FIRST, &c->vgg[0][0], h[0], w[0], c->abl_ch[0], dst, level, 0)
            .out_split = split && second.ws != nullptr;
      }
    }
  }

  // The format rule of the split mode, once for every plan.  A conv multiplies split operands
  // (in_split) when its weights have a split copy and its input can arrive split: a pool
  // converts fp32 to split on the way, a conv that reads split operands writes either format, a
  // conv that reads fp32 writes fp32 (conv1 of an AlexNet: 3 input channels).  A step then
  // writes what its reader takes: a pool and an LRN the format of the next conv, a conv in
  // front of a conv that conv's (an fp32 conv behind a split one gets fp32, GemmArgs::out_split
  // = 0), a conv in front of a pool or the head the format it reads itself.  There is no
  // conversion back to fp32 except that hand-over; walk() asserts that none is needed.  The one
  // step outside the rule is VGG_FIRST, whose format plan_vgg has set.  Split activations sit
  // at scale 1.
  void formats() {
    bool can = false;   // the tensor in flight can be had in split format
    for (int k = 0; k < ns; ++k) {
      SeqStep& t = st[k];
      if (t.kind == SeqStep::CONV) can = t.in_split = split && t.cw->ws != nullptr && can;
      else if (t.kind == SeqStep::POOL3 || t.kind == SeqStep::POOL2) can = true;
      else if (t.kind == SeqStep::VGG_FIRST) can = t.out_split;
    }
    bool next = false;  // what the next conv down the plan reads
    for (int k = ns - 1; k >= 0; --k) {
      SeqStep& t = st[k];
      if (t.kind == SeqStep::CONV) {
        t.out_split = k + 1 < ns && st[k + 1].kind == SeqStep::CONV ? next : t.in_split;
        next = t.in_split;
      } else if (t.kind != SeqStep::VGG_FIRST) {
        t.out_split = next;
      }
    }
    for (int k = 1; k < ns; ++k)
      if (st[k].kind != SeqStep::CONV) st[k].in_split = st[k - 1].out_split;
    for (int l = 0; l < 5; ++l) fmt[l] = end[l] > 0 && st[end[l] - 1].out_split;
  }

  void carve(Arena& ar) {
    const milan_ctx::AlexHead& hd = c->ahead;
    for (int i = 0; i < nbuf; ++i) buf[i] = ar.get<float>((size_t)n * bsz[i]);
    flat = ar.get<float>((size_t)n * hd.in[0]);
    f6 = ar.get<float>((size_t)n * hd.out[0]);
    f7 = ar.get<float>((size_t)n * hd.out[1]);
  }
  void carve_hold(Arena&, size_t) {}

  // torchvision's AlexNet: the smallest image leaves one pixel after pool5 (63 x 63).  Places:
  // conv1 needs an 11 x 11 image; a pool needs 3 pixels each way, which walk() asks for when it
  // has to cross one (19 x 19 reaches conv2, 35 x 35 every level); a classify call needs 6 x 6
  // after pool5 (SeqFamily::tail_lo, classify_checks).  VGG: seq_reach.
  int check_geometry() const {
    if (fam.vgg) return 0;
    const bool places = places_trunk(c);
    // (the unpadded conv1: C's division rounds the extent of a smaller image up to 1)
    MILAN_REQUIRE(!places || (hin >= 11 && win >= 11 && h[0] >= 1 && w[0] >= 1), MILAN_ERR_SHAPE,
                  "classify: image %dx%d is too small for the Places365 AlexNet's 11x11 conv1",
                  hin, win);
    // (the three pools need 3 pixels each way: C's division rounds a negative extent to zero)
    MILAN_REQUIRE(places ||
                      (h[0] >= 3 && w[0] >= 3 && h[1] >= 3 && w[1] >= 3 && h[4] >= 3 && w[4] >= 3),
                  MILAN_ERR_SHAPE,
                  "classify: image %dx%d is too small for AlexNet (63x63 at least)", hin, win);
    return 0;
  }

  // ResNetTrunk::walk's contract: the steps between two level boundaries
  int walk(int from, int to, const float* src, const float** out) const {
    MILAN_TRY(seq_reach(c, hin, win, to));
    const float* x = src;
    bool xs = from >= 0 && fmt[from];   // the format of x
    int at = from;                      // the level behind x
    for (int k = from < 0 ? 0 : end[from]; to >= 0 && k < end[to]; ++k) {
      const SeqStep& t = st[k];
      float* y = buf[t.dst];
      const bool conv = t.kind == SeqStep::CONV;
      MILAN_REQUIRE(t.in_split == xs && (conv ? t.in_split || !t.out_split
                                              : t.out_split || !t.in_split),
                    MILAN_ERR_STATE,
                    "internal: step %d towards level %d would read a tensor of the other format, "
                    "write split from fp32 operands, or convert split to fp32", k, at + 1);
      switch (t.kind) {
        case SeqStep::RAW:
          MILAN_TRY(launch_raw_input(x, n, t.hi, t.wi, false, y, c->status, s));
          break;
        case SeqStep::VGG_FIRST:
          MILAN_TRY(launch_vgg_first(x, n, t.hi, t.wi, t.C, c->vgg_w27, t.cw->bias, t.out_split,
                                     y, c->status, s));
          break;
        case SeqStep::POOL3:
          // (torchvision's net has asked for all three pools in check_geometry)
          MILAN_REQUIRE(t.hi >= 3 && t.wi >= 3, MILAN_ERR_SHAPE,
                        "classify: image %dx%d is too small for the Places365 AlexNet: pool%d "
                        "needs 3x3 pixels and gets %dx%d (19x19 reaches conv2, 35x35 every level)",
                        hin, win, at + 1, t.hi, t.wi);
          MILAN_TRY(launch_maxpool3s2(x, n, t.hi, t.wi, t.C, t.ho, t.wo, t.out_split, t.in_split,
                                      y, c->status, s));
          break;
        case SeqStep::POOL2:
          MILAN_TRY(launch_maxpool2s2(x, n, t.hi, t.wi, t.C, t.in_split, t.out_split, y,
                                      c->status, s));
          break;
        case SeqStep::LRN:
          MILAN_TRY(launch_lrn(x, (long long)n * t.hi * t.wi, t.C, t.in_split, c->lrn.size,
                               c->lrn.alpha, c->lrn.beta, y, c->status, s));
          break;
        case SeqStep::CONV: {
          int ho, wo;
          GemmArgs g = encoder_conv_args(*t.cw, x, n, t.hi, t.wi, y, EPI_BIAS_RELU, nullptr,
                                         c->zero, &ho, &wo, t.in_split, false);
          if (!t.out_split) g.out_split = 0;   // (a split conv in front of an fp32 one)
          MILAN_TRY(launch_gemm(g, s));
          break;
        }
      }
      if (t.slot >= 0) {
        ++c->vgg_launches[t.slot];
        c->vgg_split[t.slot] = t.in_split;
      }
      x = y; xs = t.out_split;
      if (t.level < 0) continue;
      at = t.level;
      if (c->abl_count[at] > 0) MILAN_TRY(mask(at, y, y, -1));
      if (tap[at]) MILAN_TRY(emit(at, x));
    }
    *out = x;
    return 0;
  }

  // pool5 + adaptive average pool + flatten in (C, h, w) order (the family's tail kernel: the two
  // add up their bins in different orders), fc6 / fc7 / linear8 or classifier.0 / .3 / .6 (+
  // argmax) of the masked level-4 tensor; dropout is the identity in eval mode.  The Places net
  // has no adaptive pool: with the 6 x 6 pooled pixels it requires, every bin of
  // alex_tail_kernel's average is one pixel, divided by 1.
  int head(const float* x4, float* lg, long long* pr) const {
    const milan_ctx::AlexHead& hd = c->ahead;
    const int C = c->abl_ch[4];
    MILAN_REQUIRE(hd.installed && std::min(th, tw) >= fam.tail_lo &&
                      std::max(th, tw) <= fam.tail_hi,
                  MILAN_ERR_STATE,
                  "internal: head without fc layers or with %d x %d pixels after pool5", th, tw);
    const dim3 grid((fam.bins * fam.bins * C + 255) / 256, n);
    const auto vgg_tail = fmt[4] ? vgg_tail_kernel<true> : vgg_tail_kernel<false>;
    const auto alex_tail = fmt[4] ? alex_tail_kernel<true> : alex_tail_kernel<false>;
    if (fam.vgg)
      hipLaunchKernelGGL(vgg_tail, grid, dim3(256), 0, s, x4, h[4], w[4], C, th, tw, flat);
    else
      hipLaunchKernelGGL(alex_tail, grid, dim3(256), 0, s, x4, h[4], w[4], C, th, tw, 1.f, flat);
    MILAN_CHECK_HIP(hipGetLastError());
    MILAN_TRY(linear_run(flat, hd.w[0], hd.b[0], n, hd.in[0], hd.out[0], true, f6, s));
    MILAN_TRY(linear_run(f6, hd.w[1], hd.b[1], n, hd.in[1], hd.out[1], true, f7, s));
    MILAN_TRY(linear_run(f7, hd.w[2], hd.b[2], n, hd.in[2], hd.out[2], false, lg, s));
    if (pr) {
      hipLaunchKernelGGL(row_argmax_kernel, dim3(n), dim3(64), 0, s, lg, hd.out[2], pr);
      MILAN_CHECK_HIP(hipGetLastError());
    }
    return 0;
  }

  // The sweep's walk to `level` continues from the level held before it (`at`, -1: the
  // images): the suffixes write levels above their own and the working tensor, never a held one.
  int hold_level(const float* images, int at, int level, const float** held) const {
    return walk(at, level, at < 0 ? images : *held, held);
  }
};

template <class T>
static size_t workspace_dry(const milan_ctx* c, int n_images, int H, int W, int sweep_units) {
  Arena a; a.dry = true;
  const int sub = encoder_sub_batch_size();
  T t(c, n_images < sub ? n_images : sub, H, W, false, nullptr);
  carve(t, sweep_units < 0 ? 0 : sweep_units, n_images, a);
  return a.off;
}

size_t classify_workspace(const milan_ctx* c, int n_images, int H, int W, int sweep_units) {
  if (n_images <= 0 || H < 1 || W < 1) return 0;
  if (seq_trunk(c)) return workspace_dry<SeqTrunk>(c, n_images, H, W, sweep_units);
  if (resnet_trunk(c)) return workspace_dry<ResNetTrunk>(c, n_images, H, W, sweep_units);
  return 0;
}

// The pass loop: `n` images in slices of the encoder's sub-batch size, every pass on the same
// scratch.  body(t, lo) runs on the pass's trunk `t`; `lo` is its first image.
template <class T, class Body>
static int for_each_pass(const milan_ctx* c, int n, int H, int W, bool split, int sweep_units,
                         const char* what, const Arena& ws, hipStream_t s, Body body) {
  const int sub = encoder_sub_batch_size();
  for (int lo = 0; lo < n; lo += sub) {
    const int cnt = n - lo < sub ? n - lo : sub;
    Arena a = ws;
    T t(c, cnt, H, W, split, s);
    carve(t, sweep_units, n, a);
    MILAN_TRY(t.check_geometry());
    MILAN_REQUIRE(a.off <= a.size, MILAN_ERR_WORKSPACE,
                  "%s: workspace too small (%zu needed, %zu given)", what, a.off, a.size);
    // (the image index is a grid's y or z in the taps, the pools and the heads)
    MILAN_REQUIRE(cnt <= 65535, MILAN_ERR_ARG, "%s: sub-batch of %d images", what, cnt);
    MILAN_TRY(body(t, lo));
  }
  return 0;
}

// milan_classify (taps == nullptr: walk to level 4, then the head) and milan_activations
// (taps[l] != nullptr for the requested levels, `top` the highest: each one converted to fp32
// NCHW when it is produced; no head)
template <class T>
static int run(milan_ctx* c, const float* images, int n, int H, int W, bool split, float* logits,
               int64_t* predictions, float* const* taps, int top, const char* what, Arena& ws,
               hipStream_t s) {
  return for_each_pass<T>(c, n, H, W, split, 0, what, ws, s, [&](T& t, int lo) -> int {
    const float* from = images + (size_t)lo * 3 * H * W;
    const float* x;
    if (taps) {
      for (int l = 0; l < 5; ++l)
        if (taps[l]) t.tap[l] = taps[l] + (size_t)lo * t.lvl_sz[l];
      return t.walk(-1, top, from, &x);
    }
    MILAN_TRY(t.walk(-1, 4, from, &x));
    float* lg = logits ? logits + (size_t)lo * c->fc_classes : t.logits;
    return t.head(x, lg, predictions ? (long long*)predictions + lo : nullptr);
  });
}

// Units grouped by level, levels ascending: the forward up to and including a level runs once
// per pass with the base set's masks and is held (T::hold_level); every unit is one masked copy
// into the working tensor plus the suffix and the head.
template <class T>
static int sweep(milan_ctx* c, const float* images, int n, int H, int W, bool split,
                 const int32_t* levels, const int32_t* units, int count, const int64_t* targets,
                 int32_t* correct, int64_t* predictions, Arena& ws, hipStream_t s) {
  long long* preds_all = (long long*)predictions;
  MILAN_TRY(for_each_pass<T>(c, n, H, W, split, count, "classify_sweep", ws, s,
                             [&](T& t, int lo) -> int {
    if (preds_all == nullptr) preds_all = t.preds;   // (the same address in every pass)
    const float* from = images + (size_t)lo * 3 * H * W;
    const float* held = nullptr;
    int at = -1;
    for (int level = 0; level < 5; ++level) {
      bool any = false;
      for (int j = 0; j < count && !any; ++j) any = levels[j] == level;
      if (!any) continue;
      MILAN_TRY(t.hold_level(from, at, level, &held));
      at = level;
      for (int j = 0; j < count; ++j) {
        if (levels[j] != level) continue;
        MILAN_TRY(t.mask(level, held, t.work, units[j]));
        const float* x4;
        MILAN_TRY(t.walk(level, 4, t.work, &x4));
        MILAN_TRY(t.head(x4, t.logits, preds_all + (size_t)j * n + lo));
      }
    }
    return 0;
  }));
  if (correct != nullptr) {
    hipLaunchKernelGGL(correct_count_kernel, dim3(count), dim3(256), 0, s, preds_all,
                       (const long long*)targets, n, correct);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// milan_set_alexnet_head (fc6 / fc7 / linear8) and milan_set_vgg_head (classifier.0 / .3 / .6):
// the three Linear layers (device fp32, row-major (out, in)) packed into library-owned memory.
// `asked`: a row of the family that the entry point serves.  Switches the classify family on
// for a torchvision AlexNet context.
int classify_set_head(milan_ctx* c, const SeqFamily& asked, const float* const* w,
                      const float* const* b, const int* out, const int* in, hipStream_t s) {
  const SeqFamily* fam = seq_family(c->d.trunk_kind);
  const char* what = asked.setter;
  MILAN_REQUIRE(fam != nullptr && fam->vgg == asked.vgg, MILAN_ERR_ARG,
                "%s: the context's trunk is not %s", what, asked.trunk);
  MILAN_REQUIRE(c->stem.w != nullptr, MILAN_ERR_STATE, "encoder weights were not uploaded");
  int channels[5];
  for (int l = 0; l < 5; ++l) channels[l] = seq_channels(c, l);
  const int per = fam->bins * fam->bins;
  MILAN_REQUIRE(out[0] >= 1 && out[1] >= 1 && out[2] >= 1 && in[0] == channels[4] * per &&
                    in[1] == out[0] && in[2] == out[1],
                MILAN_ERR_SHAPE,
                "%s: %s (%d, %d), %s (%d, %d), %s (%d, %d) do not chain from %d x %d features",
                what, fam->fc[0], out[0], in[0], fam->fc[1], out[1], in[1], fam->fc[2], out[2],
                in[2], channels[4], per);
  milan_ctx::AlexHead& hd = c->ahead;
  for (int i = 0; i < 3; ++i) {
    // (a second call with the same widths reuses the first one's memory)
    MILAN_REQUIRE(hd.w[i] == nullptr || (hd.out[i] == out[i] && hd.in[i] == in[i]),
                  MILAN_ERR_STATE, "%s: a head of other widths is installed", what);
    if (hd.w[i] == nullptr) {
      MILAN_TRY(dev_alloc(c, (void**)&hd.w[i], sizeof(float) * linear_packed_floats(out[i], in[i])));
      MILAN_TRY(dev_alloc(c, (void**)&hd.b[i], sizeof(float) * (size_t)out[i]));
    }
    hd.out[i] = out[i]; hd.in[i] = in[i];
    MILAN_TRY(linear_pack(w[i], out[i], in[i], hd.w[i], s));
    MILAN_CHECK_HIP(hipMemcpyAsync(hd.b[i], b[i], sizeof(float) * (size_t)out[i],
                                   hipMemcpyDeviceToDevice, s));
  }
  if (c->abl_mask == nullptr) MILAN_TRY(init_mask_table(c, channels, s));
  // (the caller's tensors may go once this returns)
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  c->fc_classes = out[2];
  c->fc_in = in[2];
  hd.installed = true;
  return 0;
}

// milan_set_alexnet_lrn: the Places trunk's optional LRN after pool1 and pool2 (0: off)
int classify_set_alexnet_lrn(milan_ctx* c, int local_size, float alpha, float beta) {
  MILAN_REQUIRE(places_trunk(c), MILAN_ERR_ARG,
                "milan_set_alexnet_lrn: the context's trunk is not the Places365 AlexNet");
  MILAN_REQUIRE(local_size == 0 || (local_size >= 1 && local_size % 2 == 1 && local_size <= 17),
                MILAN_ERR_ARG,
                "milan_set_alexnet_lrn: local_size %d is neither 0 (off) nor an odd number in 1..17",
                local_size);
  c->lrn.size = local_size;
  c->lrn.alpha = alpha;
  c->lrn.beta = beta;
  return 0;
}

int linear_rowwise_run(const float* x, const float* W, const float* bias, int M, int K, int N,
                       float* y, hipStream_t s) {
  MILAN_REQUIRE(x && W && y && M >= 1 && M <= 65535 && K >= 1 && N >= 1, MILAN_ERR_ARG,
                "linear_rowwise: bad argument");
  hipLaunchKernelGGL(fc_kernel, dim3((N + 3) / 4, M), dim3(256), 0, s, x, W, bias, K, N, y);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// milan_vgg_trace counts from the start of a classify-family call
static void vgg_trace_reset(const milan_ctx* c) {
  for (int i = 0; i < 20; ++i) c->vgg_launches[i] = c->vgg_split[i] = 0;
}

// `head`: the call runs avgpool + fc (milan_activations stops before them and does not)
static int classify_checks(milan_ctx* c, int n, int H, int W, bool* split, bool head = true) {
  MILAN_REQUIRE(classifier_trunk(c), MILAN_ERR_ARG,
                "classification needs a ResNet trunk, a Places365 AlexNet trunk, or an AlexNet "
                "trunk whose head milan_set_alexnet_head has installed");
  MILAN_REQUIRE(c->stem.w != nullptr && c->abl_mask != nullptr, MILAN_ERR_STATE,
                "encoder weights were not uploaded");
  const SeqFamily* fam = seq_family(c->d.trunk_kind);
  MILAN_REQUIRE(!head || fam == nullptr || c->ahead.installed, MILAN_ERR_STATE, "%s",
                fam->no_head);
  MILAN_REQUIRE(!head || fam != nullptr || c->fc_w != nullptr, MILAN_ERR_STATE,
                "this context was created without fc.weight: it has no classifier head");
  MILAN_REQUIRE(!c->trunk_f16, MILAN_ERR_ARG,
                "classification runs in the f32 and split_f16 modes, not in the fast f16 mode");
  MILAN_REQUIRE(n > 0 && H >= 1 && W >= 1, MILAN_ERR_SHAPE,
                "classify: need n>0 and H,W>=1 (got n=%d H=%d W=%d)", n, H, W);
  if (head && fam != nullptr && fam->head_image != nullptr) {
    // what pool5 has to leave: the Places net's fc6 reads C5 x 6 x 6 features with no adaptive
    // pool in front of it, a VGG's adaptive pool needs a pixel (32 x 32: five 2x2 pools)
    const SeqTrunk t(c, 1, H, W, false, nullptr);
    MILAN_REQUIRE(t.h[0] >= 3 && t.w[0] >= 3 && std::min(t.th, t.tw) >= fam->tail_lo &&
                      std::max(t.th, t.tw) <= fam->tail_hi,
                  MILAN_ERR_SHAPE, fam->head_image, H, W, c->ahead.in[0]);
  }
  bool sp = c->precision == MILAN_PRECISION_SPLIT_F16 && c->d.trunk_width % 8 == 0;
  // (Places: conv3 is dense and reads a multiple of 64 channels; the grouped levels decide for
  // themselves, SeqTrunk::formats)
  if (places_trunk(c)) sp = sp && c->alex[2].ws != nullptr;
  // (AlexNet: conv1 has 3 input channels and stays fp32, as in alexnet_run_batch)
  for (int l = 1; l < 5 && sp && alex_trunk(c); ++l) sp = c->alex[l].ws != nullptr;
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
  vgg_trace_reset(c);
  auto go = seq_trunk(c) ? run<SeqTrunk> : run<ResNetTrunk>;
  return go(c, images, n, H, W, split, logits, predictions, nullptr, 4, "classify", ws, s);
}

int classify_sweep(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                   const int32_t* units, int count, const int64_t* targets, int32_t* correct,
                   int64_t* predictions, Arena& ws, hipStream_t s) {
  bool split;
  MILAN_TRY(classify_checks(c, n, H, W, &split));
  MILAN_TRY(check_units(c, levels, units, count, "milan_classify_sweep"));
  if (count == 0) return 0;
  vgg_trace_reset(c);
  auto go = seq_trunk(c) ? sweep<SeqTrunk> : sweep<ResNetTrunk>;
  return go(c, images, n, H, W, split, levels, units, count, targets, correct, predictions, ws, s);
}

// milan_activations: the walk of classify_run, once per sub-batch up to the highest requested
// level; its scratch is classify_workspace(..., 0)
int activations_run(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                    int count, float* const* outputs, Arena& ws, hipStream_t s) {
  bool split;
  MILAN_TRY(classify_checks(c, n, H, W, &split, false));
  float* taps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int top = -1;
  for (int i = 0; i < count; ++i) {
    MILAN_REQUIRE(levels[i] >= 0 && levels[i] <= 4, MILAN_ERR_ARG,
                  "milan_activations: level %d is not one of 0..4 (%s)", levels[i],
                  level_names(c));
    // (the walk's own question, ahead of the one for an output that such a level leaves empty)
    MILAN_TRY(seq_reach(c, H, W, levels[i]));
    MILAN_REQUIRE(taps[levels[i]] == nullptr, MILAN_ERR_ARG,
                  "milan_activations: level %d is requested twice", levels[i]);
    MILAN_REQUIRE(outputs[i] != nullptr, MILAN_ERR_ARG,
                  "milan_activations: outputs[%d] is null", i);
    taps[levels[i]] = outputs[i];
    top = std::max(top, (int)levels[i]);
  }
  vgg_trace_reset(c);
  auto go = seq_trunk(c) ? run<SeqTrunk> : run<ResNetTrunk>;
  // (SeqFamily::taps_call: the families' messages about the workspace and the sub-batch name
  // the call as they did when each was written)
  return go(c, images, n, H, W, split, nullptr, nullptr, taps, top,
            seq_trunk(c) ? seq_family(c->d.trunk_kind)->taps_call : "activations", ws, s);
}

}  // namespace milan
