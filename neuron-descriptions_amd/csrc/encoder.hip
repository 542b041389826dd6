// Masked-exemplar pyramid encoder: PyramidConvEncoder.forward
// (reference src/milan/encoders.py:286-320) over a torchvision bottleneck
// ResNet trunk (call site encoders.py:274,346-350).
//
// Data layout in HBM: activations are NHWC fp32 (a conv tap = contiguous Cin
// run = one coalesced 16-B chunk per lane for the implicit GEMM); the network
// input is NHWC4 (RGB + a zero lane) so the 7x7 stem is the same kernel with
// Cin = 4.  Eval-mode BatchNorm is folded into the conv weights/bias at
// finalize time, except for the stem whose RAW output is a pyramid tap
// (nethook retains 'conv1' before bn1/relu, src/deps/netdissect/nethook.py:
// 226-235); bn1+relu+maxpool run as one fused kernel.
#include "common.h"
#include <optional>
#include <vector>

#include <cstdio>
#include <cstdlib>

namespace milan {

static constexpr float kBnEps = 1e-5f;  // torchvision 0.12 BatchNorm2d default

// ---------------------------------------------------------------------------
// weight packing (one-time)
// ---------------------------------------------------------------------------
// OIHW conv weight (+ optional eval-BN) -> [Cout][Kp], k = (kh*KW+kw)*CinP + i.
__global__ void pack_conv_kernel(const float* __restrict__ w, int cout, int cin,
                                 int cinp, int kh, int kw, int kp,
                                 const float* __restrict__ gamma,
                                 const float* __restrict__ beta,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ var,
                                 float* __restrict__ wp,
                                 float* __restrict__ bias) {
  const long total = (long)cout * kp;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int o = idx / kp, k = idx - (long)o * kp;
    const int tap = k / cinp, i = k - tap * cinp;
    float v = 0.f;
    if (tap < kh * kw && i < cin) {
      const int y = tap / kw, x = tap - y * kw;
      v = w[(((long)o * cin + i) * kh + y) * kw + x];
      if (gamma) v *= gamma[o] / sqrtf(var[o] + kBnEps);
    }
    wp[idx] = v;
    if (bias && k == 0) {
      const float sc = gamma[o] / sqrtf(var[o] + kBnEps);
      bias[o] = beta[o] - mean[o] * sc;
    }
  }
}

__global__ void bn_affine_kernel(const float* gamma, const float* beta,
                                 const float* mean, const float* var, int c,
                                 float* scale, float* shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c) {
    const float sc = gamma[i] / sqrtf(var[i] + kBnEps);
    scale[i] = sc;
    shift[i] = beta[i] - mean[i] * sc;
  }
}

static const Tensor* find(milan_ctx* c, const std::string& name) {
  auto it = c->raw.find(name);
  return it == c->raw.end() ? nullptr : &it->second;
}

// Slice-major k order of a k x k conv's packed rows: 8-channel groups of `gb` 16-byte pieces
// (2: split format, 1: plain f16) move from [tap][Cin / 8] to [Cin / (8 gps)][tap][gps]:
//   dst[n][(slice * taps + tap) * gps + gi] = src[n][tap * (Cin / 8) + slice * gps + gi]
__global__ void slice_major_kernel(const float* __restrict__ src, int cout, int taps, int cin,
                                   int gps, int gb, float* __restrict__ dst) {
  const int gpt = cin / 8;       // groups per tap
  const int gpr = taps * gpt;    // groups per row
  const long total = (long)cout * gpr;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const long n = idx / gpr;
    const int d = idx - n * gpr;
    const int gi = d % gps, st = d / gps;
    const int slice = st / taps, tap = st - slice * taps;
    const float4* sp = reinterpret_cast<const float4*>(src) +
                       (n * gpr + tap * gpt + slice * gps + gi) * gb;
    float4* dp = reinterpret_cast<float4*>(dst) + idx * gb;
    for (int e = 0; e < gb; ++e) dp[e] = sp[e];
  }
}

int make_slice_major(const float* ws, int cout, int taps, int cin, int gps, int gb, float* dst,
                     hipStream_t s) {
  const long groups = (long)cout * taps * (cin / 8);
  const int blocks = (int)((groups + 255) / 256 < 4096 ? (groups + 255) / 256 : 4096);
  hipLaunchKernelGGL(slice_major_kernel, dim3(blocks), dim3(256), 0, s, ws, cout, taps, cin,
                     gps, gb, dst);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// (the experiments build's LDS-strip kernel: 16-channel chunks of a 3x3 conv)
int make_chunk_major(const float* ws, int cout, int cin, float* dst,
                     hipStream_t s) {
  return make_slice_major(ws, cout, 9, cin, 2, 2, dst, s);
}

__global__ void scale_vec_kernel(const float* __restrict__ a, float m, int n,
                                 float* __restrict__ o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] * m;
}
// copy of a folded per-channel vector in the split trunk's activation scale
// (milan_ctx::act_scale, an exact power of two: the products are exact)
static int scaled_copy(milan_ctx* c, const float* src, int n, float** dst, hipStream_t s) {
  if (!src) { *dst = nullptr; return 0; }
  MILAN_TRY(dev_alloc(c, (void**)dst, sizeof(float) * n));
  hipLaunchKernelGGL(scale_vec_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src,
                     c->act_scale, n, *dst);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// fast mode: split rows [groups of (hi x8 | lo x8)] -> plain f16 rows (the hi halves);
// `groups` 32-byte groups in, 16 bytes out each
__global__ void split_hi_to_f16_kernel(const float* __restrict__ src, long groups,
                                       float* __restrict__ dst) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < groups;
       q += (long)gridDim.x * blockDim.x)
    *reinterpret_cast<v4*>(dst + q * 4) = *reinterpret_cast<const v4*>(src + q * 8);
}
static int make_f16_weight(milan_ctx* c, ConvW* w, hipStream_t s) {
  w->wf = nullptr;
  if (!w->ws || w->cin % 64 != 0 || w->Kp % 64 != 0 || w->K != w->Kp) return 0;
  const long groups = (long)w->cout * w->Kp / 8;
  MILAN_TRY(dev_alloc(c, (void**)&w->wf, sizeof(float) * (size_t)groups * 4));
  const int blocks = (int)((groups + 255) / 256 < 4096 ? (groups + 255) / 256 : 4096);
  hipLaunchKernelGGL(split_hi_to_f16_kernel, dim3(blocks), dim3(256), 0, s, w->ws, groups, w->wf);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int pack_conv(milan_ctx* c, const std::string& conv,
                     const std::string& bn, int stride, int pad, ConvW* out,
                     hipStream_t s, bool split_without_bn = false, int groups = 1) {
  const Tensor* w = find(c, conv + ".weight");
  MILAN_REQUIRE(w && w->shape.size() == 4, MILAN_ERR_STATE,
                "missing conv weight %s.weight", conv.c_str());
  const float *g = nullptr, *b = nullptr, *m = nullptr, *v = nullptr;
  if (!bn.empty()) {
    const Tensor *tg = find(c, bn + ".weight"), *tb = find(c, bn + ".bias"),
                 *tm = find(c, bn + ".running_mean"),
                 *tv = find(c, bn + ".running_var");
    MILAN_REQUIRE(tg && tb && tm && tv, MILAN_ERR_STATE,
                  "missing batchnorm tensors %s.*", bn.c_str());
    MILAN_REQUIRE(tg->numel() == w->shape[0], MILAN_ERR_SHAPE,
                  "%s channels != %s out channels", bn.c_str(), conv.c_str());
    g = tg->dev; b = tb->dev; m = tm->dev; v = tv->dev;
  }
  // A grouped conv's weight is (cout, cin / groups, kh, kw): its rows are packed exactly like
  // a dense conv's of cin / groups channels -- K and Kp per group, the groups' rows back to
  // back -- and so are the split and slice-major copies below (ConvW::groups)
  MILAN_REQUIRE(groups >= 1 && w->shape[0] % groups == 0 &&
                    (groups == 1 || w->shape[1] % 4 == 0),
                MILAN_ERR_SHAPE, "%s.weight: %ld x %ld channels do not split into %d groups of "
                "a multiple of 4 input channels", conv.c_str(), (long)w->shape[0],
                (long)w->shape[1], groups);
  out->groups = groups;
  out->cout = (int)w->shape[0];
  out->cin = ((int)w->shape[1] + 3) / 4 * 4;
  out->cin_real = (int)w->shape[1];
  out->kh = (int)w->shape[2];
  out->kw = (int)w->shape[3];
  out->stride = stride;
  out->pad = pad;
  out->K = out->kh * out->kw * out->cin;
  out->Kp = (out->K + 31) / 32 * 32;
  MILAN_TRY(dev_alloc(c, (void**)&out->w,
                      sizeof(float) * (size_t)out->cout * out->Kp));
  if (g) MILAN_TRY(dev_alloc(c, (void**)&out->bias, sizeof(float) * out->cout));
  const long total = (long)out->cout * out->Kp;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_conv_kernel, dim3(blocks), dim3(256), 0, s, w->dev,
                     out->cout, (int)w->shape[1], out->cin, out->kh, out->kw,
                     out->Kp, g, b, m, v, out->w, out->bias);
  MILAN_CHECK_HIP(hipGetLastError());
  if (!g) {
    // a conv with its own bias and no BatchNorm (AlexNet)
    if (const Tensor* tb = find(c, conv + ".bias")) {
      MILAN_REQUIRE(tb->numel() == out->cout, MILAN_ERR_SHAPE,
                    "%s.bias has %ld entries for %d channels", conv.c_str(),
                    (long)tb->numel(), out->cout);
      MILAN_TRY(dev_alloc(c, (void**)&out->bias, sizeof(float) * out->cout));
      MILAN_CHECK_HIP(hipMemcpyAsync(out->bias, tb->dev,
                                     sizeof(float) * out->cout,
                                     hipMemcpyDeviceToDevice, s));
    }
  }
  if ((g || split_without_bn) && out->cin % 32 == 0) {  // split-f16 copy
    MILAN_TRY(make_split_weight(c, out->w, out->cout, out->Kp, &out->ws,
                                &out->ws_inv, s));
    if (out->ws) MILAN_TRY(scaled_copy(c, out->bias, out->cout, &out->bias_s, s));
    MILAN_TRY(make_f16_weight(c, out, s));
    if (out->ws && out->kh * out->kw > 1 && out->kh * out->kw <= 32 && out->Kp == out->K) {
      // (32-channel slice, tap, channel) order for the ping-pong kernel (GemmArgs::Wt)
      const int taps = out->kh * out->kw;
      MILAN_TRY(dev_alloc(c, (void**)&out->wst, sizeof(float) * (size_t)out->cout * out->Kp));
      MILAN_TRY(make_slice_major(out->ws, out->cout, taps, out->cin, 4, 2, out->wst, s));
      // (slice_major_kernel assumes whole slices: cin % 32 for split rows -- guaranteed by
      // the enclosing test -- and cin % 64 for the plain f16 rows)
      if (out->wf && out->cin % 64 == 0) {
        MILAN_TRY(dev_alloc(c, (void**)&out->wft, sizeof(float) * (size_t)out->cout * out->Kp / 2));
        MILAN_TRY(make_slice_major(out->wf, out->cout, taps, out->cin, 8, 1, out->wft, s));
      }
    }
#if MILAN_EXPERIMENTS
    if (out->ws && out->kh == 3 && out->kw == 3 && out->Kp == out->K &&
        out->cin % 16 == 0) {
      // chunk-major copy for the LDS-strip 3x3 kernel and MILAN_TAPS_INNER: 32-byte groups
      // of 8 channels move from [tap][Cin/8] to [Cin/16][tap][2]
      MILAN_TRY(dev_alloc(c, (void**)&out->ws3,
                          sizeof(float) * (size_t)out->cout * out->Kp));
      MILAN_TRY(make_chunk_major(out->ws, out->cout, out->cin, out->ws3, s));
    }
#endif
  }
  return 0;
}

// [c3 | downsample] along K: out = relu(W3 t2 + Wd x_s + (b3 + bd)), one GEMM
// instead of two plus a round trip of the downsample output through HBM.
__global__ void concat_k_kernel(const float* __restrict__ a, int ka,
                                const float* __restrict__ b, int kb, int n,
                                float* __restrict__ out) {
  const int kt = ka + kb;
  const long total = (long)n * kt;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int r = idx / kt, col = idx - (long)r * kt;
    out[idx] = col < ka ? a[(long)r * ka + col] : b[(long)r * kb + (col - ka)];
  }
}
__global__ void add2_kernel(const float* a, const float* b, int n, float* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) o[i] = a[i] + b[i];
}

static int fuse_c3_down(milan_ctx* c, Bottleneck* b, hipStream_t s) {
  const ConvW &c3 = b->c3, &dn = b->down;
  if (c3.K != c3.Kp || dn.K != dn.Kp || c3.K % 32 || dn.K % 32 ||
      c3.cout != dn.cout || !c3.ws || !dn.ws)
    return 0;  // shapes the fused path does not cover: keep them separate
  ConvW f;
  f.cout = c3.cout; f.cin = c3.cin; f.cin_real = c3.cin_real;
  f.kh = f.kw = 1; f.stride = 1; f.pad = 0;
  f.K = f.Kp = c3.K + dn.K;
  MILAN_TRY(dev_alloc(c, (void**)&f.w, sizeof(float) * (size_t)f.cout * f.Kp));
  MILAN_TRY(dev_alloc(c, (void**)&f.bias, sizeof(float) * f.cout));
  const long total = (long)f.cout * f.Kp;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(concat_k_kernel, dim3(blocks), dim3(256), 0, s, c3.w, c3.K,
                     dn.w, dn.K, f.cout, f.w);
  hipLaunchKernelGGL(add2_kernel, dim3((f.cout + 255) / 256), dim3(256), 0, s,
                     c3.bias, dn.bias, f.cout, f.bias);
  MILAN_CHECK_HIP(hipGetLastError());
  MILAN_TRY(make_split_weight(c, f.w, f.cout, f.Kp, &f.ws, &f.ws_inv, s));
  MILAN_TRY(scaled_copy(c, f.bias, f.cout, &f.bias_s, s));
  MILAN_TRY(make_f16_weight(c, &f, s));
  b->c3d = f;
  return 0;
}

int pack_conv_plain(const float* w_oihw, int cout, int cin, int kh, int kw,
                    float* wp, hipStream_t s) {
  const int cinp = (cin + 3) / 4 * 4;
  const int kp = (kh * kw * cinp + 31) / 32 * 32;
  const long total = (long)cout * kp;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_conv_kernel, dim3(blocks), dim3(256), 0, s, w_oihw,
                     cout, cin, cinp, kh, kw, kp, nullptr, nullptr, nullptr,
                     nullptr, wp, nullptr);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Pixel-pair stem (split-f16 mode).  A 3-channel pixel would waste 5 of the 8
// slots of a split-format group, so a group holds TWO horizontally adjacent
// pixels (x = 2p-1, 2p; RGB0 RGB0).  With stride 2 / pad 3 the 7 taps of one
// kernel row of output column wo are exactly groups wo-1 .. wo+2 (the 8th tap
// has zero weight): the 7x7/2 stem becomes a KH=7 x KW=4 convolution over
// groups with horizontal stride 1 / pad 1, K = 7*4*8 = 224 slots instead of
// the 392 a Cin=8 padding would need.  Weights: k = (kh*4 + j)*8 + e with tap
// t = 2j + e/4, channel e%4.
__global__ void pack_stem_pairs_kernel(const float* __restrict__ w, int cout,
                                       float* __restrict__ wp) {
  const int total = cout * 224;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += gridDim.x * blockDim.x) {
    const int o = idx / 224, k = idx - o * 224;
    const int e = k & 7, j = (k >> 3) & 3, kh = k >> 5;
    const int t = 2 * j + (e >> 2), ch = e & 3;
    wp[idx] = (t < 7 && ch < 3) ? w[((o * 3 + ch) * 7 + kh) * 7 + t] : 0.f;
  }
}

static int pack_stem_pairs(milan_ctx* c, const Tensor* w, hipStream_t s) {
  ConvW& f = c->stem_pair;
  f = ConvW();
  if (w->shape[1] != 3 || w->shape[2] != 7 || w->shape[3] != 7 ||
      w->shape[0] > 64 || w->shape[0] % 8)
    return 0;  // not the torchvision stem: split mode keeps the fp32 stem
  f.cout = (int)w->shape[0];
  f.cin = 8; f.cin_real = 3; f.kh = 7; f.kw = 4; f.stride = 2; f.pad = 3;
  f.K = f.Kp = 224;
  MILAN_TRY(dev_alloc(c, (void**)&f.w, sizeof(float) * (size_t)f.cout * f.Kp));
  hipLaunchKernelGGL(pack_stem_pairs_kernel, dim3((f.cout * 224 + 255) / 256),
                     dim3(256), 0, s, w->dev, f.cout, f.w);
  MILAN_CHECK_HIP(hipGetLastError());
  return make_split_weight(c, f.w, f.cout, f.Kp, &f.ws, &f.ws_inv, s);
}

int encoder_finalize(milan_ctx* c, hipStream_t s) {
  const std::string p = "encoder.encoder.model.";
  const int kind = c->d.trunk_kind;
  if (kind == MILAN_TRUNK_NONE) return 0;  // decoder-only context
  if (kind == MILAN_TRUNK_ALEXNET || kind == MILAN_TRUNK_ALEXNET_PLACES) {
    // torchvision's AlexNet.features, or the Places365 AlexNet: conv1 unpadded,
    // conv2 / conv4 / conv5 in two groups unless the weights say otherwise
    // (split_groups=False: dense weights, groups of 1)
    const AlexSpec& spec = alex_spec(kind);
    if (!find(c, p + spec.key[0] + ".weight")) return 0;  // decoder-only context
    MILAN_REQUIRE(!spec.width8 || c->d.trunk_width % 8 == 0, MILAN_ERR_SHAPE,
                  "the Places365 AlexNet needs a width that is a multiple of 8 (got %d)",
                  c->d.trunk_width);
    int cin_full = 3;
    for (int i = 0; i < 5; ++i) {
      const std::string name = p + spec.key[i];
      int groups = 1;
      if (spec.weight_groups) {
        const Tensor* w = find(c, name + ".weight");
        MILAN_REQUIRE(w && w->shape.size() == 4 && w->shape[1] >= 1 &&
                          cin_full % (int)w->shape[1] == 0,
                      MILAN_ERR_SHAPE, "%s.weight is missing or does not divide %d input "
                      "channels into groups", spec.key[i], cin_full);
        groups = cin_full / (int)w->shape[1];
      }
      MILAN_TRY(pack_conv(c, name, "", spec.stride[i], spec.pad[i], &c->alex[i], s, i > 0,
                          groups));
      MILAN_REQUIRE(c->alex[i].cout == spec.mult[i] * c->d.trunk_width &&
                        c->alex[i].bias != nullptr,
                    MILAN_ERR_SHAPE, "%s: %d channels, expected %d (with a bias)", spec.key[i],
                    c->alex[i].cout, spec.mult[i] * c->d.trunk_width);
      cin_full = c->alex[i].cout;
    }
    c->stem = c->alex[0];  // "encoder weights present" marker
  } else if (kind == MILAN_TRUNK_VGG) {
    // torchvision's VGG without batch norm: the blocks follow from the keys
    // `vgg.B.J` -- B = 1..5, J contiguous from 0, at most four convs per block
    if (!find(c, p + "vgg.1.0.weight")) return 0;  // decoder-only context
    const int wd = c->d.trunk_width;
    MILAN_REQUIRE(wd % 8 == 0, MILAN_ERR_SHAPE,
                  "the VGG trunk needs a width that is a multiple of 8 (got %d)", wd);
    const size_t plen = p.size() + 4;  // "<prefix>vgg."
    for (const auto& kv : c->raw) {
      const std::string& key = kv.first;
      if (key.compare(0, plen, p + "vgg.") != 0) continue;
      int b = 0, j = 0, used = 0;
      const bool ok = sscanf(key.c_str() + plen, "%d.%d.%n", &b, &j, &used) == 2 && used > 0 &&
                      (key.compare(plen + used, std::string::npos, "weight") == 0 ||
                       key.compare(plen + used, std::string::npos, "bias") == 0);
      MILAN_REQUIRE(ok && b >= 1 && b <= 5 && j >= 0 && j <= 3, MILAN_ERR_SHAPE,
                    "%s is not a VGG key: vgg.B.J.weight / .bias with B in 1..5 and J in 0..3",
                    key.c_str() + p.size());
      // (a gap in J: the conv in front of this one has to be there)
      MILAN_REQUIRE(j == 0 || find(c, p + "vgg." + std::to_string(b) + "." +
                                          std::to_string(j - 1) + ".weight"),
                    MILAN_ERR_SHAPE, "VGG block %d has conv %d but no conv %d: the convs of a "
                    "block are numbered from 0 without a gap", b, j, j - 1);
    }
    int cin = 3;
    for (int b = 0; b < 5; ++b) {
      const int cout = wd * (b < 3 ? 1 << b : 8);
      c->vgg_n[b] = 0;
      for (int j = 0; j < 4; ++j) {
        const std::string name = p + "vgg." + std::to_string(b + 1) + "." + std::to_string(j);
        const Tensor* w = find(c, name + ".weight");
        if (!w) break;
        MILAN_REQUIRE(w->shape.size() == 4 && w->shape[0] == cout && w->shape[1] == cin &&
                          w->shape[2] == 3 && w->shape[3] == 3 && find(c, name + ".bias"),
                      MILAN_ERR_SHAPE,
                      "vgg.%d.%d: expected a (%d, %d, 3, 3) weight with a bias (block %d has "
                      "%d x min(2^%d, 8) channels)", b + 1, j, cout, cin, b + 1, wd, b);
        ConvW& cw = c->vgg[b][j];
        MILAN_TRY(pack_conv(c, name, "", 1, 1, &cw, s, true));
        MILAN_REQUIRE(cw.bias != nullptr, MILAN_ERR_SHAPE, "vgg.%d.%d.bias has the wrong size",
                      b + 1, j);
        cin = cout;
        c->vgg_n[b] = j + 1;
      }
      MILAN_REQUIRE(c->vgg_n[b] >= 1, MILAN_ERR_SHAPE, "VGG block %d has no conv (vgg.%d.0.weight)",
                    b + 1, b + 1);
    }
    MILAN_TRY(dev_alloc(c, (void**)&c->vgg_w27, sizeof(float) * 27 * (size_t)wd));
    MILAN_TRY(vgg_pack_first(find(c, p + "vgg.1.0.weight")->dev, wd, c->vgg_w27, s));
    c->stem = c->vgg[0][0];  // "encoder weights present" marker
  } else {
  if (!find(c, p + "conv1.weight")) return 0;  // decoder-only context
  MILAN_TRY(pack_conv(c, p + "conv1", "", 2, 3, &c->stem, s));
  MILAN_REQUIRE(c->stem.cout == c->d.trunk_width, MILAN_ERR_SHAPE,
                "stem width %d != dims.trunk_width %d", c->stem.cout,
                c->d.trunk_width);
  MILAN_TRY(pack_stem_pairs(c, find(c, p + "conv1.weight"), s));
  {
    const Tensor *tg = find(c, p + "bn1.weight"), *tb = find(c, p + "bn1.bias"),
                 *tm = find(c, p + "bn1.running_mean"),
                 *tv = find(c, p + "bn1.running_var");
    MILAN_REQUIRE(tg && tb && tm && tv, MILAN_ERR_STATE, "missing bn1.*");
    const int w = c->stem.cout;
    MILAN_TRY(dev_alloc(c, (void**)&c->bn1_scale, sizeof(float) * w));
    MILAN_TRY(dev_alloc(c, (void**)&c->bn1_shift, sizeof(float) * w));
    hipLaunchKernelGGL(bn_affine_kernel, dim3((w + 255) / 256), dim3(256), 0, s,
                       tg->dev, tb->dev, tm->dev, tv->dev, w, c->bn1_scale,
                       c->bn1_shift);
    MILAN_TRY(scaled_copy(c, c->bn1_scale, w, &c->bn1_scale_s, s));
    MILAN_TRY(scaled_copy(c, c->bn1_shift, w, &c->bn1_shift_s, s));
  }
  const bool basic = kind == MILAN_TRUNK_BASIC;
  for (int li = 0; li < 4; ++li) {
    c->blocks[li].clear();
    for (int bi = 0; bi < c->d.trunk_blocks[li]; ++bi) {
      Bottleneck b;
      b.basic = basic;
      const std::string q =
          p + "layer" + std::to_string(li + 1) + "." + std::to_string(bi) + ".";
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      MILAN_REQUIRE((find(c, q + "conv3.weight") != nullptr) == !basic,
                    MILAN_ERR_STATE,
                    "%s does not look like a %s block (dims.trunk_kind = %d)",
                    q.c_str(), basic ? "basic" : "bottleneck", kind);
      if (basic) {
        // BasicBlock: 3x3 (carries the stride) -> 3x3, expansion 1
        MILAN_TRY(pack_conv(c, q + "conv1", q + "bn1", stride, 1, &b.c1, s));
        MILAN_TRY(pack_conv(c, q + "conv2", q + "bn2", 1, 1, &b.c2, s));
      } else {
        MILAN_TRY(pack_conv(c, q + "conv1", q + "bn1", 1, 0, &b.c1, s));
        MILAN_TRY(pack_conv(c, q + "conv2", q + "bn2", stride, 1, &b.c2, s));
        MILAN_TRY(pack_conv(c, q + "conv3", q + "bn3", 1, 0, &b.c3, s));
      }
      b.has_down = find(c, q + "downsample.0.weight") != nullptr;
      // torchvision adds a downsample wherever the block changes the shape
      MILAN_REQUIRE(b.has_down == (bi == 0 && (!basic || li > 0)),
                    MILAN_ERR_STATE, "unexpected downsample layout at %s",
                    q.c_str());
      if (b.has_down) {
        MILAN_TRY(pack_conv(c, q + "downsample.0", q + "downsample.1", stride,
                            0, &b.down, s));
        if (!basic) MILAN_TRY(fuse_c3_down(c, &b, s));
      }
      c->blocks[li].push_back(b);
    }
  }
  }
  if (const Tensor* t = find(c, "encoder.mean")) {
    MILAN_CHECK_HIP(hipMemcpyAsync(c->mean, t->dev, 3 * sizeof(float),
                                   hipMemcpyDeviceToHost, s));
  }
  if (const Tensor* t = find(c, "encoder.std")) {
    MILAN_CHECK_HIP(hipMemcpyAsync(c->stdv, t->dev, 3 * sizeof(float),
                                   hipMemcpyDeviceToHost, s));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// input conversion: NCHW u8/f32 -> normalised NHWC4 f32
// ---------------------------------------------------------------------------
// x = float(u8) * float32(1/255)  (src/milannotations/datasets.py:191-197 via
// renormalize.py:119-136: a multiply, not a divide), then (x - mean) / std
// (src/milan/encoders.py:295).
template <typename T>
__global__ void preprocess_kernel(const T* __restrict__ img, long n_pix_total,
                                  int hw, float m0, float m1, float m2,
                                  float s0, float s1, float s2,
                                  float4* __restrict__ out,
                                  const void* __restrict__ mul = nullptr,
                                  int mul_u8 = 1, int* __restrict__ poison = nullptr,
                                  unsigned* __restrict__ status = nullptr,
                                  const int* __restrict__ order = nullptr,
                                  const int* __restrict__ live = nullptr) {
  // the byte->float product is rounded on its own, as in the reference: no
  // contraction into the mean subtraction
#pragma clang fp contract(off)
  const float inv255 = (float)(1.0 / 255.0);
  if (live) n_pix_total = min(n_pix_total, (long)*live * hw);   // (image count on the device)
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < n_pix_total;
       p += (long)gridDim.x * blockDim.x) {
    const long n = p / hw, r = p - n * hw;
    const T* base = img + (order ? (long)order[n] : n) * 3 * hw + r;
    float v0, v1, v2;
    if constexpr (sizeof(T) == 1) {
      v0 = (float)base[0] * inv255;
      v1 = (float)base[hw] * inv255;
      v2 = (float)base[2 * (long)hw] * inv255;
    } else {
      v0 = base[0]; v1 = base[hw]; v2 = base[2 * (long)hw];
    }
    // SpatialConvEncoder (encoders.py:204-208): normalise, THEN mask
    const float k = mul == nullptr ? 1.f
                    : mul_u8     ? (float)((const uint8_t*)mul)[p]
                                 : ((const float*)mul)[p];
    const float o0 = ((v0 - m0) / s0) * k, o1 = ((v1 - m1) / s1) * k, o2 = ((v2 - m2) / s2) * k;
    if constexpr (sizeof(T) != 1) {
      // a pixel that is not finite poisons its image: the reference's pyramid pools
      // NaN x mask over every level (pinned by tests/test_gpu_status.py against the oracle)
      if (poison != nullptr && !(fabsf(o0) + fabsf(o1) + fabsf(o2) < INFINITY)) {
        poison[n] = 1;
        if (status) atomicOr(status, 2u /* MILAN_STATUS_NONFINITE_INPUT */);
      }
    }
    out[p] = make_float4(o0, o1, o2, 0.f);
  }
}

// ---------------------------------------------------------------------------
// stem tail: y = maxpool3x3/2,pad1( relu( x*scale + shift ) ), NHWC
// ---------------------------------------------------------------------------
__global__ void bn_relu_maxpool_kernel(const float4* __restrict__ x, int n,
                                       int H, int W, int C4, int Ho, int Wo,
                                       const float4* __restrict__ scale,
                                       const float4* __restrict__ shift,
                                       float4* __restrict__ y,
                                       const int* __restrict__ live = nullptr) {
  if (live) n = min(n, *live);   // (image count on the device)
  const long total = (long)n * Ho * Wo * C4;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c = idx % C4;
    long t = idx / C4;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const long img = t / Ho;
    const float4 sc = scale[c], sh = shift[c];
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = 0; dy < 3; ++dy) {
      const int hi = ho * 2 - 1 + dy;
      if (hi < 0 || hi >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int wi = wo * 2 - 1 + dx;
        if (wi < 0 || wi >= W) continue;
        const float4 v = x[((img * H + hi) * W + wi) * C4 + c];
        best.x = fmaxf(best.x, fmaxf(v.x * sc.x + sh.x, 0.f));
        best.y = fmaxf(best.y, fmaxf(v.y * sc.y + sh.y, 0.f));
        best.z = fmaxf(best.z, fmaxf(v.z * sc.z + sh.z, 0.f));
        best.w = fmaxf(best.w, fmaxf(v.w * sc.w + sh.w, 0.f));
      }
    }
    y[idx] = best;
  }
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

__device__ inline void enc_split8(const float* v, f32x4_t* hi_out, f32x4_t* lo_out,
                                  float* sat = nullptr) {
  split8_rne(v, hi_out, lo_out, sat);  // common.h
}

// split-format groups [hi x8 | lo x8] -> 8 fp32 values each
__global__ void split_to_f32_kernel(const float* __restrict__ x, long groups,
                                    float* __restrict__ y, float mul) {
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < groups;
       q += (long)gridDim.x * blockDim.x) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(x + q * 8);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(x + q * 8 + 4);
    const f16x8_t hh = __builtin_bit_cast(f16x8_t, a);
    const f16x8_t ll = __builtin_bit_cast(f16x8_t, b);
    f32x4_t o0, o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = ((float)hh[e] + (float)ll[e]) * mul;
      o1[e] = ((float)hh[4 + e] + (float)ll[4 + e]) * mul;
    }
    *reinterpret_cast<f32x4_t*>(y + q * 8) = o0;
    *reinterpret_cast<f32x4_t*>(y + q * 8 + 4) = o1;
  }
}

// split-format groups -> plain f16 (fast mode, at the layer2 -> layer3 boundary):
// f16(hi + lo), one rounding of the 22-bit value
__global__ void split_to_f16_kernel(const float* __restrict__ x, long groups,
                                    float* __restrict__ y,
                                    const int* __restrict__ live = nullptr,
                                    long groups_per_image = 0) {
  if (live) groups = min(groups, (long)*live * groups_per_image);   // (image count on the device)
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < groups;
       q += (long)gridDim.x * blockDim.x) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(x + q * 8);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(x + q * 8 + 4);
    const f16x8_t hh = __builtin_bit_cast(f16x8_t, a);
    const f16x8_t ll = __builtin_bit_cast(f16x8_t, b);
    f16x8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)((float)hh[e] + (float)ll[e]);
    *reinterpret_cast<f32x4_t*>(y + q * 4) = __builtin_bit_cast(f32x4_t, o);
  }
}

// NCHW u8/f32 -> normalised pixel-pair groups in split-f16 format:
// out[img][y][p] = split8(RGB0 of x=2p-1, RGB0 of x=2p), p in [0, G), zeros
// outside the image (see pack_stem_pairs_kernel).
template <typename T>
__global__ void preprocess_pairs_kernel(const T* __restrict__ img, long n_groups,
                                        int H, int W, int G, float m0, float m1,
                                        float m2, float s0, float s1, float s2,
                                        float* __restrict__ out,
                                        const void* __restrict__ mul = nullptr,
                                        int mul_u8 = 1, int* __restrict__ poison = nullptr,
                                        unsigned* __restrict__ status = nullptr,
                                        const int* __restrict__ order = nullptr,
                                        const int* __restrict__ live = nullptr) {
#pragma clang fp contract(off)  // see preprocess_kernel
  const float inv255 = (float)(1.0 / 255.0);
  const long hw = (long)H * W;
  float sat = 0.f;
  if (live) n_groups = min(n_groups, (long)*live * H * G);   // (image count on the device)
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n_groups;
       q += (long)gridDim.x * blockDim.x) {
    const int p = q % G;
    const long row = q / G;            // img * H + y
    const long n = row / H;
    const int y = row - n * H;
    // (`order`: batch slot n holds image order[n]; never together with `mul` / `poison`)
    const T* base = img + (order ? (long)order[n] : n) * 3 * hw + (long)y * W;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int x = 2 * p - 1 + h;
      float a = 0.f, b = 0.f, cc = 0.f;
      if (x >= 0 && x < W) {
        if constexpr (sizeof(T) == 1) {
          a = (float)base[x] * inv255;
          b = (float)base[hw + x] * inv255;
          cc = (float)base[2 * hw + x] * inv255;
        } else {
          a = base[x]; b = base[hw + x]; cc = base[2 * hw + x];
        }
        const long mp = n * hw + (long)y * W + x;
        const float k = mul == nullptr ? 1.f
                        : mul_u8     ? (float)((const uint8_t*)mul)[mp]
                                     : ((const float*)mul)[mp];
        a = ((a - m0) / s0) * k; b = ((b - m1) / s1) * k;
        cc = ((cc - m2) / s2) * k;
      }
      v[4 * h] = a; v[4 * h + 1] = b; v[4 * h + 2] = cc; v[4 * h + 3] = 0.f;
    }
    if constexpr (sizeof(T) != 1) {
      if (poison != nullptr &&
          !(fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]) + fabsf(v[4]) + fabsf(v[5]) + fabsf(v[6]) < INFINITY)) {
        poison[n] = 1;  // (see preprocess_kernel)
        if (status) atomicOr(status, 2u /* MILAN_STATUS_NONFINITE_INPUT */);
      }
    }
    f32x4_t hi, lo;
    enc_split8(v, &hi, &lo, &sat);
    f32x4_t* o = reinterpret_cast<f32x4_t*>(out + q * 8);
    o[0] = hi;
    o[1] = lo;
  }
  report_saturation(status, sat);
}

// The table of the uint8 stem (stem.hip, StemArgs::lut): entry c * 256 + v = the split value
// (hi | lo << 16) preprocess_pairs_kernel<uint8_t> writes for byte v in channel c -- the same
// operations, value by value -- and entry 768 = 0 for the zero padding.  96 threads x 8 values.
__global__ void stem_lut_kernel(float m0, float m1, float m2, float s0, float s1, float s2,
                                unsigned* __restrict__ lut) {
#pragma clang fp contract(off)  // see preprocess_kernel
  const float inv255 = (float)(1.0 / 255.0);
  const int t = threadIdx.x;
  if (t >= 96) { if (t == 96) lut[768] = 0u; return; }
  const int ch = t >> 5, v0 = (t & 31) * 8;
  const float m = ch == 0 ? m0 : (ch == 1 ? m1 : m2), sd = ch == 0 ? s0 : (ch == 1 ? s1 : s2);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (((float)(v0 + e) * inv255) - m) / sd;
  f32x4_t hi, lo;
  enc_split8(v, &hi, &lo);
  const unsigned short* h = reinterpret_cast<const unsigned short*>(&hi);
  const unsigned short* l = reinterpret_cast<const unsigned short*>(&lo);
#pragma unroll
  for (int e = 0; e < 8; ++e) lut[ch * 256 + v0 + e] = (unsigned)h[e] | ((unsigned)l[e] << 16);
}

// Same, 8 channels per thread, output in split-f16 format (gemm.hip).
__global__ void bn_relu_maxpool_split_kernel(const float* __restrict__ x, int n,
                                             int H, int W, int C, int Ho, int Wo,
                                             const float* __restrict__ scale,
                                             const float* __restrict__ shift,
                                             float* __restrict__ y,
                                             unsigned* __restrict__ status,
                                             const int* __restrict__ live = nullptr) {
  const int C8 = C >> 3;
  if (live) n = min(n, *live);   // (image count on the device)
  const long total = (long)n * Ho * Wo * C8;
  float sat = 0.f;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c8 = idx % C8;
    long t = idx / C8;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const long img = t / Ho;
    float sc[8], sh[8], best[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sc[e] = scale[c8 * 8 + e];
      sh[e] = shift[c8 * 8 + e];
      best[e] = -INFINITY;
    }
    for (int dy = 0; dy < 3; ++dy) {
      const int hi = ho * 2 - 1 + dy;
      if (hi < 0 || hi >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int wi = wo * 2 - 1 + dx;
        if (wi < 0 || wi >= W) continue;
        const float* p = x + ((img * H + hi) * W + wi) * C + c8 * 8;
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          best[e] = fmaxf(best[e], fmaxf(a[e] * sc[e] + sh[e], 0.f));
          best[4 + e] = fmaxf(best[4 + e], fmaxf(b[e] * sc[4 + e] + sh[4 + e], 0.f));
        }
      }
    }
    f32x4_t hi4, lo4;
    enc_split8(best, &hi4, &lo4, &sat);
    float* d = y + idx * 8;
    *reinterpret_cast<f32x4_t*>(d) = hi4;
    *reinterpret_cast<f32x4_t*>(d + 4) = lo4;
  }
  report_saturation(status, sat);
}

// ---------------------------------------------------------------------------
// mask pyramid: bilinear resize (align_corners=False) + normalise + compact
// ---------------------------------------------------------------------------
// src/milan/encoders.py:303-314.  One workgroup per (image, level).  Output:
// an ORDERED list of (pixel, weight) for the non-zero weights plus its length,
// so the pooling kernel touches only feature pixels under the mask.  (Levels: enc_plan.h)

template <typename T>
__global__ __launch_bounds__(256) void mask_pyramid_kernel(
    const T* __restrict__ masks, int H, int W, Levels lv,
    int* __restrict__ list_idx, float* __restrict__ list_w,
    int* __restrict__ list_n, int* __restrict__ bbox = nullptr) {
  // every product/sum below is rounded as written (ATen's scalar formula), the same for the
  // uint8 and float instantiations -- except the source coordinate, which torch rounds ONCE
  // (its builds contract scale * (dst + 0.5) - 0.5 into a fused multiply-add): the explicit
  // fmaf below.  Rounded twice it is one ulp of the coordinate off at 48 of the halvings of
  // 1..240 (up to 7.6e-6 in a resized weight at 131 -> 66), at none with a power-of-two scale
  // (tests/test_trunk_ref_host.py restates both forms against F.interpolate).
#pragma clang fp contract(off)
  __shared__ float red_sum[4], red_max[4];
  const int img = blockIdx.x, l = blockIdx.y;
  const int h = lv.h[l], w = lv.w[l], P = h * w;
  const float sy = (float)H / (float)h, sx = (float)W / (float)w;
  const T* m = masks ? masks + (long)img * H * W : nullptr;
  // resized mask value of level pixel p (recomputed, not stored: any image
  // size works and the kernel needs no per-level LDS array)
  auto weight = [&](int p) -> float {
    if (m == nullptr) return 1.f;  // encoders.py:292-293: no masks == all ones
    const int oy = p / w, ox = p - oy * w;
    // ATen upsample_bilinear2d, align_corners=false
    float fy = fmaf((float)oy + 0.5f, sy, -0.5f); fy = fy < 0.f ? 0.f : fy;
    float fx = fmaf((float)ox + 0.5f, sx, -0.5f); fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, ly0 = 1.f - ly1;
    const float lx1 = fx - (float)x0, lx0 = 1.f - lx1;
    const float v00 = (float)m[y0 * W + x0], v01 = (float)m[y0 * W + x1];
    const float v10 = (float)m[y1 * W + x0], v11 = (float)m[y1 * W + x1];
    return ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
  };
  float lsum = 0.f, lmax = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) {
    const float v = weight(p);
    lsum += v;
    lmax = fmaxf(lmax, fabsf(v));
  }
  for (int o = 32; o > 0; o >>= 1) {
    lsum += __shfl_down(lsum, o);
    lmax = fmaxf(lmax, __shfl_down(lmax, o));
  }
  if ((threadIdx.x & 63) == 0) {
    red_sum[threadIdx.x >> 6] = lsum;
    red_max[threadIdx.x >> 6] = lmax;
  }
  __syncthreads();
  const float total = (red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]);
  const float amax = fmaxf(fmaxf(red_max[0], red_max[1]),
                           fmaxf(red_max[2], red_max[3]));
  // valid = not all isclose(ms, 0) (atol 1e-8): only then normalise.
  const bool valid = amax > 1e-8f;
  // ordered compaction by wave 0
  if (threadIdx.x < 64) {
    const long base = (long)img * lv.per_image + lv.off[l];
    int count = 0;
    // level 0 only: bounding box (rows y0..y1, columns x0..x1) of the listed pixels,
    // i.e. of everything the pooling of the raw conv1 tensor reads (stem.hip)
    int by0 = 0x7fffffff, by1 = -1, bx0 = 0x7fffffff, bx1 = -1;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int p = p0 + threadIdx.x;
      float v = p < P ? weight(p) : 0.f;
      if (valid) v = v / total;
      const bool nz = (p < P) && (v != 0.f);
      if (nz && l == 0) {
        const int oy = p / w, ox = p - oy * w;
        by0 = min(by0, oy); by1 = max(by1, oy);
        bx0 = min(bx0, ox); bx1 = max(bx1, ox);
      }
      const unsigned long long mask = __ballot(nz);
      const int pos =
          count + __popcll(mask & ((1ull << threadIdx.x) - 1ull));
      if (nz) {
        list_idx[base + pos] = p;
        list_w[base + pos] = v;
      }
      count += __popcll(mask);
    }
    if (threadIdx.x == 0) list_n[img * 5 + l] = count;
    if (l == 0 && bbox != nullptr) {
      for (int o = 32; o > 0; o >>= 1) {
        by0 = min(by0, __shfl_xor(by0, o)); by1 = max(by1, __shfl_xor(by1, o));
        bx0 = min(bx0, __shfl_xor(bx0, o)); bx1 = max(bx1, __shfl_xor(bx1, o));
      }
      if (threadIdx.x == 0) {
        bbox[img * 4 + 0] = by0; bbox[img * 4 + 1] = by1;
        bbox[img * 4 + 2] = bx0; bbox[img * 4 + 3] = bx1;
      }
    }
  }
}

// An image whose weight list is empty at EVERY pyramid level (an all-zero mask) pools
// x * 0: exact zeros whatever the trunk computes (encoders.py:310-317; the reference's
// isclose rule leaves such a mask un-normalised).  Those images need no trunk pass:
// order[j] = the j-th image that has work (ascending), bbox_c its bounding box, *count how
// many there are.  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void compact_images_kernel(
    const int* __restrict__ list_n, int n, const int* __restrict__ bbox,
    int* __restrict__ order, int* __restrict__ bbox_c, int* __restrict__ count) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    int any = 0;
    if (i < n)
      for (int l = 0; l < 5; ++l) any |= list_n[i * 5 + l];
    const bool live = any != 0;
    const unsigned long long m = __ballot(live);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (live) {
      const int j = off + __popcll(m & ((1ull << lane) - 1ull));
      order[j] = i;
      for (int e = 0; e < 4; ++e) bbox_c[j * 4 + e] = bbox[i * 4 + e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += wsum[w];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = base;
}

// features[img][col_off + c] = sum_p w[p] * tap[img][p][c]   (encoders.py:317)
// grid (n_images, ceil(C/64)); 4 waves split the pixel list, lane = channel.
// SHARED (image sharing, share.hip): the grid runs over EXEMPLAR slots, slot i pools the tap
// of trunk slot class_of[i]; slots with class -1 or a class outside [img0, img0 + ncls) do
// nothing (their rows were zero-filled); lists / weights / poison / feature row stay slot i's.
template <int SPLIT_IN, bool SHARED = false>   // 0: fp32 tap, 1: split format, 2: plain f16 (fast mode)
__global__ __launch_bounds__(256) void masked_pool_kernel(
    const float* __restrict__ tap, int P, int C, int level, Levels lv,
    const int* __restrict__ list_idx, const float* __restrict__ list_w,
    const int* __restrict__ list_n, float* __restrict__ features, int fstride,
    int col_off, int img0, float inv_scale, const int* __restrict__ poison = nullptr,
    const int* __restrict__ order = nullptr, const int* __restrict__ live = nullptr,
    const int* __restrict__ class_of = nullptr, int ncls = 0) {
  __shared__ float part[4][64];
  int img, trow;   // image number (lists / features) and row of `tap`
  if constexpr (SHARED) {
    img = blockIdx.x;
    const int cls = class_of[img];
    if (cls < img0 || cls >= img0 + ncls) return;
    trow = cls - img0;
  } else {
    // (image count on the device: slots beyond it hold no image -- their feature rows were
    // zero-filled -- and order[] is only defined below it)
    if (live != nullptr && (int)blockIdx.x + img0 >= *live) return;
    // `tap` points at slot img0 of the batch; lists / features are indexed by the image
    // number (`order`: the batch holds only the images with a non-empty mask, in this order)
    img = order ? order[blockIdx.x + img0] : blockIdx.x + img0;
    trow = blockIdx.x;
  }
  const int c = blockIdx.y * 64 + (threadIdx.x & 63);
  const int phase = threadIdx.x >> 6;
  const long base = (long)img * lv.per_image + lv.off[level];
  const int cnt = list_n[img * 5 + level];
  // split format: channel c lives in group c/8 = 32 B [hi x8 | lo x8]
  const long coff = SPLIT_IN == 1 ? (long)(c >> 3) * 8 : c;
  const float* t = tap + (SPLIT_IN == 2 ? (long)trow * P * (C / 2) : (long)trow * P * C + coff);
  auto fetch = [&](int p) -> float {
    if constexpr (SPLIT_IN == 2) {
      return (float)reinterpret_cast<const _Float16*>(t + (long)p * (C / 2))[c];
    } else if constexpr (SPLIT_IN == 1) {
      const _Float16* q =
          reinterpret_cast<const _Float16*>(t + (long)p * C) + (c & 7);
      return (float)q[0] + (float)q[8];
    } else {
      return t[(long)p * C];
    }
  };
  float acc0 = 0.f, acc1 = 0.f;
  if (c < C) {
    int i = phase;
    for (; i + 4 < cnt; i += 8) {
      const int p0 = list_idx[base + i], p1 = list_idx[base + i + 4];
      const float w0 = list_w[base + i], w1 = list_w[base + i + 4];
      acc0 += w0 * fetch(p0);
      acc1 += w1 * fetch(p1);
    }
    if (i < cnt) acc0 += list_w[base + i] * fetch(list_idx[base + i]);
  }
  part[phase][threadIdx.x & 63] = acc0 + acc1;
  __syncthreads();
  if (phase == 0 && c < C) {
    // (inv_scale: 1 / activation scale of a split-format tap, an exact power of two)
    float f = ((part[0][threadIdx.x] + part[1][threadIdx.x]) +
               (part[2][threadIdx.x] + part[3][threadIdx.x])) * inv_scale;
    // an image with a non-finite pixel: every level of the reference's pyramid is NaN
    if (poison != nullptr && poison[img]) f = __builtin_nanf("");
    features[(long)img * fstride + col_off + c] = f;
  }
}

// The same for split-format taps with a lane per 8-CHANNEL GROUP (round 5): a pixel's group is
// two 16-byte loads (hi, lo) instead of two 2-byte loads per channel, a wave covers 64 groups of
// one listed pixel -- or 64 / (C / 8) pixels when the level has fewer groups -- and the four
// waves walk the list interleaved.  grid (n_images, ceil(C / 512)); partial sums are added in a
// fixed order (slot ascending), so results do not depend on timing (not the bits of
// masked_pool_kernel<1>: another association of the same fp32 sum).
template <bool SHARED = false>   // (see masked_pool_kernel)
__global__ __launch_bounds__(256) void masked_pool_split8_kernel(
    const float* __restrict__ tap, int P, int C, int level, Levels lv,
    const int* __restrict__ list_idx, const float* __restrict__ list_w,
    const int* __restrict__ list_n, float* __restrict__ features, int fstride,
    int col_off, int img0, float inv_scale, const int* __restrict__ poison,
    const int* __restrict__ order, int lpp, const int* __restrict__ live = nullptr,
    const int* __restrict__ class_of = nullptr, int ncls = 0) {
  __shared__ float part[4 * 64 * 8];
  int img, trow;
  if constexpr (SHARED) {
    img = blockIdx.x;
    const int cls = class_of[img];
    if (cls < img0 || cls >= img0 + ncls) return;
    trow = cls - img0;
  } else {
    const int slot_img = blockIdx.x + img0;
    if (live != nullptr && slot_img >= *live) return;   // (see masked_pool_kernel)
    img = order ? order[slot_img] : slot_img;
    trow = blockIdx.x;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = C / 8, pw = 64 / lpp;
  const int gl = lane % lpp, sub = lane / lpp;
  const int g = blockIdx.y * 64 + gl;
  const int slot = wave * pw + sub, nslots = 4 * pw;
  const long base = (long)img * lv.per_image + lv.off[level];
  const int cnt = list_n[img * 5 + level];
  const float* t = tap + (long)trow * P * C + (long)g * 8;
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { a0[e] = 0.f; a1[e] = 0.f; }
  auto add = [&](int i, float (&acc)[8]) {
    const float* q = t + (long)list_idx[base + i] * C;
    const float w = list_w[base + i];
    const f32x4_t hi = *reinterpret_cast<const f32x4_t*>(q);
    const f32x4_t lo = *reinterpret_cast<const f32x4_t*>(q + 4);
    float v[8];
    join8_exact(hi, lo, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += w * v[e];
  };
  if (g < G) {
    int i = slot;
    for (; i + nslots < cnt; i += 2 * nslots) { add(i, a0); add(i + nslots, a1); }
    if (i < cnt) add(i, a0);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[(wave * 64 + lane) * 8 + e] = a0[e] + a1[e];
  __syncthreads();
  if (wave == 0 && sub == 0 && g < G) {
    float sum[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int sb = 0; sb < pw; ++sb)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum[e] += part[(w * 64 + sb * lpp + gl) * 8 + e];
    const bool bad = poison != nullptr && poison[img];
    float* f = features + (long)img * fstride + col_off + g * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bad ? __builtin_nanf("") : sum[e] * inv_scale;
  }
}

// rows of poisoned images -> NaN (SpatialConvEncoder read-out; see preprocess_kernel)
__global__ void poison_fill_kernel(float* __restrict__ out, long per_image, int n,
                                   const int* __restrict__ poison) {
  const long total = (long)n * per_image;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x)
    if (poison[i / per_image]) out[i] = __builtin_nanf("");
}

// calibration (milan_encoder_absmax): max |x| of a trunk activation tensor, fp32 mode
__global__ void act_absmax_kernel(const float* __restrict__ x, long n,
                                  unsigned* __restrict__ out) {
  float m = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float a = fabsf(x[i]);
    m = (a > m || a != a) ? a : m;   // (NaN propagates into the maximum)
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_xor(m, o);
    m = (t > m || t != t) ? t : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}


// ---------------------------------------------------------------------------
// Mask-aware tail of the last stage (round 6, MILAN_FUSE_SPARSE_TAIL)
// ---------------------------------------------------------------------------
// The last stage's output is read by NOTHING but the level-4 pooling, and that reads only the
// pixels under the (bilinearly shrunk) mask: on the benchmark's masks 5.3 of 49 pixels per
// image.  Working backwards through the last two bottlenecks (neither has a downsample
// branch): the last block's c3 / c2 are needed at those pixels S2, its c1 -- and the block
// before it, as input and residual -- at their 3x3 neighbourhoods S1 = dilate(S2) (33 %), that
// block's c1 at S0 = dilate(S1) (56 %).  The reference computes all 49 and multiplies most by
// zero (src/milan/encoders.py:310-317); here the row sets are built on the device from the
// pooling's own pixel lists, the 1x1 convs run over gathered rows, the 3x3 over an explicit
// im2col of the needed rows in the (slice, tap, channel) order of the tap-inner kernel -- the
// same products in the same order, so the pooled features are bitwise those of the dense pass
// (tests/test_gpu_sparse_tail.py) -- and the row counts stay on the device (GemmArgs::m_live).
// (kTailMaxP, kTailMaxP3 -- pixels of the last two stages per image -- are in enc_plan.h)

// Image sharing: set 0 of trunk slot c is the UNION of its members' level-4 lists, gathered
// here as a byte map s0[c][p] (zero-filled; every writer stores the same 1).  Dilation
// distributes over union, so sets 1 and 2 of tail_sets_kernel are then exactly the pixels
// some member's pooling depends on.
// (level 3: the same for the level-3 lists, which join set W of tail_sets3_kernel)
__global__ __launch_bounds__(64) void tail_union_kernel(
    const int* __restrict__ list_idx, const int* __restrict__ list_n, Levels lv,
    const int* __restrict__ class_of, int P, unsigned char* __restrict__ s0, int level) {
  const int i = blockIdx.x, c = class_of[i];
  if (c < 0) return;
  const long base = (long)i * lv.per_image + lv.off[level];
  const int cnt = list_n[i * 5 + level];
  for (int e = threadIdx.x; e < cnt; e += 64) s0[(long)c * P + list_idx[base + e]] = 1;
}

// sets k = 0 (listed pixels), 1 (dilated once), 2 (dilated twice) of batch slot j, ascending
// (s0 != nullptr: set 0 is given as a byte map, see tail_union_kernel)
// dummy (MILAN_FUSE_TAIL_LISTS): a live slot whose set 0 is empty -- a mask that misses every
// centre of the last level -- gets pixel 0, so that EVERY set of every live slot is non-empty
// and 256 consecutive entries of a row list span at most 256 slots (GemmArgs::row_list).
// Nothing reads the extra rows.
__global__ __launch_bounds__(64) void tail_sets_kernel(
    const int* __restrict__ list_idx, const int* __restrict__ list_n, Levels lv,
    const int* __restrict__ order, const int* __restrict__ live, int n,
    int* __restrict__ loc, int* __restrict__ cnt,
    const unsigned char* __restrict__ s0, int dummy) {
  __shared__ unsigned char s[3][kTailMaxP];
  const int j = blockIdx.x, lane = threadIdx.x;
  const int h = lv.h[4], w = lv.w[4], P = h * w;
  if (live != nullptr && j >= *live) {
    if (lane < 3) cnt[lane * n + j] = 0;
    return;
  }
  const int img = order ? order[j] : j;
  if (s0 != nullptr) {
    for (int p = lane; p < P; p += 64) s[0][p] = s0[(long)j * P + p];
  } else {
    for (int p = lane; p < P; p += 64) s[0][p] = 0;
    __syncthreads();
    const long base = (long)img * lv.per_image + lv.off[4];
    const int c = list_n[img * 5 + 4];
    for (int i = lane; i < c; i += 64) s[0][list_idx[base + i]] = 1;
  }
  __syncthreads();
  if (dummy) {
    int any = 0;
    for (int p = lane; p < P; p += 64) any |= s[0][p];
    if (__ballot(any != 0) == 0ull && lane == 0) s[0][0] = 1;
    __syncthreads();
  }
  for (int k = 1; k < 3; ++k) {
    for (int p = lane; p < P; p += 64) {
      const int y = p / w, x = p - y * w;
      unsigned char v = 0;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if (yy >= 0 && yy < h && xx >= 0 && xx < w) v |= s[k - 1][yy * w + xx];
        }
      s[k][p] = v;
    }
    __syncthreads();
  }
  for (int k = 0; k < 3; ++k) {
    int count = 0;
    int* out = loc + ((long)k * n + j) * P;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int p = p0 + lane;
      const bool nz = p < P && s[k][p];
      const unsigned long long m = __ballot(nz);
      if (nz) out[count + __popcll(m & ((1ull << lane) - 1ull))] = p;
      count += __popcll(m);
    }
    if (lane == 0) cnt[k * n + j] = count;
  }
}

// Row sets of the stage BEFORE the last one (MILAN_FUSE_TAIL_LISTS), from set k0 of the last
// stage = the pixels its first block's output is needed at.  That block's k x k / strided conv
// c2 reads its c1 output -- a 1x1 conv: the block input -- at
//   set 0 (V) = { (y * stride - pad + a, x * stride - pad + b) inside the image },
// its downsample conv reads the block input at (y * ds_stride, x * ds_stride), and the pooling
// of this stage reads its own pixel list:
//   set 1 (W) = V + the downsample's pixels + the listed pixels (s3 != nullptr: their union
//               over the members of the trunk slot, see tail_union_kernel)
// is where the last block of this stage is needed.  Ascending, like tail_sets_kernel.
__global__ __launch_bounds__(64) void tail_sets3_kernel(
    const int* __restrict__ loc, const int* __restrict__ cnt, int k0,
    const int* __restrict__ list_idx, const int* __restrict__ list_n, Levels lv,
    const int* __restrict__ order, const int* __restrict__ live, int n, int kh, int kw,
    int stride, int pad, int ds_stride, const unsigned char* __restrict__ s3,
    int* __restrict__ loc3, int* __restrict__ cnt3) {
  __shared__ unsigned char s[2][kTailMaxP3];
  const int j = blockIdx.x, lane = threadIdx.x;
  const int w4 = lv.w[4], P4 = lv.h[4] * w4;
  const int h3 = lv.h[3], w3 = lv.w[3], P3 = h3 * w3;
  if (live != nullptr && j >= *live) {
    if (lane < 2) cnt3[lane * n + j] = 0;
    return;
  }
  for (int p = lane; p < P3; p += 64) {
    s[0][p] = 0;
    s[1][p] = s3 != nullptr ? s3[(long)j * P3 + p] : 0;
  }
  __syncthreads();
  if (s3 == nullptr) {
    const int img = order ? order[j] : j;
    const long base = (long)img * lv.per_image + lv.off[3];
    const int c = list_n[img * 5 + 3];
    for (int i = lane; i < c; i += 64) s[1][list_idx[base + i]] = 1;
  }
  const int c0 = cnt[k0 * n + j];
  const int* l0 = loc + ((long)k0 * n + j) * P4;
  for (int i = lane; i < c0; i += 64) {
    const int p = l0[i], y = p / w4, x = p - y * w4;
    for (int a = 0; a < kh; ++a)
      for (int b = 0; b < kw; ++b) {
        const int yy = y * stride - pad + a, xx = x * stride - pad + b;
        if (yy >= 0 && yy < h3 && xx >= 0 && xx < w3) { s[0][yy * w3 + xx] = 1; s[1][yy * w3 + xx] = 1; }
      }
    const int yd = y * ds_stride, xd = x * ds_stride;
    if (yd < h3 && xd < w3) s[1][yd * w3 + xd] = 1;
  }
  __syncthreads();
  for (int k = 0; k < 2; ++k) {
    int count = 0;
    int* out = loc3 + ((long)k * n + j) * P3;
    for (int p0 = 0; p0 < P3; p0 += 64) {
      const int p = p0 + lane;
      const bool nz = p < P3 && s[k][p];
      const unsigned long long m = __ballot(nz);
      if (nz) out[count + __popcll(m & ((1ull << lane) - 1ull))] = p;
      count += __popcll(m);
    }
    if (lane == 0) cnt3[k * n + j] = count;
  }
}

// off[k][j] = rows of set k in the slots before j; U[k] = their total
__global__ __launch_bounds__(256) void tail_scan_kernel(const int* __restrict__ cnt, int n,
                                                        int* __restrict__ off, int* __restrict__ U) {
  __shared__ int tmp[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  int base = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const int v = j < n ? cnt[(long)k * n + j] : 0;
    tmp[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int add = tid >= o ? tmp[tid - o] : 0;
      __syncthreads();
      tmp[tid] += add;
      __syncthreads();
    }
    if (j < n) off[(long)k * n + j] = base + tmp[tid] - v;
    base += tmp[255];
    __syncthreads();
  }
  if (tid == 0) U[k] = base;
}

// rows[k][off[k][j] + i] = j * P + loc[k][j][i]  (row of the dense (slot, pixel) tensors)
__global__ void tail_fill_kernel(const int* __restrict__ loc, const int* __restrict__ cnt,
                                 const int* __restrict__ off, int n, int P, int* __restrict__ rows) {
  const int j = blockIdx.x, k = blockIdx.y;
  const int c = cnt[k * n + j], o = off[k * n + j];
  for (int i = threadIdx.x; i < c; i += blockDim.x)
    rows[(long)k * n * P + o + i] = j * P + loc[((long)k * n + j) * P + i];
}

// dst[u][:] = src[idx[u]][:] / dst[idx[u]][:] = src[u][:]  (rows of w4 x 16 bytes), u < *live
template <bool SCATTER>
__global__ void tail_rows_kernel(const float4* __restrict__ src, const int* __restrict__ idx,
                                 const int* __restrict__ live, int w4, float4* __restrict__ dst) {
  const long total = (long)*live * w4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long u = i / w4;
    const int q = (int)(i - u * w4);
    if (SCATTER) dst[(long)idx[u] * w4 + q] = src[i];
    else dst[i] = src[(long)idx[u] * w4 + q];
  }
}

// explicit im2col of a 3x3 / 1 / 1 conv for the rows in `rows`: column order (32-channel slice,
// tap, channel) = the k order of the tap-inner ping-pong kernel and of ConvW::wst; pixels
// outside the image contribute zeros.  t1: dense [slots * P][C] split format, C % 32 == 0.
__global__ void tail_im2col_kernel(const float4* __restrict__ t1, const int* __restrict__ rows,
                                   const int* __restrict__ live, int h, int w, int C,
                                   float4* __restrict__ acol) {
  const int per = 9 * C / 4, P = h * w, c4 = C / 4;
  const long total = (long)*live * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long u = i / per;
    const int q = (int)(i - u * per);
    const int sl = q / 72, r = q - sl * 72, tap = r >> 3, f = r & 7;
    const int row = rows[u];
    const int j = row / P, p = row - j * P;
    const int y = p / w + tap / 3 - 1, x = p % w + tap % 3 - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < h && x >= 0 && x < w)
      v = t1[((long)j * P + y * w + x) * c4 + sl * 8 + f];
    acol[i] = v;
  }
}

// ---------------------------------------------------------------------------
// driver: carve (enc_carve), plan (plan_encoder, enc_plan.h), walk the plan
// ---------------------------------------------------------------------------
// The knobs of the encoder pass, from the environment: the only getenv on it (README /
// DESIGN 5).  MILAN_TAPS_INNER exists in the experiments build alone.
static EncEnv read_enc_env() {
  auto num = [](const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
  };
  EncEnv env;
  env.stem_u8 = num("MILAN_STEM_U8", 1) != 0;
  env.pool_vec = num("MILAN_POOL_VEC", 1) != 0;
  // Images per encoder pass: bounds the activation workspace (16 MB/image; 9600 =
  // 640 neurons x 15 exemplars = 154 GB of the 288).  Smaller sub-batches were
  // tried for Infinity-Cache locality and lost (tail effects of the smaller GEMM
  // grids dominate; measured: 240 -15%, 480 -8%, 960 -4% vs 3840).
  env.enc_sub = num("MILAN_ENC_SUB", 9600);
  if (env.enc_sub < 1) env.enc_sub = 9600;
#if MILAN_EXPERIMENTS
  env.taps_inner = num("MILAN_TAPS_INNER", 0) != 0;
#endif
  return env;
}
// ... once per process
static const EncEnv& enc_env() {
  static const EncEnv env = read_enc_env();
  return env;
}
static int encoder_sub_batch() { return enc_env().enc_sub; }

static void alexnet_workspace_dry(const milan_ctx* c, int n, int H, int W,
                                  Arena& a);

size_t encoder_workspace(const milan_ctx* c, int n_images, int H, int W) {
  Arena a; a.dry = true;
  const int sub = encoder_sub_batch();
  const int n = n_images < sub ? n_images : sub;
  if (c->d.trunk_kind == MILAN_TRUNK_NONE || c->d.trunk_kind == MILAN_TRUNK_ALEXNET_PLACES ||
      c->d.trunk_kind == MILAN_TRUNK_VGG)
    return 0;
  if (c->d.trunk_kind == MILAN_TRUNK_ALEXNET) {
    alexnet_workspace_dry(c, n, H, W, a);
    return a.off;
  }
  EncBuffers pl;
  enc_carve(c->d.trunk_kind, c->d.trunk_width, n, H, W, &a, &pl);
  return a.off;
}

static int encoder_run_batch(milan_ctx* c, const void* images, int image_dtype,
                             const void* masks, int mask_dtype, int n, int H,
                             int W, float* features, Arena& ws, hipStream_t s,
                             float* spatial_out = nullptr);
static int alexnet_run_batch(milan_ctx* c, const void* images, int image_dtype,
                             const void* masks, int mask_dtype, int n, int H,
                             int W, float* features, Arena& ws, hipStream_t s);

// one pass per sub-batch of images; `out` advances by `per_image` floats per image
static int run_sub_batches(milan_ctx* c, const void* images, int image_dtype, const void* masks,
                           int mask_dtype, int n, int H, int W, float* out, size_t per_image,
                           bool spatial, Arena& ws, hipStream_t s) {
  const int sub = encoder_sub_batch();
  const size_t isz = image_dtype == MILAN_DTYPE_U8 ? 1 : 4;
  const size_t msz = mask_dtype == MILAN_DTYPE_U8 ? 1 : 4;
  for (int lo = 0; lo < n; lo += sub) {
    const int cnt = n - lo < sub ? n - lo : sub;
    Arena a = ws;  // every pass reuses the same scratch
    const char* im = (const char*)images + (size_t)lo * 3 * H * W * isz;
    const char* mk = masks ? (const char*)masks + (size_t)lo * H * W * msz : nullptr;
    float* o = out + lo * per_image;
    MILAN_TRY(encoder_run_batch(c, im, image_dtype, mk, mask_dtype, cnt, H, W,
                                spatial ? nullptr : o, a, s, spatial ? o : nullptr));
    if (a.off > ws.off) ws.off = a.off > ws.size ? ws.size : ws.off;
  }
  return 0;
}

int encoder_run(milan_ctx* c, const void* images, int image_dtype,
                const void* masks, int mask_dtype, int n, int H, int W,
                float* features, Arena& ws, hipStream_t s) {
  return run_sub_batches(c, images, image_dtype, masks, mask_dtype, n, H, W, features,
                         (size_t)c->d.feature_size, false, ws, s);
}

// spatial_out != nullptr: SpatialConvEncoder mode (encoders.py:158-230) -- the
// image is normalised and THEN multiplied by its mask, no pyramid pooling, and
// the last stage's NHWC output (n, h4*w4, C4) is the result.
int encoder_run_spatial(milan_ctx* c, const void* images, int image_dtype,
                        const void* masks, int mask_dtype, int n, int H, int W,
                        float* out, Arena& ws, hipStream_t s) {
  MILAN_REQUIRE(c->d.trunk_kind != MILAN_TRUNK_ALEXNET &&
                    c->d.trunk_kind != MILAN_TRUNK_ALEXNET_PLACES &&
                    c->d.trunk_kind != MILAN_TRUNK_VGG,
                MILAN_ERR_ARG, "spatial encoding needs a ResNet trunk");
  EncBuffers pl;
  enc_carve(c->d.trunk_kind, c->d.trunk_width, 1, H, W, nullptr, &pl);
  const int C = (c->d.trunk_kind == MILAN_TRUNK_BASIC ? c->d.trunk_width
                                                      : c->d.trunk_width * 4) << 3;
  return run_sub_batches(c, images, image_dtype, masks, mask_dtype, n, H, W, out,
                         (size_t)pl.lv.h[4] * pl.lv.w[4] * C, true, ws, s);
}

// One pass: its arguments, its buffers, its schedule, and what the input phase finds out
// about the batch.  The functions below launch what the schedule names.
struct EncPass {
  milan_ctx* c;
  hipStream_t s;
  const void* images;
  int image_dtype;
  const void* masks;
  int mask_dtype, n, H, W;
  float *features, *spatial_out;
  EncBuffers pl;
  EncSchedule sc;
  // float inputs can carry NaN / Inf pixels (uint8 ones cannot): image-level poison flags
  int* poison;
  // a compacted pass: batch slot j holds image order[j] (classes: the root image of live class
  // j, and the pooling of exemplar slot i reads trunk slot class_of[i]); bbox: level-0 boxes
  const int *order, *class_of, *bbox;
};

// calibration pass (milan_encoder_absmax): max |x| over every activation tensor of the fp32
// pass (`word` 1: the word next to it, which bounds the FEATURES -- milan_encoder_absmax folds
// the raw conv1 output in there, pyramid tap 0, which is no split activation)
static int track(const EncPass& p, const float* t, long count, int word = 0) {
  if (p.c->calib == nullptr || p.sc.split || count <= 0) return 0;
  const int blocks = (int)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
  hipLaunchKernelGGL(act_absmax_kernel, dim3(blocks), dim3(256), 0, p.s, t, count,
                     p.c->calib + word);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}
static int run_gemm(const EncPass& p, const GemmArgs& g) {
  MILAN_TRY(launch_gemm(g, p.s));
  return track(p, g.C, (long)g.M * g.N);
}

// everything the schedule depends on, from the context and the call
static int enc_ask(const milan_ctx* c, const void* images, int image_dtype, const void* masks,
                   int mask_dtype, int n, int H, int W, bool spatial, EncAsk* a) {
  a->trunk_kind = c->d.trunk_kind; a->width = c->d.trunk_width; a->feature_size = c->d.feature_size;
  a->blocks = c->blocks; a->stem = &c->stem; a->stem_pair = &c->stem_pair;
  a->precision = c->precision; a->trunk_f16 = c->trunk_f16; a->fusion = c->fusion;
  a->calib = c->calib != nullptr; a->share = c->share_images != 0;
  for (int ch = 0; ch < 3; ++ch) { a->mean[ch] = c->mean[ch]; a->stdv[ch] = c->stdv[ch]; }
  a->n = n; a->H = H; a->W = W; a->image_dtype = image_dtype;
  a->images_aligned4 = (reinterpret_cast<uintptr_t>(images) & 3) == 0;
  a->masks = masks != nullptr; a->mask_dtype = mask_dtype; a->spatial = spatial;
  a->zero = c->zero;
  a->env = enc_env();
  return gemm_env(&a->genv);
}

// 1. masks -> per-level normalised sparse weight lists; which images take part; 2. images ->
// normalised NHWC4 (fp32 stem) or pixel-pair groups (split stem)
static int run_input(EncPass& p) {
  milan_ctx* c = p.c;
  const EncBuffers& pl = p.pl;
  const int n = p.n, H = p.H, W = p.W;
  hipStream_t s = p.s;
  StageScope scope(MILAN_STAGE_ENC_INPUT, s);
  if (p.spatial_out != nullptr) {
    // no pooling
  } else if (p.masks == nullptr || p.mask_dtype == MILAN_DTYPE_U8)
    hipLaunchKernelGGL(mask_pyramid_kernel<uint8_t>, dim3(n, 5), dim3(256), 0, s,
                       (const uint8_t*)p.masks, H, W, pl.lv, pl.list_idx,
                       pl.list_w, pl.list_n, pl.bbox);
  else
    hipLaunchKernelGGL(mask_pyramid_kernel<float>, dim3(n, 5), dim3(256), 0, s,
                       (const float*)p.masks, H, W, pl.lv, pl.list_idx, pl.list_w,
                       pl.list_n, pl.bbox);
  MILAN_CHECK_HIP(hipGetLastError());

  // Images with an all-zero mask pool exact zeros at every level: they stay out of the trunk
  // pass (COMPACT_SKIP_EMPTY).  Batch slot j holds image order[j]; HOW MANY slots hold work
  // stays on the device (round 6: sc.live, one word written by compact_images_kernel): every
  // launch below is sized for all n images and reads the count itself (GemmArgs::m_live), so
  // nothing is read back and the stream is never synchronised -- the header's "all work is
  // enqueued on `stream`" holds and the whole pass can be captured into a hipGraph.
  // Image sharing (COMPACT_CLASSES; share.hip): slots of this pass that show the same uint8
  // image share one trunk slot.  The same mechanism, generalised: slot j of the trunk batch
  // holds the root image of the j-th live class (order[j]), bbox_c[j] is the union of the
  // members' boxes and the pooling of exemplar slot i reads trunk slot class_of[i].  masks may
  // be NULL (every list is full: one class per distinct image).
  if (p.sc.compact == COMPACT_CLASSES) {
    ShareArgs sa{};
    sa.images = (const unsigned char*)p.images; sa.bytes = (long)3 * H * W; sa.n = n;
    sa.hash_bits = c->share_hash_bits;
    sa.skip_empty = (c->fusion & MILAN_FUSE_SKIP_EMPTY) != 0;
    sa.list_n = pl.list_n; sa.bbox = pl.bbox; sa.hash = pl.sh_hash; sa.rep = pl.sh_rep;
    sa.flag = pl.sh_flag; sa.order = pl.order; sa.bbox_c = pl.bbox_c; sa.count = pl.count;
    sa.class_of = pl.class_of;
    MILAN_TRY(launch_image_classes(sa, s));
    p.class_of = pl.class_of;
  } else if (p.sc.compact == COMPACT_SKIP_EMPTY) {
    hipLaunchKernelGGL(compact_images_kernel, dim3(1), dim3(1024), 0, s, pl.list_n, n,
                       pl.bbox, pl.order, pl.bbox_c, pl.count);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  if (p.sc.compact != COMPACT_NONE) {
    // rows of the images without work: exact zeros (the pooling writes the others)
    MILAN_TRY(launch_zero_fill(p.features, sizeof(float) * (size_t)n * c->d.feature_size, s));
    p.order = pl.order;
  }
  // the device-side counters of milan_image_sharing_stats (only while sharing is enabled: the
  // default pass launches what it always did); a pass that does not share counts slots == images
  if (c->share_images && c->share_stats != nullptr)
    MILAN_TRY(launch_share_count(c->share_stats, n, p.class_of ? p.sc.live : nullptr, s));
  p.bbox = p.order ? pl.bbox_c : pl.bbox;

  // the fused stem reads uint8 images itself (StemArgs::in_u8): no pixel-pair tensor
  // (MILAN_STEM_U8=0: through preprocess_pairs_kernel, the same bits; A/B timing)
  if (p.sc.stem_u8) {
    if (c->stem_lut == nullptr) MILAN_TRY(dev_alloc(c, (void**)&c->stem_lut, sizeof(unsigned) * 772));
    hipLaunchKernelGGL(stem_lut_kernel, dim3(1), dim3(128), 0, s, c->mean[0], c->mean[1], c->mean[2],
                       c->stdv[0], c->stdv[1], c->stdv[2], c->stem_lut);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  }
  const bool pair_stem = p.sc.pair_stem;
  const int G = (W + 2) / 2;  // pixel-pair groups per image row
  const long np = pair_stem ? (long)n * H * G : (long)n * H * W;
  const int blocks = (int)((np + 255) / 256 < 8192 ? (np + 255) / 256 : 8192);
  const float m0 = c->mean[0], m1 = c->mean[1], m2 = c->mean[2];
  const float s0 = c->stdv[0], s1 = c->stdv[1], s2 = c->stdv[2];
  const void* mul = p.spatial_out ? p.masks : nullptr;  // spatial mode: x * mask
  const int mul_u8 = p.mask_dtype == MILAN_DTYPE_U8;
  int* const poison = p.poison;
  if (poison) MILAN_TRY(launch_zero_fill(poison, sizeof(int) * (size_t)n, s));
  if (pair_stem && p.image_dtype == MILAN_DTYPE_U8)
    hipLaunchKernelGGL(preprocess_pairs_kernel<uint8_t>, dim3(blocks),
                       dim3(256), 0, s, (const uint8_t*)p.images, np, H, W, G,
                       m0, m1, m2, s0, s1, s2, pl.in4, mul, mul_u8, nullptr, c->status,
                       p.order, p.sc.live);
  else if (pair_stem)
    hipLaunchKernelGGL(preprocess_pairs_kernel<float>, dim3(blocks), dim3(256),
                       0, s, (const float*)p.images, np, H, W, G, m0, m1, m2, s0,
                       s1, s2, pl.in4, mul, mul_u8, poison, c->status);
  else if (p.image_dtype == MILAN_DTYPE_U8)
    hipLaunchKernelGGL(preprocess_kernel<uint8_t>, dim3(blocks), dim3(256), 0,
                       s, (const uint8_t*)p.images, np, H * W, m0, m1, m2, s0, s1,
                       s2, (float4*)pl.in4, mul, mul_u8, nullptr, nullptr, p.order, p.sc.live);
  else
    hipLaunchKernelGGL(preprocess_kernel<float>, dim3(blocks), dim3(256), 0, s,
                       (const float*)p.images, np, H * W, m0, m1, m2, s0, s1, s2,
                       (float4*)pl.in4, mul, mul_u8, poison, c->status);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Pools the level-`level` tensor `tap` of the n trunk slots with the kernel the schedule
// names.  Image sharing: the grid runs over all exemplar slots, which read n trunk slots.
static int run_pool(const EncPass& p, const float* tap, int level) {
  if (p.spatial_out != nullptr) return 0;
  const EncBuffers& pl = p.pl;
  const int C = p.sc.pool_C[level], col_off = p.sc.pool_col[level], kind = p.sc.pool[level];
  const int P = pl.lv.h[level] * pl.lv.w[level], F = p.c->d.feature_size, n = p.n;
  const bool shared = p.class_of != nullptr;
  const float inv_scale = kind == POOL_F32 ? 1.f : 1.f / p.c->act_scale;
  const int ncls = shared ? n : 0;
  StageScope scope(MILAN_STAGE_ENC_POOL, p.s);
  if (kind == POOL_SPLIT8) {
    const int G = C / 8;
    hipLaunchKernelGGL(shared ? masked_pool_split8_kernel<true> : masked_pool_split8_kernel<false>,
                       dim3(n, (G + 63) / 64), dim3(256), 0, p.s, tap, P, C, level, pl.lv,
                       pl.list_idx, pl.list_w, pl.list_n, p.features, F, col_off, 0, inv_scale,
                       p.poison, p.order, G < 64 ? G : 64, p.sc.live, p.class_of, ncls);
  } else {
    const auto kern = kind == POOL_F16     ? (shared ? masked_pool_kernel<2, true> : masked_pool_kernel<2, false>)
                      : kind == POOL_SPLIT ? (shared ? masked_pool_kernel<1, true> : masked_pool_kernel<1, false>)
                                           : (shared ? masked_pool_kernel<0, true> : masked_pool_kernel<0, false>);
    hipLaunchKernelGGL(kern, dim3(n, (C + 63) / 64), dim3(256), 0, p.s, tap, P, C, level, pl.lv,
                       pl.list_idx, pl.list_w, pl.list_n, p.features, F, col_off, 0, inv_scale,
                       p.poison, p.order, p.sc.live, p.class_of, ncls);
  }
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// 3. stem: raw conv1 (tap 0), then bn1+relu+maxpool
static int run_stem(const EncPass& p) {
  milan_ctx* c = p.c;
  const EncBuffers& pl = p.pl;
  const int n = p.n, wd = c->d.trunk_width;
  const bool spatial = p.spatial_out != nullptr;
  hipStream_t s = p.s;
  if (p.sc.fused_stem) {
    // conv1 + bn1 + ReLU + maxpool in one persistent launch (stem.hip); the raw
    // tensor is only materialised where the level-0 pooling will read it
    StemArgs sa{};
    sa.in = pl.in4; sa.ws = c->stem_pair.ws; sa.bias = c->stem_pair.bias;
    if (p.sc.stem_u8) {
      sa.in = nullptr; sa.in_u8 = (const unsigned char*)p.images; sa.lut = c->stem_lut;
      sa.order = p.order; sa.W = p.W;
    }
    sa.n_live = p.sc.live;
    sa.acc_scale = c->stem_pair.ws_inv;
    sa.scale = c->bn1_scale_s; sa.shift = c->bn1_shift_s;  // (activation scale)
    sa.raw = spatial ? nullptr : pl.raw; sa.y = pl.x0;
    sa.bbox = spatial ? nullptr : p.bbox;
    sa.zero = c->zero;
    sa.n = n; sa.H = p.H; sa.G = (p.W + 2) / 2; sa.h1 = pl.h1; sa.w1 = pl.w1;
    sa.hp = pl.hp; sa.wp = pl.wp;
    {
      StageScope scope(MILAN_STAGE_ENC_STEM, s);
      MILAN_TRY(launch_stem_fused(sa, s));
    }
    return run_pool(p, pl.raw, 0);
  }
  const GemmArgs& g = p.sc.stem;
  {
    StageScope scope(MILAN_STAGE_ENC_STEM, s);
    MILAN_TRY(launch_gemm(g, s));
  }
  MILAN_TRY(track(p, g.C, (long)g.M * g.N, 1));
  MILAN_TRY(run_pool(p, pl.raw, 0));
  {
    StageScope scope(MILAN_STAGE_ENC_STEM_TAIL, s);
    const bool split = p.sc.split;
    const long total = (long)n * pl.hp * pl.wp * (wd / (split ? 8 : 4));
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (split)
      hipLaunchKernelGGL(bn_relu_maxpool_split_kernel, dim3(blocks), dim3(256), 0,
                         s, pl.raw, n, pl.h1, pl.w1, wd, pl.hp, pl.wp,
                         c->bn1_scale_s, c->bn1_shift_s, pl.x0, c->status, p.sc.live);
    else
      hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(blocks), dim3(256), 0, s,
                         (const float4*)pl.raw, n, pl.h1, pl.w1, wd / 4, pl.hp,
                         pl.wp, (const float4*)c->bn1_scale,
                         (const float4*)c->bn1_shift, (float4*)pl.x0, p.sc.live);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return track(p, pl.x0, (long)n * pl.hp * pl.wp * wd);
}

// 3b. the row sets of the mask-aware tail (sc.tail; kernels above): sets 0..2 of the last
// stage from the level-4 pixel lists, and with k0 >= 0 the sets V, W of the stage before
static int run_tail_sets(const EncPass& p) {
  const EncBuffers& pl = p.pl;
  const int n = p.n, P4 = pl.lv.h[4] * pl.lv.w[4], P3 = pl.lv.h[3] * pl.lv.w[3];
  hipStream_t s = p.s;
  if (p.sc.tail) {
    const unsigned char* s0 = nullptr;
    if (p.class_of != nullptr) {
      MILAN_TRY(launch_zero_fill(pl.tail_s0, ((size_t)n * P4 + 3) & ~(size_t)3, s));
      hipLaunchKernelGGL(tail_union_kernel, dim3(n), dim3(64), 0, s, pl.list_idx, pl.list_n, pl.lv,
                         p.class_of, P4, pl.tail_s0, 4);
      s0 = pl.tail_s0;
    }
    hipLaunchKernelGGL(tail_sets_kernel, dim3(n), dim3(64), 0, s, pl.list_idx, pl.list_n, pl.lv,
                       p.order, p.sc.live, n, pl.tail_loc, pl.tail_cnt, s0, p.sc.lists ? 1 : 0);
    hipLaunchKernelGGL(tail_scan_kernel, dim3(3), dim3(256), 0, s, pl.tail_cnt, n, pl.tail_off,
                       pl.tail_U);
    hipLaunchKernelGGL(tail_fill_kernel, dim3(n, 3), dim3(64), 0, s, pl.tail_loc, pl.tail_cnt,
                       pl.tail_off, n, P4, pl.tail_rows);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  if (p.sc.k0 >= 0) {
    const Bottleneck& f = p.c->blocks[3][0];
    const unsigned char* s3 = nullptr;
    if (p.class_of != nullptr) {
      // image sharing: a trunk slot's level-3 pixels are the union of its members' lists
      MILAN_TRY(launch_zero_fill(pl.tail_s3, ((size_t)n * P3 + 3) & ~(size_t)3, s));
      hipLaunchKernelGGL(tail_union_kernel, dim3(n), dim3(64), 0, s, pl.list_idx, pl.list_n, pl.lv,
                         p.class_of, P3, pl.tail_s3, 3);
      s3 = pl.tail_s3;
    }
    hipLaunchKernelGGL(tail_sets3_kernel, dim3(n), dim3(64), 0, s, pl.tail_loc, pl.tail_cnt, p.sc.k0,
                       pl.list_idx, pl.list_n, pl.lv, p.order, p.sc.live, n, f.c2.kh, f.c2.kw,
                       f.c2.stride, f.c2.pad, f.down.stride, s3, pl.tail_loc3, pl.tail_cnt3);
    hipLaunchKernelGGL(tail_scan_kernel, dim3(2), dim3(256), 0, s, pl.tail_cnt3, n, pl.tail_off3,
                       pl.tail_U3);
    hipLaunchKernelGGL(tail_fill_kernel, dim3(n, 2), dim3(64), 0, s, pl.tail_loc3, pl.tail_cnt3,
                       pl.tail_off3, n, P3, pl.tail_rows3);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

// c1 and c2 of a block, where they are launches of their own
static int run_front(const EncPass& p, const EncBlock& r) {
  if (r.c1 == C1_LAUNCH || r.c1 == C1_LIST) MILAN_TRY(run_gemm(p, r.g1));
  if (r.c2 == C2_CONV3) {
    // layer1's 3x3: weights in registers, input tile staged once (conv3.hip)
    const ConvW& c2 = r.b->c2;
    Conv3Args ca{};
    ca.in = r.g2.A; ca.ws = c2.ws; ca.bias = c2.bias_s; ca.acc_scale = c2.ws_inv;
    ca.out = r.g2.C; ca.zero = p.c->zero; ca.n = p.n; ca.h = r.g2.H; ca.w = r.g2.Wd;
    ca.n_live = p.sc.live;
    return launch_conv3_p64(ca, p.s);
  }
  if (r.c2 != C2_NONE) MILAN_TRY(run_gemm(p, r.g2));
  return 0;
}

// TAIL_COPY: one bottleneck on gathered rows -- c1 at set kM, c2 / c3 at set kO; X is dense
// [n * P4][4P] (valid at least on set kM), Y gets the rows of set kO
static int run_tail_copy(const EncPass& p, const EncBlock& r) {
  const EncBuffers& pl = p.pl;
  const int P4 = pl.lv.h[4] * pl.lv.w[4];
  const long rows_all = (long)p.n * P4;
  const int Cin = r.b->c1.cin, P = r.b->c1.cout, Cout = r.b->c3.cout;
  const int* rowsM = pl.tail_rows + (long)r.kM * p.n * P4;
  const int* rowsO = pl.tail_rows + (long)r.kO * p.n * P4;
  const int *UM = pl.tail_U + r.kM, *UO = pl.tail_U + r.kO;
  hipStream_t s = p.s;
  auto blocks_for = [](long items) { return (int)((items + 255) / 256 < 8192 ? (items + 255) / 256 : 8192); };
  hipLaunchKernelGGL(tail_rows_kernel<false>, dim3(blocks_for(rows_all * (Cin / 4))), dim3(256), 0, s,
                     (const float4*)r.X, rowsM, UM, Cin / 4, (float4*)r.g1.A);
  MILAN_TRY(launch_gemm(r.g1, s));
  hipLaunchKernelGGL(tail_rows_kernel<true>, dim3(blocks_for(rows_all * (P / 4))), dim3(256), 0, s,
                     (const float4*)r.g1.C, rowsM, UM, P / 4, (float4*)r.T1);
  hipLaunchKernelGGL(tail_im2col_kernel, dim3(blocks_for(rows_all * (9 * P / 4))), dim3(256), 0, s,
                     (const float4*)r.T1, rowsO, UO, r.h, r.w, P, (float4*)r.g2.A);
  MILAN_TRY(launch_gemm(r.g2, s));
  hipLaunchKernelGGL(tail_rows_kernel<false>, dim3(blocks_for(rows_all * (Cin / 4))), dim3(256), 0, s,
                     (const float4*)r.X, rowsO, UO, Cin / 4, (float4*)r.g3.aux);
  MILAN_TRY(launch_gemm(r.g3, s));
  hipLaunchKernelGGL(tail_rows_kernel<true>, dim3(blocks_for(rows_all * (Cout / 4))), dim3(256), 0, s,
                     (const float4*)r.g3.C, rowsO, UO, Cout / 4, (float4*)r.Y);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int run_block(const EncPass& p, const EncBlock& r) {
  switch (r.form) {
    case EF_TAIL_COPY:
      return run_tail_copy(p, r);
    case EF_BASIC:
      MILAN_TRY(run_gemm(p, r.g1));
      if (r.has_gd) MILAN_TRY(run_gemm(p, r.gd));
      return run_gemm(p, r.g2);
    case EF_CHAIN_PLAIN:
    case EF_CHAIN_DS:
      MILAN_TRY(run_front(p, r));
      return launch_chain(r.chain, p.s);
    case EF_F16:
    case EF_TAIL_LISTS:
    case EF_LIST_FIRST:
    case EF_LIST_LAST3:
    case EF_TWO_SOURCE:
    case EF_PLAIN:
      MILAN_TRY(run_front(p, r));
      if (r.has_gd) MILAN_TRY(run_gemm(p, r.gd));
      return run_gemm(p, r.g3);
  }
  MILAN_REQUIRE(false, MILAN_ERR_STATE, "internal: block without a form");
}

// spatial mode: layer4 output, NHWC == the reference's permute(0, 2, 3, 1): (n, h*w, C)
static int run_spatial_out(const EncPass& p) {
  const int C = p.sc.pool_C[4], h = p.sc.h_out[3], w = p.sc.w_out[3];
  const float* x = p.sc.out[3];
  const long rows = (long)p.n * h * w;
  hipStream_t s = p.s;
  if (p.sc.split) {
    const long total = rows * (C / 8);
    const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(split_to_f32_kernel, dim3(blocks), dim3(256), 0, s, x,
                       total, p.spatial_out, 1.f / p.c->act_scale);
    MILAN_CHECK_HIP(hipGetLastError());
  } else {
    MILAN_CHECK_HIP(hipMemcpyAsync(p.spatial_out, x, sizeof(float) * rows * C,
                                   hipMemcpyDeviceToDevice, s));
  }
  if (p.poison) {
    const long per_image = (long)h * w * C;
    const long total = (long)p.n * per_image;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(poison_fill_kernel, dim3(blocks), dim3(256), 0, s, p.spatial_out,
                       per_image, p.n, p.poison);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

static int encoder_run_batch(milan_ctx* c, const void* images, int image_dtype,
                             const void* masks, int mask_dtype, int n, int H,
                             int W, float* features, Arena& ws, hipStream_t s,
                             float* spatial_out) {
  const bool spatial = spatial_out != nullptr;
  MILAN_REQUIRE(c->d.trunk_kind != MILAN_TRUNK_ALEXNET_PLACES, MILAN_ERR_ARG,
                "the Places365 AlexNet trunk has no encoder config: it classifies, ablates and "
                "taps activations only");
  MILAN_REQUIRE(c->d.trunk_kind != MILAN_TRUNK_VGG, MILAN_ERR_ARG,
                "the VGG trunk has no encoder config: it classifies, ablates and taps "
                "activations only");
  MILAN_REQUIRE(!spatial || c->d.trunk_kind != MILAN_TRUNK_ALEXNET, MILAN_ERR_ARG,
                "spatial encoding needs a ResNet trunk");
  MILAN_REQUIRE(c->stem.w != nullptr, MILAN_ERR_STATE,
                "encoder weights were not uploaded");
  MILAN_REQUIRE(n > 0 && H >= 1 && W >= 1, MILAN_ERR_SHAPE,
                "encode: need n>0 and H,W>=1 (got n=%d H=%d W=%d)", n, H, W);
  if (c->d.trunk_kind == MILAN_TRUNK_ALEXNET) {
    // (image sharing covers the ResNet trunks: accepted and ignored here, slots == images)
    if (c->share_images && c->share_stats != nullptr)
      MILAN_TRY(launch_share_count(c->share_stats, n, nullptr, s));
    return alexnet_run_batch(c, images, image_dtype, masks, mask_dtype, n, H, W,
                             features, ws, s);
  }
  EncPass p{c, s, images, image_dtype, masks, mask_dtype, n, H, W, features, spatial_out};
  enc_carve(c->d.trunk_kind, c->d.trunk_width, n, H, W, &ws, &p.pl);
  MILAN_REQUIRE(ws.off <= ws.size, MILAN_ERR_WORKSPACE,
                "encode: workspace too small (%zu needed, %zu given)", ws.off,
                ws.size);
  EncAsk ask;
  MILAN_TRY(enc_ask(c, images, image_dtype, masks, mask_dtype, n, H, W, spatial, &ask));
  p.sc = plan_encoder(ask, p.pl);
  p.poison = image_dtype == MILAN_DTYPE_F32 ? p.pl.poison : nullptr;
  p.order = p.class_of = p.bbox = nullptr;

  MILAN_TRY(run_input(p));
  MILAN_TRY(run_stem(p));
  MILAN_TRY(run_tail_sets(p));
  // 4. the stages; tap after each stage
  for (int li = 0; li < 4; ++li) {
    {
      StageScope scope(MILAN_STAGE_ENC_LAYER1 + li, s);
      if (p.sc.fast && li == 2) {
        // the residual stream leaves the split format: f16(hi + lo) into the spare buffer
        const long groups = p.sc.f16_groups;
        const int nb = (int)((groups + 255) / 256 < 16384 ? (groups + 255) / 256 : 16384);
        hipLaunchKernelGGL(split_to_f16_kernel, dim3(nb), dim3(256), 0, s, p.sc.f16_src, groups,
                           p.pl.ds, p.sc.live, groups / n);
        MILAN_CHECK_HIP(hipGetLastError());
      }
      for (int k = p.sc.first[li]; k < p.sc.first[li + 1]; ++k)
        MILAN_TRY(run_block(p, p.sc.blocks[k]));
    }
    MILAN_REQUIRE(p.sc.h_out[li] == p.pl.lv.h[li + 1] && p.sc.w_out[li] == p.pl.lv.w[li + 1],
                  MILAN_ERR_SHAPE, "internal: stage %d geometry mismatch", li + 1);
    MILAN_TRY(run_pool(p, p.sc.out[li], li + 1));
  }
  if (spatial) MILAN_TRY(run_spatial_out(p));
  return 0;
}

// ---------------------------------------------------------------------------
// Pieces of the plain schedule that classify.hip drives on its own (milan_classify*): the
// input conversion without normalisation, the stem conv's arguments, the unfused stem tail
// and conv_args.  encoder_run_batch above does not call them.
// ---------------------------------------------------------------------------
int encoder_sub_batch_size() { return encoder_sub_batch(); }

GemmArgs encoder_conv_args(const ConvW& cw, const float* in, int n, int H, int W, float* out,
                           int epi, const float* aux, const float* zero, int* Ho, int* Wo,
                           bool split, bool scaled_bias) {
  return conv_args(cw, in, n, H, W, out, epi, aux, zero, Ho, Wo, split, scaled_bias);
}

// (n,3,H,W) float NCHW, taken as it is (mean 0, std 1: (v - 0) / 1 is v) -> NHWC4 fp32, or
// pixel-pair groups in split format for the pair stem
int launch_raw_input(const float* images, int n, int H, int W, bool pairs, float* out,
                     unsigned* status, hipStream_t s) {
  const int G = (W + 2) / 2;
  const long np = pairs ? (long)n * H * G : (long)n * H * W;
  const int blocks = (int)((np + 255) / 256 < 8192 ? (np + 255) / 256 : 8192);
  if (pairs)
    hipLaunchKernelGGL(preprocess_pairs_kernel<float>, dim3(blocks), dim3(256), 0, s, images, np,
                       H, W, G, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, out, nullptr, 1, nullptr, status);
  else
    hipLaunchKernelGGL(preprocess_kernel<float>, dim3(blocks), dim3(256), 0, s, images, np, H * W,
                       0.f, 0.f, 0.f, 1.f, 1.f, 1.f, (float4*)out, nullptr, 1, nullptr, nullptr);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// conv1 7x7/2 as encoder_run_batch's unfused stem launches it: raw fp32 output (n, h1, w1, width)
GemmArgs encoder_stem_args(const milan_ctx* c, const float* in4, int n, int H, int W, float* raw,
                           bool pair_stem) {
  return stem_args(c->stem, c->stem_pair, c->zero, in4, n, H, W, raw, pair_stem);
}

// bn1 + ReLU + maxpool 3x3/2 of the raw conv1 tensor -> fp32 or split format (activation scale)
int launch_stem_tail(const milan_ctx* c, const float* raw, int n, int h1, int w1, int hp, int wp,
                     bool split, float* y, hipStream_t s) {
  const int wd = c->d.trunk_width;
  const long total = (long)n * hp * wp * (wd / (split ? 8 : 4));
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  if (split)
    hipLaunchKernelGGL(bn_relu_maxpool_split_kernel, dim3(blocks), dim3(256), 0, s, raw, n, h1, w1,
                       wd, hp, wp, c->bn1_scale_s, c->bn1_shift_s, y, c->status, nullptr);
  else
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)raw, n,
                       h1, w1, wd / 4, hp, wp, (const float4*)c->bn1_scale,
                       (const float4*)c->bn1_shift, (float4*)y, nullptr);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// milan_set_act_scale_log2: the pre-multiplied copies of every folded bias / bn1 vector are
// rewritten in place for the new activation scale (exact: a power of two)
int encoder_rescale(milan_ctx* c, hipStream_t s) {
  auto redo = [&](const float* src, float* dst, int n) -> int {
    if (!src || !dst) return 0;
    hipLaunchKernelGGL(scale_vec_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src,
                       c->act_scale, n, dst);
    MILAN_CHECK_HIP(hipGetLastError());
    return 0;
  };
  if (c->stem.w) {
    MILAN_TRY(redo(c->bn1_scale, c->bn1_scale_s, c->stem.cout));
    MILAN_TRY(redo(c->bn1_shift, c->bn1_shift_s, c->stem.cout));
  }
  for (int li = 0; li < 4; ++li)
    for (Bottleneck& b : c->blocks[li])
      for (ConvW* w : {&b.c1, &b.c2, &b.c3, &b.down, &b.c3d})
        MILAN_TRY(redo(w->bias, w->bias_s, w->cout));
  return 0;
}

// ---------------------------------------------------------------------------
// 'alexnet' pyramid config (reference src/milan/encoders.py:330-335)
// ---------------------------------------------------------------------------
// Taps are torchvision's features.0/3/6/8/10, i.e. the five conv modules.
// nethook retains `output.detach()` (src/deps/netdissect/nethook.py:226-235),
// which shares storage with the conv output, and every AlexNet conv is followed
// by nn.ReLU(inplace=True): what the encoder pools is relu(conv + bias) (pinned
// by golden G11).  So each conv runs with the bias+ReLU epilogue and its output
// is both the tap and the next layer's (max-pooled) input.

// 3x3 / stride 2 max-pool over NHWC, `pad` pixels of implicit -inf padding.
__global__ void maxpool3s2_f32_kernel(const float4* __restrict__ x, int n, int H,
                                      int W, int C4, int Ho, int Wo, int pad,
                                      float4* __restrict__ y) {
  const long total = (long)n * Ho * Wo * C4;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int cc = idx % C4;
    long t = idx / C4;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const long img = t / Ho;
    float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = 0; dy < 3; ++dy) {
      const int hi = ho * 2 - pad + dy;
      if (hi < 0 || hi >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int wi = wo * 2 - pad + dx;
        if (wi < 0 || wi >= W) continue;
        const float4 v = x[((img * H + hi) * W + wi) * C4 + cc];
        best.x = fmaxf(best.x, v.x); best.y = fmaxf(best.y, v.y);
        best.z = fmaxf(best.z, v.z); best.w = fmaxf(best.w, v.w);
      }
    }
    y[idx] = best;
  }
}

// Same, 8 channels per thread, split-format output; input fp32 or split.
template <bool IN_SPLIT>
__global__ void maxpool3s2_split_kernel(const float* __restrict__ x, int n, int H,
                                        int W, int C, int Ho, int Wo, int pad,
                                        float* __restrict__ y,
                                        unsigned* __restrict__ status) {
  const int C8 = C >> 3;
  const long total = (long)n * Ho * Wo * C8;
  float sat = 0.f;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int c8 = idx % C8;
    long t = idx / C8;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const long img = t / Ho;
    float best[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) best[e] = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
      const int hi = ho * 2 - pad + dy;
      if (hi < 0 || hi >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int wi = wo * 2 - pad + dx;
        if (wi < 0 || wi >= W) continue;
        const float* p = x + ((img * H + hi) * W + wi) * C + c8 * 8;
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p + 4);
        float v[8];
        if constexpr (IN_SPLIT) {
          const f16x8_t hh = __builtin_bit_cast(f16x8_t, a);
          const f16x8_t ll = __builtin_bit_cast(f16x8_t, b);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = (float)hh[e] + (float)ll[e];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) best[e] = fmaxf(best[e], v[e]);
      }
    }
    f32x4_t hi4, lo4;
    enc_split8(best, &hi4, &lo4, &sat);
    float* d = y + idx * 8;
    *reinterpret_cast<f32x4_t*>(d) = hi4;
    *reinterpret_cast<f32x4_t*>(d + 4) = lo4;
  }
  report_saturation(status, sat);
}

// The trunk's 3x3 / stride 2 max-pool without padding (pool1, pool2), for alexnet_run_batch
// below and for classify.hip's AlexNet walk: fp32 -> fp32, or with `split` fp32 / split
// (`in_split`) -> split at scale 1; saturation is reported in `status`
int launch_maxpool3s2(const float* x, int n, int H, int W, int C, int Ho, int Wo, bool split,
                      bool in_split, float* y, unsigned* status, hipStream_t s) {
  const long total = (long)n * Ho * Wo * (C / (split ? 8 : 4));
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  if (!split)
    hipLaunchKernelGGL(maxpool3s2_f32_kernel, dim3(blocks), dim3(256), 0, s, (const float4*)x, n,
                       H, W, C / 4, Ho, Wo, 0, (float4*)y);
  else if (in_split)
    hipLaunchKernelGGL(maxpool3s2_split_kernel<true>, dim3(blocks), dim3(256), 0, s, x, n, H, W,
                       C, Ho, Wo, 0, y, status);
  else
    hipLaunchKernelGGL(maxpool3s2_split_kernel<false>, dim3(blocks), dim3(256), 0, s, x, n, H, W,
                       C, Ho, Wo, 0, y, status);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

struct AlexPlan {
  Levels lv;
  int hq[3], wq[3];        // max-pooled sizes after conv1 / conv2 (/ conv5: not used here)
  int C[5];
  float *in4, *a[5], *q[2];
  int *list_idx, *list_n;
  float* list_w;
};

static void alexnet_plan(const milan_ctx* c, int n, int H, int W, Arena& ar,
                         AlexPlan* pl) {
  Levels& lv = pl->lv;
  alex_geometry(c, H, W, lv.h, lv.w, pl->hq, pl->wq);
  long off = 0;
  for (int l = 0; l < 5; ++l) { lv.off[l] = off; off += (long)lv.h[l] * lv.w[l]; }
  lv.per_image = off;
  for (int l = 0; l < 5; ++l) pl->C[l] = c->alex[l].cout;
  pl->in4 = ar.get<float>((size_t)n * H * W * 4);
  for (int l = 0; l < 5; ++l)
    pl->a[l] = ar.get<float>((size_t)n * lv.h[l] * lv.w[l] * pl->C[l]);
  for (int l = 0; l < 2; ++l)
    pl->q[l] = ar.get<float>((size_t)n * pl->hq[l] * pl->wq[l] * pl->C[l]);
  pl->list_idx = ar.get<int>((size_t)n * lv.per_image);
  pl->list_w = ar.get<float>((size_t)n * lv.per_image);
  pl->list_n = ar.get<int>((size_t)n * 5);
}

static void alexnet_workspace_dry(const milan_ctx* c, int n, int H, int W,
                                  Arena& a) {
  AlexPlan pl;
  alexnet_plan(c, n, H, W, a, &pl);
}

static int alexnet_run_batch(milan_ctx* c, const void* images, int image_dtype,
                             const void* masks, int mask_dtype, int n, int H,
                             int W, float* features, Arena& ws, hipStream_t s) {
  AlexPlan pl;
  alexnet_plan(c, n, H, W, ws, &pl);
  MILAN_REQUIRE(ws.off <= ws.size, MILAN_ERR_WORKSPACE,
                "encode: workspace too small (%zu needed, %zu given)", ws.off,
                ws.size);
  MILAN_REQUIRE(pl.hq[1] >= 1 && pl.wq[1] >= 1, MILAN_ERR_SHAPE, "encode: image %dx%d unsupported by the alexnet "
                "pyramid", H, W);
  const int F = c->d.feature_size;
  if (masks == nullptr || mask_dtype == MILAN_DTYPE_U8)
    hipLaunchKernelGGL(mask_pyramid_kernel<uint8_t>, dim3(n, 5), dim3(256), 0, s,
                       (const uint8_t*)masks, H, W, pl.lv, pl.list_idx,
                       pl.list_w, pl.list_n);
  else
    hipLaunchKernelGGL(mask_pyramid_kernel<float>, dim3(n, 5), dim3(256), 0, s,
                       (const float*)masks, H, W, pl.lv, pl.list_idx, pl.list_w,
                       pl.list_n);
  {
    const long np = (long)n * H * W;
    const int blocks = (int)((np + 255) / 256 < 8192 ? (np + 255) / 256 : 8192);
    if (image_dtype == MILAN_DTYPE_U8)
      hipLaunchKernelGGL(preprocess_kernel<uint8_t>, dim3(blocks), dim3(256), 0,
                         s, (const uint8_t*)images, np, H * W, c->mean[0],
                         c->mean[1], c->mean[2], c->stdv[0], c->stdv[1],
                         c->stdv[2], (float4*)pl.in4);
    else
      hipLaunchKernelGGL(preprocess_kernel<float>, dim3(blocks), dim3(256), 0, s,
                         (const float*)images, np, H * W, c->mean[0], c->mean[1],
                         c->mean[2], c->stdv[0], c->stdv[1], c->stdv[2],
                         (float4*)pl.in4);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  // split-f16 mode from conv2 on (conv1 has Cin = 3: fp32 kernel, fp32 tap)
  bool split = c->precision == MILAN_PRECISION_SPLIT_F16;
  for (int l = 0; l < 5; ++l)
    split = split && pl.C[l] % 8 == 0 && (l == 0 || c->alex[l].ws != nullptr);

  int col = 0;
  auto pool = [&](int l, bool tap_split) -> int {
    const int P = pl.lv.h[l] * pl.lv.w[l], C = pl.C[l];
    if (tap_split)
      hipLaunchKernelGGL(masked_pool_kernel<1>, dim3(n, (C + 63) / 64),
                         dim3(256), 0, s, pl.a[l], P, C, l, pl.lv, pl.list_idx,
                         pl.list_w, pl.list_n, features, F, col, 0, 1.f);
    else
      hipLaunchKernelGGL(masked_pool_kernel<0>, dim3(n, (C + 63) / 64),
                         dim3(256), 0, s, pl.a[l], P, C, l, pl.lv, pl.list_idx,
                         pl.list_w, pl.list_n, features, F, col, 0, 1.f);
    MILAN_CHECK_HIP(hipGetLastError());
    col += C;
    return 0;
  };

  int ho, wo;
  GemmArgs g0 = conv_args(c->alex[0], pl.in4, n, H, W, pl.a[0], EPI_BIAS_RELU,
                          nullptr, c->zero, &ho, &wo);
  MILAN_TRY(launch_gemm(g0, s));
  MILAN_TRY(pool(0, false));
  // (pool1 reads conv1's fp32 output; both pools write the format the next conv reads)
  MILAN_TRY(launch_maxpool3s2(pl.a[0], n, pl.lv.h[0], pl.lv.w[0], pl.C[0], pl.hq[0], pl.wq[0],
                              split, false, pl.q[0], c->status, s));
  const float* in = pl.q[0];
  int h = pl.hq[0], w = pl.wq[0];
  for (int l = 1; l < 5; ++l) {
    // (the AlexNet path keeps activation scale 1: its taps are pooled as stored; ho x wo is
    // the plan's extent of the level: alex_geometry reads the same ConvW)
    GemmArgs g = conv_args(c->alex[l], in, n, h, w, pl.a[l], EPI_BIAS_RELU,
                           nullptr, c->zero, &ho, &wo, split, false);
    MILAN_TRY(launch_gemm(g, s));
    MILAN_TRY(pool(l, split));
    in = pl.a[l];
    h = ho; w = wo;
    if (l == 1) {
      MILAN_TRY(launch_maxpool3s2(pl.a[1], n, pl.lv.h[1], pl.lv.w[1], pl.C[1], pl.hq[1],
                                  pl.wq[1], split, split, pl.q[1], c->status, s));
      in = pl.q[1];
      h = pl.hq[1]; w = pl.wq[1];
    }
  }
  return 0;
}

}  // namespace milan
