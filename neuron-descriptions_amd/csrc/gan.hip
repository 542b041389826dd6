// The non-local (SAGAN) attention block of a BigGAN generator, between its 1 x 1 convs:
//   beta = softmax_j(theta_i . phi_j)   (no scale factor),   out_i = sum_j beta_ij g_j
// for an image of H x W pixels with C channels: theta (H W, C / 8) are the queries, phi
// (H W / 4, C / 8) and g (H W / 4, C / 2) the 2 x 2 max-pooled keys and values.  At BigGAN-256
// (128 x 128, C = 192) that is 16 384 queries against 4 096 keys per image: the scores, 268 MB
// of fp32 per image, never exist here.
//
// sagan_attention_kernel follows vit::attention_kernel: a workgroup of four
// waves owns 128 query rows of one image, 32 per wave, and streams the keys through LDS 32 at a
// time under an online softmax in base 2; both products are v_mfma_f32_32x32x2_f32, transposed
// so that no operand moves between lanes:
//   S^T = phi theta^T  A = phi tile (row = key), B = theta^T (column = query): the query sits
//                      on the lane, the 32 keys in 16 registers x 2 lane halves.
//   O^T = g^T P^T      A = g^T (row = value column d), B = P^T = the S^T accumulator as it
//                      stands: register r of lane half h is key (r & 3) + 8 (r >> 2) + 4 h.
// What differs from the ViT's kernel:
//   * dk = C / 8 (the reduction width of S) is not dv = C / 2 (the row count of O^T): the
//     kernel is instantiated per K = C / 32, dk = 4 K, dv = 16 K.
//   * dk is a multiple of 4 only.  Lane half h takes columns 4 s + 2 h, 4 s + 2 h + 1 of each
//     group of four (one 8-byte LDS read per two MFMAs) instead of one contiguous half, so no
//     width needs padding; phi rows lie dk + 2 floats apart, an odd multiple of 2, which puts
//     the 32 keys of a ds_read_b64 lane group on 32 distinct even banks of the 64.
//   * phi and g arrive as one row, phi | g, as the pooled output of a fused theta | phi | g
//     conv: a tile of 32 keys is one contiguous run of 32 (dk + dv) floats.
//   * O^T is ceil(dv / 32) accumulator blocks per wave, 3 at C = 192 and 6 at C = 384, all in
//     one wave.  The compiler reports 148 VGPRs + 48 AGPRs at C = 192 (two waves per SIMD,
//     15 616 bytes of LDS) and 244 + 96 at C = 384 (one wave per SIMD, 30 976 bytes), no spill
//     at any width.  Splitting dv over workgroups would compute S and the softmax once per
//     split to buy occupancy that an MFMA-bound loop (48 of its 60 MFMAs per tile at C = 192
//     are the P V product) does not need, so it is not done.
//
// Precision: exact fp32; the weights are v_exp_f32 of an exponent formed by two FMAs with
// log2(e) split hi + lo.  Determinism: fixed orders, no atomics; the bits of one image depend
// on nothing else in the launch.
//
// The generator walk (milan_gan_*) is described above its code, further down.
#include "tower_common.h"

#include <math.h>
#include <algorithm>

namespace milan {
namespace gan {
struct BnDesc;
}
}

struct milan_gan_ctx {
  milan_gan_dims d{};
  milan::tower::Weights w;
  struct Bn {
    const float *gain_w = nullptr, *bias_w = nullptr, *mean = nullptr, *var = nullptr;
    int off = 0;  // first column in the folded scale / shift arrays
  };
  struct Block {
    int cin = 0, cout = 0, side = 0;  // side: of the block's input
    const float *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr,
                *sc_w = nullptr, *sc_b = nullptr;
    Bn bn1, bn2;
    bool attn = false;
    const float *theta = nullptr, *phi = nullptr, *g = nullptr, *o = nullptr, *gamma = nullptr;
    // packed [N][Kp] for launch_gemm: conv1, conv2, conv_sc, theta | phi | g, gamma * o
    float *p1 = nullptr, *p2 = nullptr, *psc = nullptr, *ptpg = nullptr, *po = nullptr;
  };
  std::vector<Block> blocks;
  const float *shared = nullptr, *linear_w = nullptr, *linear_b = nullptr, *out_w = nullptr,
              *out_b = nullptr;
  Bn out_bn;
  int chunk = 0, z_in = 0, bn_total = 0, bn_count = 0, bn_max_c = 0;
  // owned: the packed weights, the BnDesc table, 64 zero floats, the padded output conv
  float* packed = nullptr;
  milan::gan::BnDesc* descs = nullptr;
  float *zero = nullptr, *pout = nullptr, *out_b4 = nullptr;
};

namespace milan {
namespace gan {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int SA_THREADS = 256;
constexpr int SA_BM = 128;  // query rows per workgroup (32 per wave)
constexpr int SA_BN = 32;   // keys per LDS tile
constexpr int SA_MAX_K = 12;  // C = 384

__host__ __device__ constexpr int ldk_of(int dk) { return dk + 2; }
static size_t sa_lds_bytes(int dk, int dv) {
  return sizeof(float) * (size_t)SA_BN * (ldk_of(dk) + dv);
}

// theta: query row i of image b at theta + (b * Tq + i) * ldq, dk floats.
// phig: [n][Tk][dk + dv] (phi | g).  out: [n][Tq][dv].  grid.x = n * ceil(Tq / SA_BM).
template <int KQ>
__global__ __launch_bounds__(SA_THREADS) void sagan_attention_kernel(
    const float* __restrict__ theta, long ldq, const float* __restrict__ phig,
    float* __restrict__ out, int Tq, int Tk, int qtiles, float c_hi, float c_lo) {
  constexpr int DK = 4 * KQ, DV = 16 * KQ, ROW = DK + DV;
  constexpr int HALF = DK / 2;        // k-steps of S^T, two per group of four columns
  constexpr int ND = (DV + 31) / 32;  // 32-row blocks of O^T
  constexpr int LDK = ldk_of(DK), LDV = DV;
  constexpr int F4 = SA_BN * ROW / 4;                      // float4 per tile of keys
  constexpr int PER = (F4 + SA_THREADS - 1) / SA_THREADS;  // of them per thread
  extern __shared__ __align__(16) float lds[];
  float* Ks = lds;
  float* Vs = lds + SA_BN * LDK;  // 32 (dk + 2) floats: a multiple of 16 bytes

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int img = blockIdx.x / qtiles, qt = blockIdx.x % qtiles;
  const float* kv_base = phig + (size_t)img * Tk * ROW;
  const int q0 = qt * SA_BM + w * 32;  // first query row of this wave
  const int query = q0 + l31;
  const bool wave_on = q0 < Tq;        // a wave wholly past Tq only helps with the tiles

  // theta^T operand: lane (query, h) keeps theta[query][4 s + 2 h + {0, 1}], s < DK / 4
  float qreg[HALF];
  {
    const float* qp = theta + ((size_t)img * Tq + (query < Tq ? query : 0)) * ldq + 2 * h;
#pragma unroll
    for (int s = 0; s < HALF; s += 2) {
      float2 v = make_float2(0.f, 0.f);
      if (query < Tq) v = *reinterpret_cast<const float2*>(qp + 2 * s);
      qreg[s] = v.x; qreg[s + 1] = v.y;
    }
  }

  v16f acc[ND];
#pragma unroll
  for (int b = 0; b < ND; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // the next tile's global loads are in flight while this one's MFMAs run.  Float4 i of a tile
  // is floats 4 i .. 4 i + 3 of its contiguous run; DK % 4 == 0 keeps it inside phi or inside g.
  float4 rkv[PER];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = tid + u * SA_THREADS;
      rkv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < F4 && j0 + i / (ROW / 4) < Tk)
        rkv[u] = *reinterpret_cast<const float4*>(kv_base + (size_t)j0 * ROW + (size_t)i * 4);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = tid + u * SA_THREADS;
      const int key = i / (ROW / 4), c = (i % (ROW / 4)) * 4;
      if (i < F4) {
        if (c < DK) {  // phi rows are 8-byte aligned only
          float* p = Ks + key * LDK + c;
          *reinterpret_cast<float2*>(p) = make_float2(rkv[u].x, rkv[u].y);
          *reinterpret_cast<float2*>(p + 2) = make_float2(rkv[u].z, rkv[u].w);
        } else {
          *reinterpret_cast<float4*>(Vs + key * LDV + (c - DK)) = rkv[u];
        }
      }
    }
  };

  fetch(0);
  for (int j0 = 0; j0 < Tk; j0 += SA_BN) {
    stash();
    __syncthreads();
    if (j0 + SA_BN < Tk) fetch(j0 + SA_BN);
    if (wave_on) {
      // S^T[key][query]: MFMA k-index h of step (s, e) is column 4 s + 2 h + e
      v16f st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      const float* kp = Ks + l31 * LDK + 2 * h;
#pragma unroll
      for (int s = 0; s < HALF; s += 2) {
        const float2 kv = *reinterpret_cast<const float2*>(kp + 2 * s);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qreg[s], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qreg[s + 1], st, 0, 0, 0);
      }
      // register r of lane half h is key j0 + (r & 3) + 8 (r >> 2) + 4 h.  Weights in base 2:
      // exp(s - m) = exp2(s c - m2), c = log2(e) = c_hi + c_lo.  m2 is the running max of the
      // rounded s c_hi; the exponent itself is two FMAs on the unrounded product.  A key past
      // Tk gets weight 0 by selection (key j0 is always real, so the max is finite).
      const bool partial = j0 + SA_BN > Tk;
      if (partial) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (j0 + (r & 3) + 8 * (r >> 2) + 4 * h >= Tk) st[r] = -INFINITY;
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[r] * c_hi);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x = fmaf(st[r], c_lo, fmaf(st[r], c_hi, -m_new));
        float p = __builtin_amdgcn_exp2f(x);
        if (partial && j0 + (r & 3) + 8 * (r >> 2) + 4 * h >= Tk) p = 0.f;
        st[r] = p;
        sum += p;
      }
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
#pragma unroll
      for (int b = 0; b < ND; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] *= alpha;
      // O^T[d][query] += g[key][d] P^T[key][query]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vp = Vs + ((r & 3) + 8 * (r >> 2) + 4 * h) * LDV + l31;
#pragma unroll
        for (int b = 0; b < ND; ++b) {
          float vv = 0.f;
          if (DV % 32 == 0 || b * 32 + l31 < DV) vv = vp[b * 32];
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[r], acc[b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (!wave_on || query >= Tq) return;
  // O^T accumulator: column = query (this lane), row d = 32 b + 8 g + 4 h + (r & 3), r = 4 g + ..
  float* op = out + ((size_t)img * Tq + query) * DV;
#pragma unroll
  for (int b = 0; b < ND; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = b * 32 + 8 * g + 4 * h;
      if (DV % 32 != 0 && d0 >= DV) continue;
      float4 v;
      v.x = acc[b][4 * g] / l_run;
      v.y = acc[b][4 * g + 1] / l_run;
      v.z = acc[b][4 * g + 2] / l_run;
      v.w = acc[b][4 * g + 3] / l_run;
      *reinterpret_cast<float4*>(op + d0) = v;
    }
}

template <int KQ>
static int launch_sa(const float* theta, long ldq, const float* phig, float* out, long n, int Tq,
                     int Tk, hipStream_t s) {
  const int qtiles = (Tq + SA_BM - 1) / SA_BM;
  const size_t lds = sa_lds_bytes(4 * KQ, 16 * KQ);
  MILAN_TRY(ensure_lds_attr((const void*)sagan_attention_kernel<KQ>, (int)lds));
  const double c = 1.4426950408889634;  // log2(e)
  const float c_hi = (float)c, c_lo = (float)(c - (double)c_hi);
  hipLaunchKernelGGL(sagan_attention_kernel<KQ>, dim3((unsigned)(n * qtiles)), dim3(SA_THREADS),
                     lds, s, theta, ldq, phig, out, Tq, Tk, qtiles, c_hi, c_lo);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int launch_sagan_attention(const float* theta, long ldq, const float* phig, float* out,
                                  long n, int H, int W, int C, hipStream_t s) {
  MILAN_REQUIRE(n >= 0, MILAN_ERR_SHAPE, "sagan_attention: %ld images", n);
  MILAN_REQUIRE(C >= 32 && C % 32 == 0 && C <= 32 * SA_MAX_K, MILAN_ERR_SHAPE,
                "sagan_attention: channels %d (dk = channels / 8, dv = channels / 2) must be a "
                "multiple of 32 from 32 to %d", C, 32 * SA_MAX_K);
  MILAN_REQUIRE(H >= 2 && H % 2 == 0 && H <= 32768, MILAN_ERR_SHAPE,
                "sagan_attention: height %d must be even (the keys are 2 x 2 max-pooled) and at "
                "most 32768", H);
  MILAN_REQUIRE(W >= 2 && W % 2 == 0 && W <= 32768, MILAN_ERR_SHAPE,
                "sagan_attention: width %d must be even (the keys are 2 x 2 max-pooled) and at "
                "most 32768", W);
  const int dk = C / 8;
  MILAN_REQUIRE(ldq >= dk && ldq % 2 == 0, MILAN_ERR_SHAPE,
                "sagan_attention: theta_stride %ld must be even and at least dk = %d", ldq, dk);
  const int Tq = H * W, Tk = Tq / 4;
  const long qtiles = (Tq + SA_BM - 1) / SA_BM;
  MILAN_REQUIRE(n * qtiles < (1L << 31), MILAN_ERR_SHAPE,
                "sagan_attention: %ld images x %ld query tiles exceed the launch grid", n, qtiles);
  if (n == 0) return 0;
  switch (C / 32) {
    case 1: return launch_sa<1>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 2: return launch_sa<2>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 3: return launch_sa<3>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 4: return launch_sa<4>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 5: return launch_sa<5>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 6: return launch_sa<6>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 7: return launch_sa<7>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 8: return launch_sa<8>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 9: return launch_sa<9>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 10: return launch_sa<10>(theta, ldq, phig, out, n, Tq, Tk, s);
    case 11: return launch_sa<11>(theta, ldq, phig, out, n, Tq, Tk, s);
    default: return launch_sa<12>(theta, ldq, phig, out, n, Tq, Tk, s);
  }
}


// ---- the generator walk -------------------------------------------------------------------------
// Channel multipliers (in, out) of the GBlocks per output resolution (appendix B of the BigGAN
// paper); block i takes side bottom_width * 2^i to twice that and is "at resolution" 8 << i.
struct Arch {
  int resolution, blocks;
  int in[7], out[7];
};
static const Arch ARCHS[] = {
    {512, 7, {16, 16, 8, 8, 4, 2, 1}, {16, 8, 8, 4, 2, 1, 1}},
    {256, 6, {16, 16, 8, 8, 4, 2}, {16, 8, 8, 4, 2, 1}},
    {128, 5, {16, 16, 8, 4, 2}, {16, 8, 4, 2, 1}},
    {64, 4, {16, 16, 8, 4}, {16, 8, 4, 2}},
    {32, 3, {4, 4, 4}, {4, 4, 4}},
};
static const Arch* arch_of(int resolution) {
  for (const Arch& a : ARCHS)
    if (a.resolution == resolution) return &a;
  return nullptr;
}

// One batch norm of the network for fold_bn_kernel.  Conditional (slot >= -1): gain_w / bias_w
// are (C, cond) matrices, cond = shared_dim + chunk, and the condition of sample b is
// y[b] | z[b][slot * chunk ..] (slot -1: y alone).  Plain (slot == -2, the output layer's):
// gain_w / bias_w are the C-vectors gain and bias.
struct BnDesc {
  const float *gain_w, *bias_w, *mean, *var;
  int C, slot, off;  // off: first column of this norm in the (n, total) scale / shift arrays
  float eps;
};

// y (n, S) = shared[classes[b]]  or  soft[b] (n_classes) @ shared (n_classes, S)
__global__ void embed_kernel(const float* __restrict__ shared, const int64_t* __restrict__ classes,
                             const float* __restrict__ soft, float* __restrict__ y, int n, int S,
                             int n_classes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * S) return;
  const int b = i / S, d = i - b * S;
  if (classes) {
    int64_t c = classes[b];
    c = c < 0 ? 0 : (c >= n_classes ? n_classes - 1 : c);  // (the binding refuses these)
    y[i] = shared[c * S + d];
    return;
  }
  float acc = 0.f;
  for (int c = 0; c < n_classes; ++c) acc = fmaf(soft[(size_t)b * n_classes + c], shared[(size_t)c * S + d], acc);
  y[i] = acc;
}

// Every batch norm of the walk folded to x * scale + shift per (sample, channel):
// scale = (1 + gain(cond)) / sqrt(var + eps), shift = bias(cond) - mean * scale.  One thread per
// (norm, sample, channel) walks its two weight rows in order.  grid (ceil(maxC / 128), norms, n).
__global__ __launch_bounds__(128) void fold_bn_kernel(const BnDesc* __restrict__ descs,
                                                      const float* __restrict__ y,
                                                      const float* __restrict__ z, int S, int chunk,
                                                      int dim_z, int total,
                                                      float* __restrict__ scale,
                                                      float* __restrict__ shift) {
  const BnDesc d = descs[blockIdx.y];
  const int c = blockIdx.x * 128 + threadIdx.x, b = blockIdx.z;
  if (c >= d.C) return;
  float gain, bias;
  if (d.slot == -2) {
    gain = d.gain_w[c];
    bias = d.bias_w[c];
  } else {
    const int cond = S + (d.slot >= 0 ? chunk : 0);
    const float* gw = d.gain_w + (size_t)c * cond;
    const float* bw = d.bias_w + (size_t)c * cond;
    const float* yb = y + (size_t)b * S;
    float g = 0.f, t = 0.f;
    for (int k = 0; k < S; ++k) {
      g = fmaf(yb[k], gw[k], g);
      t = fmaf(yb[k], bw[k], t);
    }
    if (d.slot >= 0) {
      const float* zb = z + (size_t)b * dim_z + (size_t)d.slot * chunk;
      for (int k = 0; k < chunk; ++k) {
        g = fmaf(zb[k], gw[S + k], g);
        t = fmaf(zb[k], bw[S + k], t);
      }
    }
    gain = 1.f + g;
    bias = t;
  }
  const float sc = gain / sqrtf(d.var[c] + d.eps);
  const size_t o = (size_t)b * total + d.off + c;
  scale[o] = sc;
  shift[o] = bias - d.mean[c] * sc;
}

// h (n, P, C) pixel-major = z0 W^T + bias with W (C * P, K) as torch stores it (row c * P + p):
// the model's view(n, C, bw, bw) read NHWC.  One thread per output.
__global__ void first_linear_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ w,
                                    const float* __restrict__ bias, float* __restrict__ h, long total,
                                    int P, int C, int K) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long r = i / C;
  const int p = (int)(r % P);
  const long b = r / P;
  const size_t row = (size_t)c * P + p;
  const float* wr = w + row * K;
  const float* zb = z + b * ldz;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(zb[k], wr[k], acc);
  h[i] = acc + bias[row];
}

// ccbn_relu_up2_kernel: y = relu(x * scale[b][c] + shift[b][c]) (AFFINE) or y = x, written once
// (UP = false) or to the four pixels of its nearest-neighbour 2 x upsampling (UP = true: one
// pixel read, four written).  x (n, H, W, C) NHWC, C % 4 == 0; one thread per (pixel, 4
// channels).  scale / shift: sample stride ss_stride, already offset to this norm's columns.
// Without UP, y may be x.
template <bool UP, bool AFFINE>
__global__ void ccbn_relu_up2_kernel(const float* x, const float* __restrict__ scale,
                                     const float* __restrict__ shift, long ss_stride, float* y,
                                     long total4, int H, int W, int C) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c4 = C / 4;
  const int c = (int)(i % c4) * 4;
  const long pix = i / c4;
  const int wx = (int)(pix % W);
  const long r = pix / W;
  const int hy = (int)(r % H);
  const long b = r / H;
  float4 v = *reinterpret_cast<const float4*>(x + pix * C + c);
  if (AFFINE) {
    const float4 sc = *reinterpret_cast<const float4*>(scale + b * ss_stride + c);
    const float4 sh = *reinterpret_cast<const float4*>(shift + b * ss_stride + c);
    v.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f);
    v.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
    v.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f);
    v.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
  }
  if (UP) {
    float* o = y + (((size_t)b * 2 * H + 2 * hy) * 2 * W + 2 * wx) * C + c;
    const size_t down = (size_t)2 * W * C;
    *reinterpret_cast<float4*>(o) = v;
    *reinterpret_cast<float4*>(o + C) = v;
    *reinterpret_cast<float4*>(o + down) = v;
    *reinterpret_cast<float4*>(o + down + C) = v;
  } else {
    *reinterpret_cast<float4*>(y + pix * C + c) = v;
  }
}

// 2 x 2 max-pool of columns [col0, col0 + Cp) of f (n, H, W, ld) into pg (n, H / 2, W / 2, Cp).
__global__ void pool_phi_g_kernel(const float* __restrict__ f, int ld, int col0,
                                  float* __restrict__ pg, long total4, int H, int W, int Cp) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int c4 = Cp / 4;
  const int c = (int)(i % c4) * 4;
  const long pix = i / c4;
  const int W2 = W / 2, H2 = H / 2;
  const int wx = (int)(pix % W2);
  const long r = pix / W2;
  const int hy = (int)(r % H2);
  const long b = r / H2;
  const float* p = f + (((size_t)b * H + 2 * hy) * W + 2 * wx) * ld + col0 + c;
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 bb = *reinterpret_cast<const float4*>(p + ld);
  const float4 cc = *reinterpret_cast<const float4*>(p + (size_t)W * ld);
  const float4 dd = *reinterpret_cast<const float4*>(p + (size_t)W * ld + ld);
  float4 m;
  m.x = fmaxf(fmaxf(a.x, bb.x), fmaxf(cc.x, dd.x));
  m.y = fmaxf(fmaxf(a.y, bb.y), fmaxf(cc.y, dd.y));
  m.z = fmaxf(fmaxf(a.z, bb.z), fmaxf(cc.z, dd.z));
  m.w = fmaxf(fmaxf(a.w, bb.w), fmaxf(cc.w, dd.w));
  *reinterpret_cast<float4*>(pg + pix * Cp + c) = m;
}

// A tap: columns [0, C) of x (n, P, ld) pixel-major -> (n, C, P), through a 64-pixel x 32-channel
// LDS tile so that both the reads (along c) and the writes (along p) are contiguous.
// grid (ceil(P / 64), ceil(C / 32), n).
__global__ __launch_bounds__(256) void nchw_kernel(const float* __restrict__ x, int P, int ld,
                                                   int C, float* __restrict__ out) {
  __shared__ float tile[64 * 33];
  const int t = threadIdx.x;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 32;
  const size_t img = blockIdx.z;
  const float* src = x + img * (size_t)P * ld;
  for (int i = t; i < 64 * 32; i += 256) {
    const int p = i >> 5, c = i & 31;
    if (p0 + p < P && c0 + c < C) tile[p * 33 + c] = src[(size_t)(p0 + p) * ld + c0 + c];
  }
  __syncthreads();
  float* dst = out + img * (size_t)C * P;
  for (int i = t; i < 64 * 32; i += 256) {
    const int c = i >> 6, p = i & 63;
    if (p0 + p < P && c0 + c < C) dst[(size_t)(c0 + c) * P + p0 + p] = tile[p * 33 + c];
  }
}

__global__ void scale_by_kernel(float* __restrict__ w, long total, const float* __restrict__ factor) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < total) w[i] *= factor[0];
}

static inline unsigned grid_for(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
static inline size_t up64(size_t v) { return (v + 63) / 64 * 64; }
static inline int kp_of(int k, int cin) { return (k * k * cin + 31) / 32 * 32; }

// out (n, H, W, cout; row stride ldc) = epi(conv k x k, stride 1, pad k / 2, of in (n, H, W, cin;
// pixel stride pix) with the packed weight wp), on the exact-fp32 implicit-GEMM tile.
static int conv(const float* in, long n, int H, int W, int cin, long pix, const float* wp,
                const float* bias, int cout, int k, int epi, const float* aux, int ldaux,
                float* out, int ldc, const float* zero, hipStream_t s) {
  GemmArgs g{};
  g.A = in; g.W = wp; g.bias = bias; g.aux = aux; g.C = out;
  g.M = (int)(n * H * W); g.N = cout; g.K = k * k * cin; g.Kp = kp_of(k, cin);
  g.ldc = ldc; g.ldaux = ldaux;
  g.H = H; g.Wd = W; g.Cin = cin; g.Ho = H; g.Wo = W; g.KH = k; g.KW = k;
  g.stride = 1; g.pad = k / 2; g.a_pix_stride = pix; g.a_img_stride = (long)H * W * pix;
  g.epilogue = epi; g.zero = zero;
  return launch_gemm(g, s);
}


// Workspace of a walk over n samples, in floats, 64-float aligned:
//   y      the embedded classes (n, shared_dim)
//   scale, shift   every batch norm folded, (n, bn_total) each
//   x0, x1 the ping-pong of block inputs / outputs: the largest h of the walk
//   t      a block's upsampled, normalised input (n, 2s, 2s, cin), then its upsampled
//          shortcut (n, 2s, 2s, cout); the attention's theta | phi | g (n, H W, 3 C / 4); the
//          output layer's normalised input
//   u      conv1's output (n, 2s, 2s, cout); the attention's pooled phi | g and its output;
//          the images as 4-column pixels
//   sc     the 1 x 1 shortcut conv at the block's input side (n, s, s, cout)
struct Plan {
  size_t y, scale, shift, x0, x1, t, u, sc, total_floats;
};
constexpr int MAX_GRID_Z = 65535;

static int plan(const milan_gan_ctx* c, int n, Plan* p) {
  MILAN_REQUIRE(c && c->w.finalized, MILAN_ERR_STATE, "gan: weights are not finalized");
  MILAN_REQUIRE(n > 0, MILAN_ERR_ARG, "gan: %d samples", n);
  // fold_bn_kernel and nchw_kernel put the sample in gridDim.z
  MILAN_REQUIRE(n <= MAX_GRID_Z, MILAN_ERR_ARG,
                "gan: %d samples exceed the %d that a launch grid's z takes: split the batch", n,
                MAX_GRID_Z);
  const auto& d = c->d;
  size_t x = 0, t = 0, u = 0, sc = 0;
  for (const auto& b : c->blocks) {
    const size_t in = (size_t)b.side * b.side, out = 4 * in;
    x = std::max({x, in * b.cin, out * b.cout});
    t = std::max(t, out * b.cin);
    u = std::max(u, out * b.cout);
    sc = std::max(sc, in * b.cout);
  }
  MILAN_REQUIRE((double)n * (double)std::max(t, x) < 2147483648.0, MILAN_ERR_ARG,
                "gan: %d samples x %zu floats exceed the 2^31-element GEMM range: split the "
                "batch", n, std::max(t, x));
  size_t o = 0;
  p->y = o; o += up64((size_t)n * d.shared_dim);
  p->scale = o; o += up64((size_t)n * c->bn_total);
  p->shift = o; o += up64((size_t)n * c->bn_total);
  p->x0 = o; o += up64((size_t)n * x);
  p->x1 = o; o += up64((size_t)n * x);
  p->t = o; o += up64((size_t)n * t);
  p->u = o; o += up64((size_t)n * u);
  p->sc = o; o += up64((size_t)n * sc);
  p->total_floats = o;
  return 0;
}

static int tap_out(const float* x, long n, int P, int ld, int C, float* out, hipStream_t s) {
  hipLaunchKernelGGL(nchw_kernel, dim3((P + 63) / 64, (C + 31) / 32, (unsigned)n), dim3(256), 0, s,
                     x, P, ld, C, out);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

template <bool UP, bool AFFINE>
static int bn_relu(const float* x, const float* scale, const float* shift, long ss_stride, float* y,
                   long n, int side, int C, hipStream_t s) {
  const long total4 = n * side * side * (C / 4);
  hipLaunchKernelGGL((ccbn_relu_up2_kernel<UP, AFFINE>), dim3(grid_for(total4)), dim3(256), 0, s, x,
                     scale, shift, ss_stride, y, total4, side, side, C);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace gan
}  // namespace milan

using namespace milan;

extern "C" {

int milan_sagan_attention(const float* theta, int64_t theta_stride, const float* phi_g, float* out,
                          int n, int height, int width, int channels, milan_stream stream) {
  MILAN_REQUIRE(theta && phi_g && out, MILAN_ERR_ARG, "milan_sagan_attention: null argument");
  return gan::launch_sagan_attention(theta, (long)theta_stride, phi_g, out, n, height, width,
                                     channels, (hipStream_t)stream);
}

int milan_gan_create(milan_gan_ctx** out, int device, const milan_gan_dims* dims) {
  MILAN_REQUIRE(out && dims, MILAN_ERR_ARG, "milan_gan_create: null argument");
  const milan_gan_dims& d = *dims;
  const gan::Arch* a = gan::arch_of(d.resolution);
  MILAN_REQUIRE(a, MILAN_ERR_SHAPE, "gan: resolution %d is not 32, 64, 128, 256 or 512",
                d.resolution);
  MILAN_REQUIRE(d.ch > 0 && d.ch % 4 == 0 && d.ch <= 1024, MILAN_ERR_SHAPE,
                "gan: ch %d must be a multiple of 4 (the convolutions read 4 channels at a time)",
                d.ch);
  MILAN_REQUIRE(d.bottom_width >= 1 && d.bottom_width <= 16, MILAN_ERR_SHAPE,
                "gan: bottom_width %d is not in 1 .. 16", d.bottom_width);
  MILAN_REQUIRE(d.shared_dim > 0 && d.n_classes > 0 && d.dim_z > 0, MILAN_ERR_SHAPE,
                "gan: shared_dim %d, n_classes %d and dim_z %d must be > 0", d.shared_dim,
                d.n_classes, d.dim_z);
  MILAN_REQUIRE(!d.hier || d.dim_z % (a->blocks + 1) == 0, MILAN_ERR_SHAPE,
                "gan: hierarchical dim_z %d is not a multiple of the %d slots", d.dim_z,
                a->blocks + 1);
  MILAN_REQUIRE(d.bn_eps > 0.f && d.out_bn_eps > 0.f, MILAN_ERR_SHAPE, "gan: eps must be > 0");
  int attn_block = -1;
  for (int i = 0; i < a->blocks; ++i)
    if (d.attn_resolution == (8 << i)) attn_block = i;
  MILAN_REQUIRE(d.attn_resolution == 0 || attn_block >= 0, MILAN_ERR_SHAPE,
                "gan: attn_resolution %d is not 0 or the resolution of a block (8 .. %d)",
                d.attn_resolution, 8 << (a->blocks - 1));
  if (attn_block >= 0) {
    const int C = d.ch * a->out[attn_block];
    MILAN_REQUIRE(C % 32 == 0 && C <= 32 * gan::SA_MAX_K, MILAN_ERR_SHAPE,
                  "gan: the attention block has %d channels; milan_sagan_attention takes a "
                  "multiple of 32 up to %d", C, 32 * gan::SA_MAX_K);
  }
  milan_gan_ctx* c = new milan_gan_ctx;
  c->w.device = device;
  c->d = d;
  c->chunk = d.hier ? d.dim_z / (a->blocks + 1) : 0;
  c->z_in = d.hier ? c->chunk : d.dim_z;
  c->blocks.assign(a->blocks, {});
  int off = 0;
  for (int i = 0; i < a->blocks; ++i) {
    auto& b = c->blocks[i];
    b.cin = d.ch * a->in[i];
    b.cout = d.ch * a->out[i];
    b.side = d.bottom_width << i;
    b.attn = i == attn_block;
    b.bn1.off = off; off += b.cin;
    b.bn2.off = off; off += b.cout;
    c->bn_max_c = std::max({c->bn_max_c, b.cin, b.cout});
  }
  c->out_bn.off = off; off += c->blocks.back().cout;
  c->bn_total = off;  // (every channel count is a multiple of 4, so every offset is)
  c->bn_count = 2 * a->blocks + 1;
  *out = c;
  return 0;
}

void milan_gan_destroy(milan_gan_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->w.device);
  if (c->packed) (void)hipFree(c->packed);
  if (c->descs) (void)hipFree(c->descs);
  c->w.release();
  delete c;
}

int milan_gan_set_weight(milan_gan_ctx* c, const char* name, const float* data,
                         const int64_t* shape, int ndim) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "milan_gan_set_weight: bad argument");
  return c->w.set("gan", name, data, shape, ndim);
}

int milan_gan_taps(const milan_gan_ctx* c) {
  if (!c) return 0;
  int taps = 0;
  for (const auto& b : c->blocks) taps += b.attn ? 2 : 1;
  return taps;
}

int milan_gan_finalize_weights(milan_gan_ctx* c, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(!c->w.finalized, MILAN_ERR_STATE, "gan weights already finalized");
  const auto& d = c->d;
  const hipStream_t s = (hipStream_t)stream;
  const size_t S = d.shared_dim, cond = S + c->chunk, P = (size_t)d.bottom_width * d.bottom_width;
  std::vector<tower::Want> wants;
  wants.push_back({"shared.weight", (size_t)d.n_classes * S, &c->shared});
  wants.push_back({"linear.weight", c->blocks[0].cin * P * c->z_in, &c->linear_w});
  wants.push_back({"linear.bias", c->blocks[0].cin * P, &c->linear_b});
  auto bn = [&](const std::string& p, milan_gan_ctx::Bn& b, size_t C) {
    wants.push_back({p + ".gain.weight", C * cond, &b.gain_w});
    wants.push_back({p + ".bias.weight", C * cond, &b.bias_w});
    wants.push_back({p + ".stored_mean", C, &b.mean});
    wants.push_back({p + ".stored_var", C, &b.var});
  };
  for (size_t i = 0; i < c->blocks.size(); ++i) {
    auto& b = c->blocks[i];
    const std::string p = "blocks." + std::to_string(i) + ".0.";
    const size_t ci = b.cin, co = b.cout;
    wants.push_back({p + "conv1.weight", co * ci * 9, &b.conv1_w});
    wants.push_back({p + "conv1.bias", co, &b.conv1_b});
    wants.push_back({p + "conv2.weight", co * co * 9, &b.conv2_w});
    wants.push_back({p + "conv2.bias", co, &b.conv2_b});
    wants.push_back({p + "conv_sc.weight", co * ci, &b.sc_w});
    wants.push_back({p + "conv_sc.bias", co, &b.sc_b});
    bn(p + "bn1", b.bn1, ci);
    bn(p + "bn2", b.bn2, co);
    if (b.attn) {
      const std::string q = "blocks." + std::to_string(i) + ".1.";
      wants.push_back({q + "theta.weight", co / 8 * co, &b.theta});
      wants.push_back({q + "phi.weight", co / 8 * co, &b.phi});
      wants.push_back({q + "g.weight", co / 2 * co, &b.g});
      wants.push_back({q + "o.weight", co * (co / 2), &b.o});
      wants.push_back({q + "gamma", 1, &b.gamma});
    }
  }
  const size_t last = c->blocks.back().cout;
  wants.push_back({"output_layer.0.gain", last, &c->out_bn.gain_w});
  wants.push_back({"output_layer.0.bias", last, &c->out_bn.bias_w});
  wants.push_back({"output_layer.0.stored_mean", last, &c->out_bn.mean});
  wants.push_back({"output_layer.0.stored_var", last, &c->out_bn.var});
  wants.push_back({"output_layer.2.weight", 3 * last * 9, &c->out_w});
  wants.push_back({"output_layer.2.bias", 3, &c->out_b});
  MILAN_TRY(c->w.finalize("gan", wants, s));

  // the convolutions in launch_gemm's packed order [N][Kp], k = (kh, kw, cin)
  size_t total = 64 + 64;  // zero, out_b4
  for (const auto& b : c->blocks) {
    total += gan::up64((size_t)b.cout * gan::kp_of(3, b.cin)) +
             gan::up64((size_t)b.cout * gan::kp_of(3, b.cout)) +
             gan::up64((size_t)b.cout * gan::kp_of(1, b.cin));
    if (b.attn)
      total += gan::up64((size_t)(b.cout / 8 * 6) * gan::kp_of(1, b.cout)) +
               gan::up64((size_t)b.cout * gan::kp_of(1, b.cout / 2));
  }
  total += gan::up64((size_t)4 * gan::kp_of(3, (int)last));
  MILAN_CHECK_HIP(hipMalloc((void**)&c->packed, total * sizeof(float)));
  MILAN_TRY(launch_zero_fill(c->packed, total * sizeof(float), s));
  float* at = c->packed;
  auto take = [&](size_t floats) { float* p = at; at += gan::up64(floats); return p; };
  c->zero = take(64);
  c->out_b4 = take(64);
  for (auto& b : c->blocks) {
    b.p1 = take((size_t)b.cout * gan::kp_of(3, b.cin));
    MILAN_TRY(pack_conv_plain(b.conv1_w, b.cout, b.cin, 3, 3, b.p1, s));
    b.p2 = take((size_t)b.cout * gan::kp_of(3, b.cout));
    MILAN_TRY(pack_conv_plain(b.conv2_w, b.cout, b.cout, 3, 3, b.p2, s));
    b.psc = take((size_t)b.cout * gan::kp_of(1, b.cin));
    MILAN_TRY(pack_conv_plain(b.sc_w, b.cout, b.cin, 1, 1, b.psc, s));
    if (b.attn) {
      const int C = b.cout, dk = C / 8, kp = gan::kp_of(1, C);
      b.ptpg = take((size_t)(6 * dk) * kp);  // rows: theta | phi | g
      MILAN_TRY(pack_conv_plain(b.theta, dk, C, 1, 1, b.ptpg, s));
      MILAN_TRY(pack_conv_plain(b.phi, dk, C, 1, 1, b.ptpg + (size_t)dk * kp, s));
      MILAN_TRY(pack_conv_plain(b.g, 4 * dk, C, 1, 1, b.ptpg + (size_t)2 * dk * kp, s));
      const long po = (long)C * gan::kp_of(1, C / 2);
      b.po = take((size_t)po);  // gamma * o
      MILAN_TRY(pack_conv_plain(b.o, C, C / 2, 1, 1, b.po, s));
      hipLaunchKernelGGL(gan::scale_by_kernel, dim3(gan::grid_for(po)), dim3(256), 0, s, b.po, po,
                         b.gamma);
      MILAN_CHECK_HIP(hipGetLastError());
    }
  }
  // the 3-channel output conv as 4 rows (the fourth zero) so that the tile stores float4
  c->pout = take((size_t)4 * gan::kp_of(3, (int)last));
  MILAN_TRY(pack_conv_plain(c->out_w, 3, (int)last, 3, 3, c->pout, s));
  MILAN_CHECK_HIP(hipMemcpyAsync(c->out_b4, c->out_b, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));

  std::vector<gan::BnDesc> descs;
  for (size_t i = 0; i < c->blocks.size(); ++i) {
    const auto& b = c->blocks[i];
    const int slot = d.hier ? (int)i + 1 : -1;
    descs.push_back({b.bn1.gain_w, b.bn1.bias_w, b.bn1.mean, b.bn1.var, b.cin, slot, b.bn1.off, d.bn_eps});
    descs.push_back({b.bn2.gain_w, b.bn2.bias_w, b.bn2.mean, b.bn2.var, b.cout, slot, b.bn2.off, d.bn_eps});
  }
  descs.push_back({c->out_bn.gain_w, c->out_bn.bias_w, c->out_bn.mean, c->out_bn.var, (int)last, -2,
                   c->out_bn.off, d.out_bn_eps});
  MILAN_CHECK_HIP(hipMalloc((void**)&c->descs, descs.size() * sizeof(gan::BnDesc)));
  MILAN_CHECK_HIP(hipMemcpyAsync(c->descs, descs.data(), descs.size() * sizeof(gan::BnDesc),
                                 hipMemcpyHostToDevice, s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

size_t milan_gan_workspace_bytes(const milan_gan_ctx* c, int n) {
  gan::Plan p;
  if (gan::plan(c, n, &p) != 0) return 0;
  return p.total_floats * sizeof(float);
}

int milan_gan_run(milan_gan_ctx* c, const float* z, const int64_t* classes, const float* y,
                  int y_embedded, int n, float* const* taps, float* images_out, void* ws,
                  size_t ws_bytes, milan_stream stream) {
  using namespace milan::gan;
  MILAN_REQUIRE(c && z && ws, MILAN_ERR_ARG, "milan_gan_run: null argument");
  MILAN_REQUIRE((classes != nullptr) != (y != nullptr), MILAN_ERR_ARG,
                "milan_gan_run: exactly one of classes and y must be given");
  Plan p;
  MILAN_TRY(plan(c, n, &p));
  const auto& d = c->d;
  const int nb = (int)c->blocks.size();
  // tap j: layer0, .., layerK, attnK, layerK+1, ..; the walk ends after the deepest one asked
  // for unless the images are wanted
  int last_tap = -1;
  const int n_taps = milan_gan_taps(c);
  if (taps)
    for (int j = 0; j < n_taps; ++j)
      if (taps[j]) last_tap = j;
  MILAN_REQUIRE(images_out || last_tap >= 0, MILAN_ERR_ARG,
                "milan_gan_run: neither a tap nor the images are asked for");
  MILAN_REQUIRE(ws_bytes >= p.total_floats * sizeof(float), MILAN_ERR_WORKSPACE,
                "milan_gan_run: workspace %zu < %zu bytes", ws_bytes,
                p.total_floats * sizeof(float));
  MILAN_CHECK_HIP(hipSetDevice(c->w.device));
  set_status_word(nullptr);
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  const int S = d.shared_dim;
  const long N = n;
  const float* ye = y_embedded ? y : w + p.y;
  if (!y_embedded) {
    hipLaunchKernelGGL(embed_kernel, dim3(grid_for(N * S)), dim3(256), 0, s, c->shared, classes, y,
                       w + p.y, n, S, d.n_classes);
    MILAN_CHECK_HIP(hipGetLastError());
  } else {
    MILAN_REQUIRE(y != nullptr, MILAN_ERR_ARG, "milan_gan_run: y_embedded without y");
  }
  float *scale = w + p.scale, *shift = w + p.shift;
  hipLaunchKernelGGL(fold_bn_kernel, dim3((c->bn_max_c + 127) / 128, c->bn_count, n), dim3(128), 0,
                     s, c->descs, ye, z, S, c->chunk, d.dim_z, c->bn_total, scale, shift);
  MILAN_CHECK_HIP(hipGetLastError());
  float *x = w + p.x0, *xn = w + p.x1, *t = w + p.t, *u = w + p.u, *sc = w + p.sc;
  {
    const int P = d.bottom_width * d.bottom_width, C = c->blocks[0].cin;
    const long total = N * P * C;
    hipLaunchKernelGGL(first_linear_kernel, dim3(grid_for(total)), dim3(256), 0, s, z, d.dim_z,
                       c->linear_w, c->linear_b, x, total, P, C, c->z_in);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  const long ss = c->bn_total;
  int tap = 0;
  for (int i = 0; i < nb; ++i) {
    const auto& b = c->blocks[i];
    const int si = b.side, so = 2 * b.side;
    // t = up2(relu(ccbn1(x)));  u = relu(ccbn2(conv1(t)))
    MILAN_TRY((bn_relu<true, true>(x, scale + b.bn1.off, shift + b.bn1.off, ss, t, N, si, b.cin, s)));
    MILAN_TRY(conv(t, N, so, so, b.cin, b.cin, b.p1, b.conv1_b, b.cout, 3, EPI_BIAS, nullptr, 0, u,
                   b.cout, c->zero, s));
    MILAN_TRY((bn_relu<false, true>(u, scale + b.bn2.off, shift + b.bn2.off, ss, u, N, so, b.cout, s)));
    // the shortcut: the 1 x 1 conv at the input side, upsampled afterwards (t is free again)
    MILAN_TRY(conv(x, N, si, si, b.cin, b.cin, b.psc, b.sc_b, b.cout, 1, EPI_BIAS, nullptr, 0, sc,
                   b.cout, c->zero, s));
    MILAN_TRY((bn_relu<true, false>(sc, nullptr, nullptr, 0, t, N, si, b.cout, s)));
    MILAN_TRY(conv(u, N, so, so, b.cout, b.cout, b.p2, b.conv2_b, b.cout, 3, EPI_BIAS_ADD, t,
                   b.cout, xn, b.cout, c->zero, s));
    std::swap(x, xn);
    if (taps && taps[tap]) MILAN_TRY(tap_out(x, N, so * so, b.cout, b.cout, taps[tap], s));
    if (!images_out && tap == last_tap) return 0;
    ++tap;
    if (b.attn) {
      const int C = b.cout, dk = C / 8, P = so * so;
      float* f = t;                                   // theta | phi | g, (n, P, 6 dk)
      float* pg = u;                                  // pooled phi | g, (n, P / 4, 5 dk)
      float* att = u + (size_t)N * (P / 4) * 5 * dk;        // (n, P, 4 dk)
      MILAN_TRY(conv(x, N, so, so, C, C, b.ptpg, nullptr, 6 * dk, 1, EPI_BIAS, nullptr, 0, f, 6 * dk,
                     c->zero, s));
      const long total4 = N * (P / 4) * (5 * dk / 4);
      hipLaunchKernelGGL(pool_phi_g_kernel, dim3(grid_for(total4)), dim3(256), 0, s, f, 6 * dk, dk,
                         pg, total4, so, so, 5 * dk);
      MILAN_CHECK_HIP(hipGetLastError());
      MILAN_TRY(launch_sagan_attention(f, 6 * dk, pg, att, N, so, so, C, s));
      MILAN_TRY(conv(att, N, so, so, 4 * dk, 4 * dk, b.po, nullptr, C, 1, EPI_BIAS_ADD, x, C, xn, C,
                     c->zero, s));
      std::swap(x, xn);
      if (taps && taps[tap]) MILAN_TRY(tap_out(x, N, P, C, C, taps[tap], s));
      if (!images_out && tap == last_tap) return 0;
      ++tap;
    }
  }
  if (!images_out) return 0;
  // images = tanh(conv3x3(relu(bn(x)))), 4-column pixels in u, then (n, 3, R, R)
  const int R = 2 * c->blocks.back().side, C = c->blocks.back().cout;
  MILAN_TRY((bn_relu<false, true>(x, scale + c->out_bn.off, shift + c->out_bn.off, ss, t, N, R, C, s)));
  MILAN_TRY(conv(t, N, R, R, C, C, c->pout, c->out_b4, 4, 3, EPI_BIAS_TANH, nullptr, 0, u, 4,
                 c->zero, s));
  MILAN_TRY(tap_out(u, N, R * R, 4, 3, images_out, s));
  return 0;
}

}  // extern "C"
