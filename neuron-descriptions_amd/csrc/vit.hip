// A DINO-style pre-LN vision transformer (facebookresearch/dino, vision_transformer.py) with
// taps on blocks.N.mlp.fc1, and the streaming attention it needs.
//
// A context of its own (milan_vit_ctx): dims + one weight arena in DINO's state-dict layout,
// row-major as torch stores it.  Every contraction goes through tgemm::gemm_rows (tgemm.h;
// split count a function of K alone) and attention works per (sequence, head), so an image's
// taps do not depend on the other images of the call.  LayerNorm, the erf GELU, the patch
// gather and the weight store are the towers' shared parts (tower.hip).
//
// Attention (attention_kernel): the towers' shared kernel holds Q, K, V of a whole head in LDS,
// which ends near 64 tokens.  Here a workgroup owns 128 query rows of one (sequence, head), 32 per
// wave, and streams K / V through LDS 32 keys at a time with the online softmax (running max
// and sum per query row); the T x T scores exist only as one 32 x 32 accumulator tile per wave.
// Both products run on the fp32 MFMA (v_mfma_f32_32x32x2_f32), transposed so that no operand
// ever moves between lanes:
//   S^T = K Q^T   A = K tile (row = key), B = Q^T (column = query).  The accumulator then has
//                 the query on the lane and the 32 keys in 16 registers x 2 lane halves, so
//                 the softmax statistics of a query are lane-local plus one exchange with
//                 lane ^ 32.
//   O^T = V^T P^T A = V^T (row = head column d), B = P^T.  Step r takes register r of the
//                 S^T accumulator as its B operand as it stands: lane half h supplies key
//                 (r & 3) + 8 (r >> 2) + 4 h, and the A operand reads that key's row of V.
// The rescale of O by exp(m_old - m_new) is per query, hence per lane.
//
// Precision: exact fp32; the softmax weights are v_exp_f32 of an exponent formed by FMAs.  Determinism: fixed orders, no atomics;
// the bits of one (sequence, head) depend on nothing else in the launch.
#include "tower_common.h"

#include <string.h>
#include <algorithm>

struct milan_vit_ctx {
  milan_vit_dims d{};
  milan::tower::Weights w;
  struct Block {
    const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b,
        *fc2_w, *fc2_b;
  };
  std::vector<Block> blocks;
  const float *conv_w = nullptr, *conv_b = nullptr, *cls = nullptr, *pos = nullptr,
              *norm_w = nullptr, *norm_b = nullptr;
};

namespace milan {
namespace vit {

using tgemm::Scratch;
using tgemm::View;
using tgemm::view;
using namespace milan::tower;

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int ATT_THREADS = 256;
constexpr int ATT_BM = 128;  // query rows per workgroup (32 per wave)
constexpr int ATT_BN = 32;   // keys per LDS tile
constexpr int ATT_MAX_HD = 128;

// LDS row strides in floats.  K rows are read 16 bytes per lane, lane = key: stride HD + 4
// spreads 16 consecutive keys over all banks.  V rows are read 4 bytes per lane, the two lane
// halves 4 keys apart: 4 * (HD + 8) is 32 banks, so the halves do not collide.
__host__ __device__ constexpr int ldk_of(int hd) { return hd + 4; }
__host__ __device__ constexpr int ldv_of(int hd) { return hd + 8; }
static size_t att_lds_bytes(int hd) {
  return sizeof(float) * (size_t)ATT_BN * (ldk_of(hd) + ldv_of(hd));
}

// qkv: [seq][T][3 W] (q | k | v, heads contiguous inside each), out: [seq][T][W].
// grid.x = seqs * ceil(T / ATT_BM), grid.y = heads.
template <int HD>
__global__ __launch_bounds__(ATT_THREADS) void attention_kernel(const float* __restrict__ qkv,
                                                                float* __restrict__ out, int T,
                                                                int W, int qtiles, float c_hi,
                                                                float c_lo) {
  constexpr int HALF = HD / 2;       // k-steps of S^T: lane half h sums columns h * HALF + s
  constexpr int ND = (HD + 31) / 32; // 32-column blocks of O^T
  constexpr int LDK = ldk_of(HD), LDV = ldv_of(HD);
  constexpr int F4 = ATT_BN * HD / 4;                             // float4 per K (or V) tile
  constexpr int PER = (F4 + ATT_THREADS - 1) / ATT_THREADS;       // of them per thread
  extern __shared__ __align__(16) float lds[];
  float* Ks = lds;
  float* Vs = lds + ATT_BN * LDK;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int seq = blockIdx.x / qtiles, qt = blockIdx.x % qtiles, head = blockIdx.y;
  const size_t row3 = (size_t)3 * W;
  const float* base = qkv + (size_t)seq * T * row3 + (size_t)head * HD;
  const int q0 = qt * ATT_BM + w * 32;  // first query row of this wave
  const int query = q0 + l31;
  const bool wave_on = q0 < T;          // a wave wholly past T only helps with the tiles

  // Q^T operand: lane (query, h) keeps Q[query][h * HALF + s], s < HALF
  float qreg[HALF];
  {
    const float* qp = base + (size_t)(query < T ? query : 0) * row3 + h * HALF;
#pragma unroll
    for (int s = 0; s < HALF; s += 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (query < T) v = *reinterpret_cast<const float4*>(qp + s);
      qreg[s] = v.x; qreg[s + 1] = v.y; qreg[s + 2] = v.z; qreg[s + 3] = v.w;
    }
  }

  v16f acc[ND];
#pragma unroll
  for (int b = 0; b < ND; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // the next tile's global loads are in flight while this one's MFMAs run
  float4 rk[PER], rv[PER];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = tid + u * ATT_THREADS;
      const int key = i / (HD / 4), c = (i % (HD / 4)) * 4;
      rk[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      rv[u] = rk[u];
      if (i < F4 && j0 + key < T) {
        const float* p = base + (size_t)(j0 + key) * row3 + c;
        rk[u] = *reinterpret_cast<const float4*>(p + W);
        rv[u] = *reinterpret_cast<const float4*>(p + 2 * W);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int i = tid + u * ATT_THREADS;
      const int key = i / (HD / 4), c = (i % (HD / 4)) * 4;
      if (i < F4) {
        *reinterpret_cast<float4*>(Ks + key * LDK + c) = rk[u];
        *reinterpret_cast<float4*>(Vs + key * LDV + c) = rv[u];
      }
    }
  };

  fetch(0);
  for (int j0 = 0; j0 < T; j0 += ATT_BN) {
    stash();
    __syncthreads();
    if (j0 + ATT_BN < T) fetch(j0 + ATT_BN);
    if (wave_on) {
      // S^T[key][query] over the head's columns; lane half h walks its own half of them
      v16f st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      const float* kp = Ks + l31 * LDK + h * HALF;
#pragma unroll
      for (int s = 0; s < HALF; s += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(kp + s);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.x, qreg[s], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.y, qreg[s + 1], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.z, qreg[s + 2], st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv.w, qreg[s + 3], st, 0, 0, 0);
      }
      // register r of lane half h is key j0 + (r & 3) + 8 (r >> 2) + 4 h.  Weights in base 2:
      // exp(s / sqrt(HD) - m) = exp2(s c - m2), c = log2(e) / sqrt(HD) = c_hi + c_lo.  m2 is the
      // running max of the rounded s c_hi; the exponent itself is two FMAs on the unrounded
      // product, so it carries one rounding of its own size and none of the score's.  A key
      // past T gets weight 0 by selection (key j0 is always real, so the max is finite).
      const bool partial = j0 + ATT_BN > T;
      if (partial) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (j0 + (r & 3) + 8 * (r >> 2) + 4 * h >= T) st[r] = -INFINITY;
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
        if (partial && j0 + (r & 3) + 8 * (r >> 2) + 4 * h >= T) p = 0.f;
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
      // O^T[d][query] += V[key][d] P^T[key][query]
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vp = Vs + ((r & 3) + 8 * (r >> 2) + 4 * h) * LDV + l31;
#pragma unroll
        for (int b = 0; b < ND; ++b) {
          float vv = 0.f;
          if (HD % 32 == 0 || b * 32 + l31 < HD) vv = vp[b * 32];
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[r], acc[b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (!wave_on || query >= T) return;
  // O^T accumulator: column = query (this lane), row d = 32 b + 8 g + 4 h + (r & 3), r = 4 g + ..
  float* op = out + ((size_t)seq * T + query) * W + (size_t)head * HD;
#pragma unroll
  for (int b = 0; b < ND; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = b * 32 + 8 * g + 4 * h;
      if (HD % 32 != 0 && d0 >= HD) continue;
      float4 v;
      v.x = acc[b][4 * g] / l_run;
      v.y = acc[b][4 * g + 1] / l_run;
      v.z = acc[b][4 * g + 2] / l_run;
      v.w = acc[b][4 * g + 3] / l_run;
      *reinterpret_cast<float4*>(op + d0) = v;
    }
}

template <int HD>
static int launch_attention_hd(const float* qkv, float* out, long seqs, int T, int W, int heads,
                               hipStream_t s) {
  const int qtiles = (T + ATT_BM - 1) / ATT_BM;
  const size_t lds = att_lds_bytes(HD);
  MILAN_TRY(ensure_lds_attr((const void*)attention_kernel<HD>, (int)lds));
  const double c = 1.4426950408889634 / sqrt((double)HD);  // log2(e) / sqrt(HD)
  const float c_hi = (float)c, c_lo = (float)(c - (double)c_hi);
  hipLaunchKernelGGL(attention_kernel<HD>, dim3((unsigned)(seqs * qtiles), heads),
                     dim3(ATT_THREADS), lds, s, qkv, out, T, W, qtiles, c_hi, c_lo);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int check_attention_shape(long seqs, int T, int W, int heads) {
  MILAN_REQUIRE(seqs >= 0 && T >= 1 && W > 0 && heads > 0 && W % heads == 0, MILAN_ERR_SHAPE,
                "attention: %ld sequences of %d tokens, width %d, %d heads", seqs, T, W, heads);
  const int hd = W / heads;
  MILAN_REQUIRE(hd % 16 == 0 && hd <= ATT_MAX_HD, MILAN_ERR_SHAPE,
                "attention: head size %d (width %d / %d heads) is not a multiple of 16 up to %d",
                hd, W, heads, ATT_MAX_HD);
  const long qtiles = (T + ATT_BM - 1) / ATT_BM;
  MILAN_REQUIRE(seqs * qtiles < (1L << 31) && heads < 65536, MILAN_ERR_SHAPE,
                "attention: %ld sequences x %ld query tiles or %d heads exceed the launch grid",
                seqs, qtiles, heads);
  return 0;
}

static int launch_attention(const float* qkv, float* out, long seqs, int T, int W, int heads,
                            hipStream_t s) {
  MILAN_TRY(check_attention_shape(seqs, T, W, heads));
  if (seqs == 0) return 0;
  switch (W / heads) {
    case 16: return launch_attention_hd<16>(qkv, out, seqs, T, W, heads, s);
    case 32: return launch_attention_hd<32>(qkv, out, seqs, T, W, heads, s);
    case 48: return launch_attention_hd<48>(qkv, out, seqs, T, W, heads, s);
    case 64: return launch_attention_hd<64>(qkv, out, seqs, T, W, heads, s);
    case 80: return launch_attention_hd<80>(qkv, out, seqs, T, W, heads, s);
    case 96: return launch_attention_hd<96>(qkv, out, seqs, T, W, heads, s);
    case 112: return launch_attention_hd<112>(qkv, out, seqs, T, W, heads, s);
    default: return launch_attention_hd<128>(qkv, out, seqs, T, W, heads, s);
  }
}

// x[(img * T + t)][:] = (t == 0 ? cls : pe[img * (T - 1) + t - 1]) + pos[t]
__global__ void embed_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                    const float* __restrict__ pos, float* __restrict__ x,
                                    long total, int T, int W) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W);
  const long row = i / W;
  const int t = (int)(row % T);
  const long img = row / T;
  const float v = t == 0 ? cls[j] : pe[(img * (T - 1) + t - 1) * W + j];
  x[i] = v + pos[(long)t * W + j];
}

// Workspace of a walk over n images: x, y ([M][W]), big ([M][max(3 W, hidden)]; before the
// blocks it holds the im2col patches and the patch embeddings), the CLS rows and the GEMMs'
// split-K scratch; in floats, 64-float aligned.
struct Plan {
  size_t x, y, big, scratch, scratch_floats, total_floats;
};

static int plan(const milan_vit_ctx* c, int n, Plan* p) {
  MILAN_REQUIRE(c && c->w.finalized, MILAN_ERR_STATE, "vit: weights are not finalized");
  MILAN_REQUIRE(n > 0, MILAN_ERR_ARG, "vit: %d images", n);
  const auto& d = c->d;
  const int G = d.resolution / d.patch, T = G * G + 1, W = d.width, H = d.hidden;
  const int kk = 3 * d.patch * d.patch, wide = std::max(3 * W, H);
  const long M = (long)n * T, np = (long)n * G * G;
  MILAN_REQUIRE(M < (1L << 31) / (long)wide && np < (1L << 31) / (long)kk, MILAN_ERR_ARG,
                "vit: %d images (%ld tokens x %d columns) exceed the 2^31-element GEMM range", n,
                M, wide);
  size_t o = 0;
  p->x = o; o += up64((size_t)M * W);
  p->y = o; o += up64((size_t)M * W);
  const size_t front = up64((size_t)np * kk) + up64((size_t)np * W);
  p->big = o; o += std::max(up64((size_t)M * wide), front);
  p->scratch_floats = std::max({tgemm::rows_scratch_floats((int)np, W, kk),
                                tgemm::rows_scratch_floats((int)M, 3 * W, W),
                                tgemm::rows_scratch_floats((int)M, W, W),
                                tgemm::rows_scratch_floats((int)M, H, W),
                                tgemm::rows_scratch_floats((int)M, W, H)});
  p->scratch = o; o += up64(p->scratch_floats);
  p->total_floats = o;
  return 0;
}
}  // namespace vit
}  // namespace milan

using namespace milan;
using namespace milan::vit;

extern "C" {

int milan_attention(const float* qkv, float* out, int seqs, int tokens, int width, int heads,
                    milan_stream stream) {
  MILAN_REQUIRE(qkv && out, MILAN_ERR_ARG, "milan_attention: null argument");
  return launch_attention(qkv, out, seqs, tokens, width, heads, (hipStream_t)stream);
}

int milan_vit_create(milan_vit_ctx** out, int device, const milan_vit_dims* dims) {
  MILAN_REQUIRE(out && dims, MILAN_ERR_ARG, "milan_vit_create: null argument");
  const milan_vit_dims& d = *dims;
  MILAN_REQUIRE(d.resolution > 0 && d.patch > 0 && d.resolution % d.patch == 0, MILAN_ERR_SHAPE,
                "vit: resolution %d is not a multiple of patch %d", d.resolution, d.patch);
  MILAN_REQUIRE(d.width > 0 && d.heads > 0 && d.width % d.heads == 0, MILAN_ERR_SHAPE,
                "vit: width %d must be a multiple of the head count %d", d.width, d.heads);
  MILAN_REQUIRE(d.layers > 0 && d.hidden > 0 && d.eps > 0.f, MILAN_ERR_SHAPE,
                "vit: layers, hidden and eps must be > 0");
  const int G = d.resolution / d.patch;
  MILAN_TRY(check_attention_shape(1, G * G + 1, d.width, d.heads));
  milan_vit_ctx* c = new milan_vit_ctx;
  c->w.device = device;
  c->d = d;
  c->blocks.assign(d.layers, {});
  *out = c;
  return 0;
}

void milan_vit_destroy(milan_vit_ctx* c) {
  if (!c) return;
  c->w.release();
  delete c;
}

int milan_vit_set_weight(milan_vit_ctx* c, const char* name, const float* data,
                         const int64_t* shape, int ndim) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "milan_vit_set_weight: bad argument");
  return c->w.set("vit", name, data, shape, ndim);
}

int milan_vit_finalize_weights(milan_vit_ctx* c, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  const auto& d = c->d;
  const int G = d.resolution / d.patch, T = G * G + 1;
  std::vector<Want> wants;
  const size_t W = d.width, H = d.hidden;
  wants.push_back({"patch_embed.proj.weight", W * 3 * d.patch * d.patch, &c->conv_w});
  wants.push_back({"patch_embed.proj.bias", W, &c->conv_b});
  wants.push_back({"cls_token", W, &c->cls});
  wants.push_back({"pos_embed", (size_t)T * W, &c->pos});
  wants.push_back({"norm.weight", W, &c->norm_w});
  wants.push_back({"norm.bias", W, &c->norm_b});
  for (int l = 0; l < d.layers; ++l) {
    const std::string p = "blocks." + std::to_string(l) + ".";
    auto& b = c->blocks[l];
    wants.push_back({p + "norm1.weight", W, &b.ln1_w});
    wants.push_back({p + "norm1.bias", W, &b.ln1_b});
    wants.push_back({p + "attn.qkv.weight", 3 * W * W, &b.qkv_w});
    wants.push_back({p + "attn.qkv.bias", 3 * W, &b.qkv_b});
    wants.push_back({p + "attn.proj.weight", W * W, &b.proj_w});
    wants.push_back({p + "attn.proj.bias", W, &b.proj_b});
    wants.push_back({p + "norm2.weight", W, &b.ln2_w});
    wants.push_back({p + "norm2.bias", W, &b.ln2_b});
    wants.push_back({p + "mlp.fc1.weight", H * W, &b.fc1_w});
    wants.push_back({p + "mlp.fc1.bias", H, &b.fc1_b});
    wants.push_back({p + "mlp.fc2.weight", W * H, &b.fc2_w});
    wants.push_back({p + "mlp.fc2.bias", W, &b.fc2_b});
  }
  return c->w.finalize("vit", wants, (hipStream_t)stream);
}

size_t milan_vit_workspace_bytes(const milan_vit_ctx* c, int n) {
  Plan p;
  if (plan(c, n, &p) != 0) return 0;
  return p.total_floats * sizeof(float);
}

int milan_vit_run(milan_vit_ctx* c, const float* images, int n, int resolution,
                  float* const* taps, float* cls_out, void* ws, size_t ws_bytes,
                  milan_stream stream) {
  MILAN_REQUIRE(c && images && ws, MILAN_ERR_ARG, "milan_vit_run: null argument");
  Plan p;
  MILAN_TRY(plan(c, n, &p));
  const auto& d = c->d;
  MILAN_REQUIRE(resolution == d.resolution, MILAN_ERR_SHAPE,
                "vit: %d x %d pixels, the model takes %d x %d", resolution, resolution,
                d.resolution, d.resolution);
  // the walk ends after fc1 of the deepest tap; the CLS output needs every block
  int last = cls_out ? d.layers - 1 : -1;
  if (!cls_out && taps)
    for (int l = 0; l < d.layers; ++l)
      if (taps[l]) last = l;
  MILAN_REQUIRE(last >= 0, MILAN_ERR_ARG, "milan_vit_run: neither a tap nor the output is asked for");
  MILAN_REQUIRE(ws_bytes >= p.total_floats * sizeof(float), MILAN_ERR_WORKSPACE,
                "milan_vit_run: workspace %zu < %zu bytes", ws_bytes,
                p.total_floats * sizeof(float));
  MILAN_CHECK_HIP(hipSetDevice(c->w.device));
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  const int G = d.resolution / d.patch, T = G * G + 1, W = d.width, H = d.hidden;
  const int kk = 3 * d.patch * d.patch;
  const int M = n * T, np = n * G * G;
  const Scratch sc{w + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  float *x = w + p.x, *y = w + p.y, *big = w + p.big;
  float* patches = big;
  float* pe = patches + up64((size_t)np * kk);
  MILAN_TRY(launch_patch_gather(images, patches, n, d.resolution, d.patch, nullptr, s));
  MILAN_TRY(tgemm::gemm_rows(view(patches, kk), 0, view(c->conv_w, kk), 1, view(pe, W), none,
                           c->conv_b, nullptr, np, W, kk, sc, s));
  hipLaunchKernelGGL(embed_tokens_kernel, dim3(blocks_for((long)M * W)), dim3(256), 0, s, pe,
                     c->cls, c->pos, x, (long)M * W, T, W);
  MILAN_CHECK_HIP(hipGetLastError());
  for (int l = 0; l <= last; ++l) {
    const auto& b = c->blocks[l];
    MILAN_TRY(launch_layernorm_rows(x, W, y, M, W, b.ln1_w, b.ln1_b, d.eps, s));
    MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.qkv_w, W), 1, view(big, 3 * W), none, b.qkv_b,
                             nullptr, M, 3 * W, W, sc, s));
    MILAN_TRY(launch_attention(big, y, n, T, W, d.heads, s));
    MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.proj_w, W), 1, view(x, W), view(x, W),
                             b.proj_b, nullptr, M, W, W, sc, s));
    MILAN_TRY(launch_layernorm_rows(x, W, y, M, W, b.ln2_w, b.ln2_b, d.eps, s));
    float* tap = taps ? taps[l] : nullptr;
    if (l == last && !cls_out) {  // the deepest tap: fc1 writes it, and the walk is over
      MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.fc1_w, W), 1, view(tap, H), none, b.fc1_b,
                               nullptr, M, H, W, sc, s));
      break;
    }
    MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.fc1_w, W), 1, view(big, H), none, b.fc1_b,
                             nullptr, M, H, W, sc, s));
    if (tap)
      MILAN_CHECK_HIP(hipMemcpyAsync(tap, big, (size_t)M * H * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
    MILAN_TRY(launch_gelu_erf(big, (long)M * H, s));
    MILAN_TRY(tgemm::gemm_rows(view(big, H), 0, view(b.fc2_w, H), 1, view(x, W), view(x, W),
                             b.fc2_b, nullptr, M, W, H, sc, s));
  }
  if (cls_out)
    MILAN_TRY(launch_layernorm_rows(x, (long)T * W, cls_out, n, W, c->norm_w, c->norm_b,
                                           d.eps, s));
  return 0;
}

}  // extern "C"
