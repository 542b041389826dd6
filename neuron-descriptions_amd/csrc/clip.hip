// The CLIP reranker (src/milan/rerankers.py): a ViT image tower whose CLS attention row is
// edited by the activation masks, a causal text tower, and the rerank score
//   (1 - lam) * sum_k cos(masked image_k, text) + lam * sum_k cos(image_k, text).
//
// A context of its own (milan_clip_ctx): dims + one weight arena in OpenAI's state-dict
// layout, row-major as torch stores it.  No weight is transposed or packed: every
// contraction goes through tgemm::gemm (tgemm.h), the strided exact-fp32 MFMA GEMM,
// which reads x.W^T through a view.  Bias and residual adds are its epilogue (bias1 / d);
// QuickGELU stays a row kernel, so no existing GEMM instantiation changes.  The plain
// LayerNorm, the L2 norm, the patch gather, the attention kernel (a whole head in LDS, with
// the causal flag and the CLS-row mask edit) and the weight store are the towers' shared
// parts (tower.hip).
//
// Precision: exact fp32 whatever milan_set_precision says on the decoder's context.
// Determinism: fixed reduction orders, no float atomics; equal inputs give equal bits.
//
// Batching: all sequences of a call (images x {masked, unmasked}) go through each layer as
// one GEMM.  The text tower is causal, so the end-of-text row depends only on the positions
// up to it: the caller passes `positions` = max(eot) + 1 and the tower runs over that many
// positions instead of the full context.
#include "tower_common.h"

#include <string.h>
#include <algorithm>

struct milan_clip_ctx {
  milan_clip_dims d{};
  milan::tower::Weights w;
  struct Block {
    const float *ln1_w, *ln1_b, *in_w, *in_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc_w, *fc_b, *pj_w,
        *pj_b;
  };
  struct Tower {
    std::vector<Block> blocks;
    int width = 0, heads = 0;
  };
  Tower vis, txt;
  const float *conv1 = nullptr, *cls = nullptr, *vpos = nullptr, *ln_pre_w = nullptr,
              *ln_pre_b = nullptr, *ln_post_w = nullptr, *ln_post_b = nullptr, *vproj = nullptr;
  const float *tok = nullptr, *tpos = nullptr, *ln_fin_w = nullptr, *ln_fin_b = nullptr,
              *tproj = nullptr;
};

namespace milan {
namespace clip {

using tgemm::Scratch;
using tgemm::View;
using tgemm::view;
using namespace milan::tower;

constexpr float LN_EPS = 1e-5f;

// Bilinear resize of the (n, 1, R, R) masks to the G x G patch grid, align_corners = False,
// no antialiasing (torch's upsample_bilinear2d: src = max(0, (dst + .5) * scale - .5)).
__global__ void mask_downsample_kernel(const float* __restrict__ masks, float* __restrict__ out,
                                       long total, int R, int G) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int gx = (int)(i % G), gy = (int)((i / G) % G);
  const long img = i / ((long)G * G);
  const float scale = (float)R / (float)G;
  float sy = ((float)gy + 0.5f) * scale - 0.5f, sx = ((float)gx + 0.5f) * scale - 0.5f;
  sy = sy < 0.f ? 0.f : sy;
  sx = sx < 0.f ? 0.f : sx;
  const int y0 = min((int)sy, R - 1), x0 = min((int)sx, R - 1);
  const int y1 = y0 + (y0 < R - 1 ? 1 : 0), x1 = x0 + (x0 < R - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const float hy = 1.f - ly, hx = 1.f - lx;
  const float* m = masks + img * (long)R * R;
  out[i] = hy * (hx * m[(long)y0 * R + x0] + lx * m[(long)y0 * R + x1]) +
           ly * (hx * m[(long)y1 * R + x0] + lx * m[(long)y1 * R + x1]);
}

// ---- LayerNorm of gathered rows -------------------------------------------------------------
// One wave per output row r.  Input row r is
//   kind 1: (t == 0 ? cls : pe[(img * (T - 1) + t - 1)]) + pos[t] (image tokens + ln_pre;
//           row r = (copy, img, t): every copy reads the same image)
//   kind 2: src[(r * T + eot(r)) * W], eot(r) = min(argmax ids[r], T - 1)  (ln_final gather)
// (plain and strided rows: launch_layernorm_rows)
struct GatherLnArgs {
  const float* src;
  const float *cls, *pos;
  const int64_t* ids;
  int ctx_len;
  int kind, T, n_img;
  const float *w, *b;
  float* dst;  // [rows][W]
  long rows;
  int W;
};

__global__ __launch_bounds__(256) void gather_layernorm_kernel(GatherLnArgs a) {
  const long r = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= a.rows) return;
  const float* row;
  int t = 0;
  if (a.kind == 1) {
    t = (int)(r % a.T);
    const long img = (r / a.T) % a.n_img;
    row = a.src + (img * (a.T - 1) + (t ? t - 1 : 0)) * (long)a.W;
  } else {
    // first position of the largest id (torch.argmax), read over the whole context
    const int64_t* ids = a.ids + r * (long)a.ctx_len;
    int64_t best = ids[0];
    int at = 0;
    for (int p = 1; p < a.ctx_len; ++p)
      if (ids[p] > best) {
        best = ids[p];
        at = p;
      }
    at = at < a.T ? at : a.T - 1;
    row = a.src + (r * a.T + at) * (long)a.W;
  }
  ln_row(
      [=](int j) {
        if (a.kind == 1) return (t == 0 ? a.cls[j] : row[j]) + a.pos[(long)t * a.W + j];
        return row[j];
      },
      a.W, LN_EPS, a.w, a.b, a.dst + r * (long)a.W, lane);
}

// x[r][t][:] = token_embedding[ids[r][t]] + positional_embedding[t], t < T of ctx_len
__global__ void text_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                  const float* __restrict__ pos, float* __restrict__ x,
                                  long total, int T, int ctx_len, int W, int V) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % W);
  const long rt = i / W;
  const int t = (int)(rt % T);
  const long r = rt / T;
  int64_t id = ids[r * ctx_len + t];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // memory safety only; Python validates
  x[i] = tok[id * W + j] + pos[(long)t * W + j];
}

// x <- x * sigmoid(1.702 x)
__global__ void quick_gelu_kernel(float* __restrict__ x, long total) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float v = x[i];
  x[i] = v * (1.f / (1.f + expf(-1.702f * v)));
}

// One wave per text row c of neuron n = neuron_of[c] (or c / candidates):
//   out[c] = (1 - lam) * sum_k <masked[n][k], text[c]> + lam * sum_k <unmasked[n][k], text[c]>
// with the sums over k in increasing k, as sim.sum(dim=0) adds them.
__global__ __launch_bounds__(256) void rerank_scores_kernel(
    const float* __restrict__ em, const float* __restrict__ eu, const float* __restrict__ text,
    const int32_t* __restrict__ neuron_of, int neurons, int k, long rows, int candidates, int E,
    float lam, float* __restrict__ out) {
  const long c = blockIdx.x * 4L + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= rows) return;
  long n = neuron_of ? neuron_of[c] : c / candidates;
  n = n < 0 ? 0 : (n >= neurons ? neurons - 1 : n);
  const float* t = text + c * E;
  float sm = 0.f, su = 0.f;
  for (int i = 0; i < k; ++i) {
    const float* a = em + (n * k + i) * (long)E;
    const float* b = eu + (n * k + i) * (long)E;
    float da = 0.f, db = 0.f;
    for (int j = lane; j < E; j += 64) {
      da += a[j] * t[j];
      db += b[j] * t[j];
    }
    sm += wave_sum(da);
    su += wave_sum(db);
  }
  if (lane == 0) out[c] = (1.f - lam) * sm + lam * su;
}

// ---- host side ------------------------------------------------------------------------------
static int launch_gather_ln(const GatherLnArgs& a, hipStream_t s) {
  if (a.rows <= 0) return 0;
  hipLaunchKernelGGL(gather_layernorm_kernel, dim3(blocks_for(a.rows, 4)), dim3(256), 0, s, a);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

// Workspace of a tower over `seqs` sequences of T tokens: x, y, big (max(3 W, 4 W) wide), the
// GEMM split-K scratch; all in floats, 64-float aligned.
struct Plan {
  size_t x, y, big, aux, scratch, scratch_floats, total_floats;
};

static size_t tower_scratch(long M, int W) {
  size_t s = 0;
  const int shapes[4][2] = {{3 * W, W}, {W, W}, {4 * W, W}, {W, 4 * W}};
  for (auto& sh : shapes) s = std::max(s, tgemm::split_scratch_floats((int)M, sh[0], sh[1]));
  return s;
}

// The pre-LN residual blocks on x [M = seqs * T][W], in place.
static int run_tower(const milan_clip_ctx::Tower& tw, float* x, float* y, float* big, long seqs,
                     int T, int causal, const float* cls_mask, int n_img, int n_masked,
                     uint64_t mask_layers, Scratch sc, hipStream_t s) {
  const int W = tw.width, hd = W / tw.heads;
  const long M = seqs * T;
  MILAN_REQUIRE(lds_attention_fits(T, hd), MILAN_ERR_ARG,
                "clip attention: %d tokens x head size %d need %zu bytes of LDS (limit %zu)", T,
                hd, lds_attention_bytes(T, hd), LDS_LIMIT);
  MILAN_REQUIRE(M < (1L << 31) / (4L * W), MILAN_ERR_ARG,
                "clip: %ld tokens x width %d exceed the 2^31-element GEMM range", M, W);
  LdsAttention att{};  // uniform sequences of T tokens
  att.qkv = big; att.out = y; att.T = T; att.max_len = T; att.W = W; att.hd = hd;
  att.causal = causal; att.n_img = n_img; att.n_masked = n_masked;
  const View none = view(nullptr, 0);
  for (size_t l = 0; l < tw.blocks.size(); ++l) {
    const auto& b = tw.blocks[l];
    MILAN_TRY(launch_layernorm_rows(x, W, y, (int)M, W, b.ln1_w, b.ln1_b, LN_EPS, s));
    MILAN_TRY(tgemm::gemm(view(y, W), 0, view(b.in_w, W), 1, view(big, 3 * W), none, b.in_b,
                        nullptr, (int)M, 3 * W, W, sc, s));
    att.cls_mask = (cls_mask && l < 64 && ((mask_layers >> l) & 1)) ? cls_mask : nullptr;
    MILAN_TRY(launch_lds_attention(att, seqs, tw.heads, s));
    MILAN_TRY(tgemm::gemm(view(y, W), 0, view(b.out_w, W), 1, view(x, W), view(x, W), b.out_b,
                        nullptr, (int)M, W, W, sc, s));
    MILAN_TRY(launch_layernorm_rows(x, W, y, (int)M, W, b.ln2_w, b.ln2_b, LN_EPS, s));
    MILAN_TRY(tgemm::gemm(view(y, W), 0, view(b.fc_w, W), 1, view(big, 4 * W), none, b.fc_b,
                        nullptr, (int)M, 4 * W, W, sc, s));
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(blocks_for(M * 4 * W)), dim3(256), 0, s, big,
                       M * 4 * W);
    MILAN_TRY(tgemm::gemm(view(big, 4 * W), 0, view(b.pj_w, 4 * W), 1, view(x, W), view(x, W),
                        b.pj_b, nullptr, (int)M, W, 4 * W, sc, s));
  }
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

static int image_plan(const milan_clip_ctx* c, int n, int copies, Plan* p) {
  MILAN_REQUIRE(c && c->w.finalized, MILAN_ERR_STATE, "clip: weights are not finalized");
  MILAN_REQUIRE(n > 0 && (copies == 1 || copies == 2), MILAN_ERR_ARG,
                "clip images: n %d, copies %d", n, copies);
  const auto& d = c->d;
  const int G = d.resolution / d.patch, T = G * G + 1, W = d.vision_width;
  const int kk = 3 * d.patch * d.patch;
  const long seqs = (long)n * copies, M = seqs * T;
  MILAN_REQUIRE(M < (1L << 31) / (4L * W) && (long)n * G * G * kk < (1L << 31), MILAN_ERR_ARG,
                "clip images: %d images are too many for one call", n);
  size_t o = 0;
  p->x = o; o += up64((size_t)M * W);
  p->y = o; o += up64((size_t)M * W);
  // big: qkv / MLP hidden; also the im2col patches and the patch embeddings before the tower
  const size_t front = up64((size_t)n * G * G * kk) + up64((size_t)n * G * G * W);
  p->big = o; o += std::max(up64((size_t)M * 4 * W), front);
  p->aux = o; o += up64((size_t)n * G * G) + 2 * up64((size_t)seqs * std::max(W, d.embed_dim));
  p->scratch_floats = std::max({tower_scratch(M, W),
                                tgemm::split_scratch_floats(n * G * G, W, kk),
                                tgemm::split_scratch_floats((int)seqs, d.embed_dim, W)});
  p->scratch = o; o += up64(p->scratch_floats);
  p->total_floats = o;
  return 0;
}

static int text_plan(const milan_clip_ctx* c, int rows, int positions, Plan* p) {
  MILAN_REQUIRE(c && c->w.finalized, MILAN_ERR_STATE, "clip: weights are not finalized");
  const auto& d = c->d;
  MILAN_REQUIRE(rows > 0 && positions > 0 && positions <= d.context_length, MILAN_ERR_ARG,
                "clip texts: rows %d, positions %d of context %d", rows, positions,
                d.context_length);
  const int W = d.text_width;
  const long M = (long)rows * positions;
  MILAN_REQUIRE(M < (1L << 31) / (4L * W), MILAN_ERR_ARG,
                "clip texts: %d rows are too many for one call", rows);
  size_t o = 0;
  p->x = o; o += up64((size_t)M * W);
  p->y = o; o += up64((size_t)M * W);
  p->big = o; o += up64((size_t)M * 4 * W);
  p->aux = o; o += 2 * up64((size_t)rows * std::max(W, d.embed_dim));
  p->scratch_floats =
      std::max(tower_scratch(M, W), tgemm::split_scratch_floats(rows, d.embed_dim, W));
  p->scratch = o; o += up64(p->scratch_floats);
  p->total_floats = o;
  return 0;
}
}  // namespace clip
}  // namespace milan

using namespace milan;
using namespace milan::clip;

extern "C" {

int milan_clip_create(milan_clip_ctx** out, int device, const milan_clip_dims* dims) {
  MILAN_REQUIRE(out && dims, MILAN_ERR_ARG, "milan_clip_create: null argument");
  const milan_clip_dims& d = *dims;
  MILAN_REQUIRE(d.resolution > 0 && d.patch > 0 && d.resolution % d.patch == 0, MILAN_ERR_SHAPE,
                "clip: resolution %d is not a multiple of patch %d", d.resolution, d.patch);
  MILAN_REQUIRE(d.vision_width > 0 && d.vision_heads > 0 && d.vision_width % d.vision_heads == 0 &&
                    d.text_width > 0 && d.text_heads > 0 && d.text_width % d.text_heads == 0,
                MILAN_ERR_SHAPE, "clip: widths (%d, %d) must be multiples of the head counts (%d, %d)",
                d.vision_width, d.text_width, d.vision_heads, d.text_heads);
  MILAN_REQUIRE(d.vision_layers > 0 && d.text_layers > 0 && d.embed_dim > 0 &&
                    d.context_length > 0 && d.vocab_size > 0,
                MILAN_ERR_SHAPE, "clip: layers, embed_dim, context_length, vocab_size must be > 0");
  const int G = d.resolution / d.patch;
  const int vhd = d.vision_width / d.vision_heads, thd = d.text_width / d.text_heads;
  const size_t lv = lds_attention_bytes(G * G + 1, vhd);
  const size_t lt = lds_attention_bytes(d.context_length, thd);
  MILAN_REQUIRE(lds_attention_fits(G * G + 1, vhd) && lds_attention_fits(d.context_length, thd),
                MILAN_ERR_SHAPE,
                "clip attention: %d image tokens x head size %d (%zu bytes) or %d text tokens x "
                "head size %d (%zu bytes) exceed %zu bytes of LDS",
                G * G + 1, vhd, lv, d.context_length, thd, lt, LDS_LIMIT);
  milan_clip_ctx* c = new milan_clip_ctx;
  c->w.device = device;
  c->d = d;
  c->vis.width = d.vision_width; c->vis.heads = d.vision_heads;
  c->txt.width = d.text_width; c->txt.heads = d.text_heads;
  c->vis.blocks.assign(d.vision_layers, {});
  c->txt.blocks.assign(d.text_layers, {});
  *out = c;
  return 0;
}

void milan_clip_destroy(milan_clip_ctx* c) {
  if (!c) return;
  c->w.release();
  delete c;
}

int milan_clip_set_weight(milan_clip_ctx* c, const char* name, const float* data,
                          const int64_t* shape, int ndim) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "milan_clip_set_weight: bad argument");
  return c->w.set("clip", name, data, shape, ndim);
}

int milan_clip_finalize_weights(milan_clip_ctx* c, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  const auto& d = c->d;
  const int G = d.resolution / d.patch, T = G * G + 1;
  // (name, element count, destination) of every tensor the towers read
  std::vector<Want> wants;
  const size_t VW = d.vision_width, TW = d.text_width, E = d.embed_dim;
  wants.push_back({"visual.conv1.weight", VW * 3 * d.patch * d.patch, &c->conv1});
  wants.push_back({"visual.class_embedding", VW, &c->cls});
  wants.push_back({"visual.positional_embedding", (size_t)T * VW, &c->vpos});
  wants.push_back({"visual.ln_pre.weight", VW, &c->ln_pre_w});
  wants.push_back({"visual.ln_pre.bias", VW, &c->ln_pre_b});
  wants.push_back({"visual.ln_post.weight", VW, &c->ln_post_w});
  wants.push_back({"visual.ln_post.bias", VW, &c->ln_post_b});
  wants.push_back({"visual.proj", VW * E, &c->vproj});
  wants.push_back({"token_embedding.weight", (size_t)d.vocab_size * TW, &c->tok});
  wants.push_back({"positional_embedding", (size_t)d.context_length * TW, &c->tpos});
  wants.push_back({"ln_final.weight", TW, &c->ln_fin_w});
  wants.push_back({"ln_final.bias", TW, &c->ln_fin_b});
  wants.push_back({"text_projection", TW * E, &c->tproj});
  for (int tower = 0; tower < 2; ++tower) {
    auto& tw = tower ? c->txt : c->vis;
    const size_t W = tw.width;
    for (size_t l = 0; l < tw.blocks.size(); ++l) {
      const std::string p = std::string(tower ? "" : "visual.") + "transformer.resblocks." +
                            std::to_string(l) + ".";
      auto& b = tw.blocks[l];
      wants.push_back({p + "ln_1.weight", W, &b.ln1_w});
      wants.push_back({p + "ln_1.bias", W, &b.ln1_b});
      wants.push_back({p + "attn.in_proj_weight", 3 * W * W, &b.in_w});
      wants.push_back({p + "attn.in_proj_bias", 3 * W, &b.in_b});
      wants.push_back({p + "attn.out_proj.weight", W * W, &b.out_w});
      wants.push_back({p + "attn.out_proj.bias", W, &b.out_b});
      wants.push_back({p + "ln_2.weight", W, &b.ln2_w});
      wants.push_back({p + "ln_2.bias", W, &b.ln2_b});
      wants.push_back({p + "mlp.c_fc.weight", 4 * W * W, &b.fc_w});
      wants.push_back({p + "mlp.c_fc.bias", 4 * W, &b.fc_b});
      wants.push_back({p + "mlp.c_proj.weight", 4 * W * W, &b.pj_w});
      wants.push_back({p + "mlp.c_proj.bias", W, &b.pj_b});
    }
  }
  return c->w.finalize("clip", wants, (hipStream_t)stream);
}

size_t milan_clip_image_workspace_bytes(const milan_clip_ctx* c, int n, int both) {
  Plan p;
  if (image_plan(c, n, both ? 2 : 1, &p) != 0) return 0;
  return p.total_floats * sizeof(float);
}

int milan_clip_encode_images(milan_clip_ctx* c, const float* images, int n, int resolution,
                             const float* masks, uint64_t mask_layers, int both,
                             const float* renorm_mul_add, float* out, void* ws, size_t ws_bytes,
                             milan_stream stream) {
  MILAN_REQUIRE(c && images && out && ws, MILAN_ERR_ARG, "milan_clip_encode_images: null argument");
  MILAN_REQUIRE(!both || masks, MILAN_ERR_ARG,
                "milan_clip_encode_images: both = 1 needs masks");
  const int copies = both ? 2 : 1;
  Plan p;
  MILAN_TRY(image_plan(c, n, copies, &p));
  const auto& d = c->d;
  MILAN_REQUIRE(resolution == d.resolution, MILAN_ERR_SHAPE,
                "clip images: %d x %d pixels, the model takes %d x %d", resolution, resolution,
                d.resolution, d.resolution);
  MILAN_REQUIRE(ws_bytes >= p.total_floats * sizeof(float), MILAN_ERR_WORKSPACE,
                "milan_clip_encode_images: workspace %zu < %zu bytes", ws_bytes,
                p.total_floats * sizeof(float));
  MILAN_CHECK_HIP(hipSetDevice(c->w.device));
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  const int G = d.resolution / d.patch, T = G * G + 1, W = d.vision_width, E = d.embed_dim;
  const int kk = 3 * d.patch * d.patch;
  const long seqs = (long)n * copies, np = (long)n * G * G;
  const Scratch sc{w + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  float* patches = w + p.big;
  float* pe = patches + up64((size_t)np * kk);
  float* cm = w + p.aux;
  float* cls_rows = cm + up64((size_t)np);
  float* emb = cls_rows + up64((size_t)seqs * std::max(W, E));
  MILAN_TRY(launch_patch_gather(images, patches, n, d.resolution, d.patch, renorm_mul_add,
                                       s));
  if (masks)
    hipLaunchKernelGGL(mask_downsample_kernel, dim3(blocks_for(np)), dim3(256), 0, s, masks, cm,
                       np, d.resolution, G);
  MILAN_CHECK_HIP(hipGetLastError());
  MILAN_TRY(tgemm::gemm(view(patches, kk), 0, view(c->conv1, kk), 1, view(pe, W), none, nullptr,
                      nullptr, (int)np, W, kk, sc, s));
  GatherLnArgs a{};
  a.src = pe; a.cls = c->cls; a.pos = c->vpos; a.kind = 1; a.T = T; a.n_img = n;
  a.w = c->ln_pre_w; a.b = c->ln_pre_b; a.dst = w + p.x; a.rows = seqs * T; a.W = W;
  MILAN_TRY(launch_gather_ln(a, s));
  MILAN_TRY(run_tower(c->vis, w + p.x, w + p.y, w + p.big, seqs, T, 0, masks ? cm : nullptr, n,
                      n, mask_layers, sc, s));
  MILAN_TRY(launch_layernorm_rows(w + p.x, (long)T * W, cls_rows, (int)seqs, W, c->ln_post_w,
                                  c->ln_post_b, LN_EPS, s));
  MILAN_TRY(tgemm::gemm(view(cls_rows, W), 0, view(c->vproj, E), 0, view(emb, E), none, nullptr,
                      nullptr, (int)seqs, E, W, sc, s));
  return launch_l2norm(emb, out, (int)seqs, E, 1, s);
}

size_t milan_clip_text_workspace_bytes(const milan_clip_ctx* c, int rows, int positions) {
  Plan p;
  if (text_plan(c, rows, positions, &p) != 0) return 0;
  return p.total_floats * sizeof(float);
}

int milan_clip_encode_texts(milan_clip_ctx* c, const int64_t* tokens, int rows, int positions,
                            float* out, void* ws, size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && tokens && out && ws, MILAN_ERR_ARG, "milan_clip_encode_texts: null argument");
  Plan p;
  MILAN_TRY(text_plan(c, rows, positions, &p));
  MILAN_REQUIRE(ws_bytes >= p.total_floats * sizeof(float), MILAN_ERR_WORKSPACE,
                "milan_clip_encode_texts: workspace %zu < %zu bytes", ws_bytes,
                p.total_floats * sizeof(float));
  MILAN_CHECK_HIP(hipSetDevice(c->w.device));
  const hipStream_t s = (hipStream_t)stream;
  const auto& d = c->d;
  float* w = (float*)ws;
  const int W = d.text_width, E = d.embed_dim, T = positions;
  const long M = (long)rows * T;
  const Scratch sc{w + p.scratch, p.scratch_floats};
  float* eot_rows = w + p.aux;
  float* emb = eot_rows + up64((size_t)rows * std::max(W, E));
  hipLaunchKernelGGL(text_embed_kernel, dim3(blocks_for(M * W)), dim3(256), 0, s, tokens, c->tok,
                     c->tpos, w + p.x, M * W, T, d.context_length, W, d.vocab_size);
  MILAN_CHECK_HIP(hipGetLastError());
  MILAN_TRY(run_tower(c->txt, w + p.x, w + p.y, w + p.big, rows, T, 1, nullptr, 1, 0, 0, sc, s));
  GatherLnArgs a{};
  a.src = w + p.x; a.kind = 2; a.T = T; a.ids = tokens; a.ctx_len = d.context_length;
  a.w = c->ln_fin_w; a.b = c->ln_fin_b; a.dst = eot_rows; a.rows = rows; a.W = W;
  MILAN_TRY(launch_gather_ln(a, s));
  MILAN_TRY(tgemm::gemm(view(eot_rows, W), 0, view(c->tproj, E), 0, view(emb, E),
                      view(nullptr, 0), nullptr, nullptr, rows, E, W, sc, s));
  return launch_l2norm(emb, out, rows, E, 1, s);
}

int milan_clip_rerank_scores(const float* masked, const float* unmasked, const float* texts,
                             const int32_t* neuron_of, int neurons, int k, int rows,
                             int candidates, int embed, float lam, float* out,
                             milan_stream stream) {
  MILAN_REQUIRE(masked && unmasked && texts && out, MILAN_ERR_ARG,
                "milan_clip_rerank_scores: null argument");
  MILAN_REQUIRE(neurons > 0 && k > 0 && rows >= 0 && embed > 0 && (neuron_of || candidates > 0),
                MILAN_ERR_ARG, "milan_clip_rerank_scores: neurons %d, k %d, rows %d, embed %d",
                neurons, k, rows, embed);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(rerank_scores_kernel, dim3(blocks_for(rows, 4)), dim3(256), 0,
                     (hipStream_t)stream, masked, unmasked, texts, neuron_of, neurons, k,
                     (long)rows, candidates, embed, lam, out);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
