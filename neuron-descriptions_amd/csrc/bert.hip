// BERTScore (src/utils/metrics.py:94-150): a BERT-family post-LN encoder over ragged
// sentences and the greedy token matching of bert_score 0.3.11.
//
// A context of its own (milan_bert_ctx): dims + one weight arena in the HuggingFace
// state-dict layout, row-major as torch stores it, nothing transposed or packed.  Every
// contraction goes through tgemm::gemm_rows (tgemm.h): the strided exact-fp32 MFMA GEMM
// with its split count a function of K alone, so a sentence's embeddings do not depend on
// the other sentences of the call.  Bias and residual adds are its epilogue.
// LayerNorm, the erf GELU, the L2 norm, the attention kernel (a whole head in LDS, ragged
// through `offsets`) and the weight store are the towers' shared parts (tower.hip).
//
// Ragged rows: the tokens of all sentences of a call are concatenated ([total][W]); the
// offsets array says where each sentence starts.  No padding row exists anywhere: the GEMMs
// run over `total` rows, attention reads each sentence's own length.
//
// Precision: exact fp32 tower; the pair kernel accumulates its cosines and its weighted sums
// in float64 (a few thousand fused multiply-adds per pair, nothing beside the tower).
// Determinism: fixed reduction orders, no float atomics; equal inputs give equal bits.
#include "tower_common.h"

#include <string.h>
#include <algorithm>

struct milan_bert_ctx {
  milan_bert_dims d{};
  milan::tower::Weights w;
  struct Layer {
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *ao_w, *ao_b, *ln1_w, *ln1_b, *in_w, *in_b,
        *out_w, *out_b, *ln2_w, *ln2_b;
  };
  std::vector<Layer> layers;
  const float *word = nullptr, *pos = nullptr, *type = nullptr, *eln_w = nullptr,
              *eln_b = nullptr;
};

namespace milan {
namespace bert {

using tgemm::Scratch;
using tgemm::View;
using tgemm::view;
using namespace milan::tower;

constexpr int MAX_TOKENS = MILAN_BERT_MAX_TOKENS;
constexpr int PAIR_THREADS = 256;
constexpr int PAIR_KC = 32;                                          // columns per LDS chunk
constexpr int PAIR_SLOTS = MAX_TOKENS * MAX_TOKENS / PAIR_THREADS;  // sim entries per thread

// Sentence of token row r: the last s with offsets[s] <= r (offsets ascending, n + 1 entries).
__device__ __forceinline__ int sentence_of(const int32_t* offsets, int n, int r) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// x[r] = LayerNorm(word[ids[r]] + pos[position_offset + t] + type[0]), t = r - offsets[s].
// One wave per token row.
__global__ __launch_bounds__(256) void embed_ln_kernel(
    const int64_t* __restrict__ ids, const int32_t* __restrict__ offsets, int n, int total,
    const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
    const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ x, int W,
    int V, int P, int position_offset, float eps) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= total) return;
  const int s = sentence_of(offsets, n, r);
  int64_t id = ids[r];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);  // memory safety only; Python validates
  int p = position_offset + (r - offsets[s]);
  p = p < 0 ? 0 : (p >= P ? P - 1 : p);
  const float* we = word + id * W;
  const float* pe = pos + (long)p * W;
  ln_row([&](int j) { return we[j] + type[j] + pe[j]; }, W, eps, w, b, x + (long)r * W, lane);
}

// One workgroup per (candidate, reference) pair.  The two sentences' normalised rows go
// through LDS PAIR_KC columns at a time ([tokens][PAIR_KC + 1] each); thread t owns the
// entries e = t, t + 256, ... of the Tc x Tr similarity block, e = i * Tr + j, and adds the
// chunk's products in increasing column order.  Then, from the block in LDS: the row maxima
// p_i and column maxima r_j over the other sentence's real tokens, the idf weights normalised
// to sum 1, P = sum_i w_i p_i and R = sum_j v_j r_j in increasing token order, F = 2PR/(P+R)
// (NaN -> 0); a sentence of at most two tokens ([cls, sep]) gives P = R = F = 0.
__global__ __launch_bounds__(PAIR_THREADS) void score_pairs_kernel(
    const float* __restrict__ emb, const int32_t* __restrict__ offsets,
    const float* __restrict__ weights, const int32_t* __restrict__ cand,
    const int32_t* __restrict__ ref, int n_sent, int W, float* __restrict__ out) {
  __shared__ float Cs[MAX_TOKENS][PAIR_KC + 1];
  __shared__ float Rs[MAX_TOKENS][PAIR_KC + 1];
  __shared__ float S[MAX_TOKENS][MAX_TOKENS + 1];
  __shared__ float pmax[MAX_TOKENS], rmax[MAX_TOKENS];
  const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int c = cand[pair], r = ref[pair];
  c = c < 0 ? 0 : (c >= n_sent ? n_sent - 1 : c);  // memory safety only
  r = r < 0 ? 0 : (r >= n_sent ? n_sent - 1 : r);
  const int c0 = offsets[c], r0 = offsets[r];
  int Tc = offsets[c + 1] - c0, Tr = offsets[r + 1] - r0;
  Tc = Tc < 0 ? 0 : (Tc > MAX_TOKENS ? MAX_TOKENS : Tc);
  Tr = Tr < 0 ? 0 : (Tr > MAX_TOKENS ? MAX_TOKENS : Tr);
  float* o = out + 3L * pair;
  if (Tc <= 2 || Tr <= 2) {
    if (tid < 3) o[tid] = 0.f;
    return;
  }
  const int entries = Tc * Tr;
  double acc[PAIR_SLOTS];
  int ei[PAIR_SLOTS], ej[PAIR_SLOTS];
#pragma unroll
  for (int u = 0; u < PAIR_SLOTS; ++u) {
    const int e = tid + u * PAIR_THREADS;
    acc[u] = 0.;
    ei[u] = e < entries ? e / Tr : 0;
    ej[u] = e < entries ? e % Tr : 0;
  }
  for (int k0 = 0; k0 < W; k0 += PAIR_KC) {
    const int kc = min(PAIR_KC, W - k0);
    for (int i = tid; i < Tc * PAIR_KC; i += PAIR_THREADS) {
      const int t = i / PAIR_KC, k = i % PAIR_KC;
      Cs[t][k] = k < kc ? emb[((long)c0 + t) * W + k0 + k] : 0.f;
    }
    for (int i = tid; i < Tr * PAIR_KC; i += PAIR_THREADS) {
      const int t = i / PAIR_KC, k = i % PAIR_KC;
      Rs[t][k] = k < kc ? emb[((long)r0 + t) * W + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PAIR_SLOTS; ++u) {
      if (tid + u * PAIR_THREADS < entries) {
        const float* a = Cs[ei[u]];
        const float* b = Rs[ej[u]];
        double s = acc[u];
        for (int k = 0; k < PAIR_KC; ++k) s = fma((double)a[k], (double)b[k], s);
        acc[u] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < PAIR_SLOTS; ++u)
    if (tid + u * PAIR_THREADS < entries) S[ei[u]][ej[u]] = (float)acc[u];
  __syncthreads();
  for (int i = w; i < Tc; i += 4) {
    float m = -INFINITY;
    for (int j = lane; j < Tr; j += 64) m = fmaxf(m, S[i][j]);
    m = wave_max(m);
    if (lane == 0) pmax[i] = m;
  }
  for (int j = w; j < Tr; j += 4) {
    float m = -INFINITY;
    for (int i = lane; i < Tc; i += 64) m = fmaxf(m, S[i][j]);
    m = wave_max(m);
    if (lane == 0) rmax[j] = m;
  }
  __syncthreads();
  if (tid == 0) {
    double wc = 0., wr = 0., P = 0., R = 0.;
    for (int i = 0; i < Tc; ++i) wc += (double)weights[c0 + i];
    for (int j = 0; j < Tr; ++j) wr += (double)weights[r0 + j];
    for (int i = 0; i < Tc; ++i) P += (double)weights[c0 + i] / wc * (double)pmax[i];
    for (int j = 0; j < Tr; ++j) R += (double)weights[r0 + j] / wr * (double)rmax[j];
    double F = 2. * P * R / (P + R);
    if (F != F) F = 0.;
    o[0] = (float)P;
    o[1] = (float)R;
    o[2] = (float)F;
  }
}

// ---- host side ------------------------------------------------------------------------------

// Workspace of an encode over `total` token rows: x, y ([total][W]), big ([total][max(3 W,
// I)]) and the GEMMs' split-K scratch; in floats, 64-float aligned.
struct Plan {
  size_t x, y, big, scratch, scratch_floats, total_floats;
};

static int plan(const milan_bert_ctx* c, int n, int total, Plan* p) {
  MILAN_REQUIRE(c && c->w.finalized, MILAN_ERR_STATE, "bert: weights are not finalized");
  const auto& d = c->d;
  MILAN_REQUIRE(n > 0 && total >= n, MILAN_ERR_ARG, "bert encode: %d sentences, %d tokens", n,
                total);
  const int W = d.width, I = d.intermediate, wide = std::max(3 * W, I);
  MILAN_REQUIRE((long)total < (1L << 31) / (long)wide, MILAN_ERR_ARG,
                "bert encode: %d tokens x %d columns exceed the 2^31-element GEMM range", total,
                wide);
  size_t o = 0;
  p->x = o; o += up64((size_t)total * W);
  p->y = o; o += up64((size_t)total * W);
  p->big = o; o += up64((size_t)total * wide);
  p->scratch_floats = std::max({tgemm::rows_scratch_floats(total, W, W),
                                tgemm::rows_scratch_floats(total, I, W),
                                tgemm::rows_scratch_floats(total, W, I)});
  p->scratch = o; o += up64(p->scratch_floats);
  p->total_floats = o;
  return 0;
}

}  // namespace bert
}  // namespace milan

using namespace milan;
using namespace milan::bert;

extern "C" {

int milan_bert_create(milan_bert_ctx** out, int device, const milan_bert_dims* dims) {
  MILAN_REQUIRE(out && dims, MILAN_ERR_ARG, "milan_bert_create: null argument");
  const milan_bert_dims& d = *dims;
  MILAN_REQUIRE(d.width > 0 && d.heads > 0 && d.width % d.heads == 0, MILAN_ERR_SHAPE,
                "bert: width %d must be a multiple of the head count %d", d.width, d.heads);
  MILAN_REQUIRE(d.vocab_size > 0 && d.layers > 0 && d.intermediate > 0 && d.max_positions > 0 &&
                    d.type_vocab > 0 && d.position_offset >= 0 && d.eps > 0.f,
                MILAN_ERR_SHAPE,
                "bert: vocab_size, layers, intermediate, max_positions, type_vocab, eps must be "
                "> 0 and position_offset >= 0");
  MILAN_REQUIRE(d.position_offset < d.max_positions, MILAN_ERR_SHAPE,
                "bert: position_offset %d leaves no position of %d", d.position_offset,
                d.max_positions);
  const int hd = d.width / d.heads;
  const size_t lds = lds_attention_bytes(MAX_TOKENS, hd);
  MILAN_REQUIRE(lds_attention_fits(MAX_TOKENS, hd), MILAN_ERR_SHAPE,
                "bert attention: %d tokens x head size %d (width %d / %d heads) need %zu bytes of "
                "LDS, a workgroup has %zu",
                MAX_TOKENS, hd, d.width, d.heads, lds, LDS_LIMIT);
  milan_bert_ctx* c = new milan_bert_ctx;
  c->w.device = device;
  c->d = d;
  c->layers.assign(d.layers, {});
  *out = c;
  return 0;
}

void milan_bert_destroy(milan_bert_ctx* c) {
  if (!c) return;
  c->w.release();
  delete c;
}

int milan_bert_set_weight(milan_bert_ctx* c, const char* name, const float* data,
                          const int64_t* shape, int ndim) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "milan_bert_set_weight: bad argument");
  return c->w.set("bert", name, data, shape, ndim);
}

int milan_bert_finalize_weights(milan_bert_ctx* c, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  const auto& d = c->d;
  std::vector<Want> wants;
  const size_t W = d.width, I = d.intermediate;
  wants.push_back({"embeddings.word_embeddings.weight", (size_t)d.vocab_size * W, &c->word});
  wants.push_back({"embeddings.position_embeddings.weight", (size_t)d.max_positions * W, &c->pos});
  wants.push_back({"embeddings.token_type_embeddings.weight", (size_t)d.type_vocab * W, &c->type});
  wants.push_back({"embeddings.LayerNorm.weight", W, &c->eln_w});
  wants.push_back({"embeddings.LayerNorm.bias", W, &c->eln_b});
  for (int l = 0; l < d.layers; ++l) {
    const std::string p = "encoder.layer." + std::to_string(l) + ".";
    auto& b = c->layers[l];
    wants.push_back({p + "attention.self.query.weight", W * W, &b.q_w});
    wants.push_back({p + "attention.self.query.bias", W, &b.q_b});
    wants.push_back({p + "attention.self.key.weight", W * W, &b.k_w});
    wants.push_back({p + "attention.self.key.bias", W, &b.k_b});
    wants.push_back({p + "attention.self.value.weight", W * W, &b.v_w});
    wants.push_back({p + "attention.self.value.bias", W, &b.v_b});
    wants.push_back({p + "attention.output.dense.weight", W * W, &b.ao_w});
    wants.push_back({p + "attention.output.dense.bias", W, &b.ao_b});
    wants.push_back({p + "attention.output.LayerNorm.weight", W, &b.ln1_w});
    wants.push_back({p + "attention.output.LayerNorm.bias", W, &b.ln1_b});
    wants.push_back({p + "intermediate.dense.weight", I * W, &b.in_w});
    wants.push_back({p + "intermediate.dense.bias", I, &b.in_b});
    wants.push_back({p + "output.dense.weight", W * I, &b.out_w});
    wants.push_back({p + "output.dense.bias", W, &b.out_b});
    wants.push_back({p + "output.LayerNorm.weight", W, &b.ln2_w});
    wants.push_back({p + "output.LayerNorm.bias", W, &b.ln2_b});
  }
  return c->w.finalize("bert", wants, (hipStream_t)stream);
}

size_t milan_bert_encode_workspace_bytes(const milan_bert_ctx* c, int n, int total) {
  Plan p;
  if (plan(c, n, total, &p) != 0) return 0;
  return p.total_floats * sizeof(float);
}

int milan_bert_encode(milan_bert_ctx* c, const int64_t* ids, const int32_t* offsets, int n,
                      int total, int max_len, int normalize, float* out, void* ws,
                      size_t ws_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && ids && offsets && out && ws, MILAN_ERR_ARG,
                "milan_bert_encode: null argument");
  Plan p;
  MILAN_TRY(plan(c, n, total, &p));
  const auto& d = c->d;
  MILAN_REQUIRE(max_len > 0 && max_len <= total, MILAN_ERR_ARG,
                "bert encode: longest sentence %d of %d tokens", max_len, total);
  MILAN_REQUIRE(max_len <= MAX_TOKENS && d.position_offset + max_len <= d.max_positions,
                MILAN_ERR_SHAPE,
                "bert encode: a sentence of %d tokens exceeds the supported %d (attention in LDS) "
                "or the %d positions after offset %d",
                max_len, MAX_TOKENS, d.max_positions, d.position_offset);
  MILAN_REQUIRE(ws_bytes >= p.total_floats * sizeof(float), MILAN_ERR_WORKSPACE,
                "milan_bert_encode: workspace %zu < %zu bytes", ws_bytes,
                p.total_floats * sizeof(float));
  MILAN_CHECK_HIP(hipSetDevice(c->w.device));
  const hipStream_t s = (hipStream_t)stream;
  float* w = (float*)ws;
  const int W = d.width, I = d.intermediate, hd = W / d.heads, M = total;
  const Scratch sc{w + p.scratch, p.scratch_floats};
  const View none = view(nullptr, 0);
  float *x = w + p.x, *y = w + p.y, *big = w + p.big;
  LdsAttention att{};  // ragged, bidirectional, no mask edit
  att.qkv = big; att.out = y; att.offsets = offsets; att.max_len = max_len; att.W = W;
  att.hd = hd;
  hipLaunchKernelGGL(embed_ln_kernel, dim3(blocks_for(M, 4)), dim3(256), 0, s, ids, offsets, n,
                     total, c->word, c->pos, c->type, c->eln_w, c->eln_b, x, W, d.vocab_size,
                     d.max_positions, d.position_offset, d.eps);
  MILAN_CHECK_HIP(hipGetLastError());
  for (const auto& b : c->layers) {
    // q | k | v side by side in big [M][3 W]: three GEMMs on the unpacked weights
    const float* qkv_w[3] = {b.q_w, b.k_w, b.v_w};
    const float* qkv_b[3] = {b.q_b, b.k_b, b.v_b};
    for (int i = 0; i < 3; ++i)
      MILAN_TRY(tgemm::gemm_rows(view(x, W), 0, view(qkv_w[i], W), 1, view(big + i * W, 3 * W),
                               none, qkv_b[i], nullptr, M, W, W, sc, s));
    MILAN_TRY(launch_lds_attention(att, n, d.heads, s));
    // x <- y Wo^T + bo + x, y <- LayerNorm(x)
    MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.ao_w, W), 1, view(x, W), view(x, W), b.ao_b,
                             nullptr, M, W, W, sc, s));
    MILAN_TRY(launch_layernorm_rows(x, W, y, M, W, b.ln1_w, b.ln1_b, d.eps, s));
    MILAN_TRY(tgemm::gemm_rows(view(y, W), 0, view(b.in_w, W), 1, view(big, I), none, b.in_b,
                             nullptr, M, I, W, sc, s));
    MILAN_TRY(launch_gelu_erf(big, (long)M * I, s));
    // y <- big Wout^T + bout + y, x <- LayerNorm(y)
    MILAN_TRY(tgemm::gemm_rows(view(big, I), 0, view(b.out_w, I), 1, view(y, W), view(y, W),
                             b.out_b, nullptr, M, W, I, sc, s));
    MILAN_TRY(launch_layernorm_rows(y, W, x, M, W, b.ln2_w, b.ln2_b, d.eps, s));
  }
  return launch_l2norm(x, out, M, W, normalize ? 1 : 0, s);
}

int milan_bert_score_pairs(const float* emb, const int32_t* offsets, const float* weights,
                           const int32_t* cand, const int32_t* ref, int pairs, int n_sent,
                           int width, float* out, milan_stream stream) {
  MILAN_REQUIRE(emb && offsets && weights && cand && ref && out, MILAN_ERR_ARG,
                "milan_bert_score_pairs: null argument");
  MILAN_REQUIRE(pairs >= 0 && n_sent > 0 && width > 0, MILAN_ERR_ARG,
                "milan_bert_score_pairs: pairs %d, sentences %d, width %d", pairs, n_sent, width);
  if (pairs == 0) return 0;
  hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)pairs), dim3(PAIR_THREADS), 0,
                     (hipStream_t)stream, emb, offsets, weights, cand, ref, n_sent, width, out);
  MILAN_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
