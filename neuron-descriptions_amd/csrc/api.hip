// extern "C" surface of libmilan_hip (see include/milan_hip.h).
#include "common.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace milan {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int dev_alloc(milan_ctx* c, void** p, size_t bytes) {
  if (bytes == 0) bytes = 16;
  MILAN_CHECK_HIP(hipMalloc(p, (bytes + 255) & ~size_t(255)));
  c->owned.push_back(*p);
  return 0;
}

__global__ void absmax_kernel(const float* __restrict__ w, long n,
                              unsigned int* __restrict__ out) {
  float m = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(w[i]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}

// Split-f16 copy of a packed [n][kp] fp32 weight into `dst` (same size);
// d_max: device scratch word.  Returns 1/scale through ws_inv.
static int split_weight_into(const float* w, int n, int kp, float* dst,
                             float* ws_inv, unsigned int* d_max, hipStream_t s) {
  MILAN_CHECK_HIP(hipMemsetAsync(d_max, 0, sizeof(unsigned int), s));
  const long total = (long)n * kp;
  long blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(absmax_kernel, dim3((int)blocks), dim3(256), 0, s, w, total,
                     d_max);
  unsigned int bits = 0;
  MILAN_CHECK_HIP(hipMemcpyAsync(&bits, d_max, sizeof(bits), hipMemcpyDeviceToHost, s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  MILAN_CHECK_HIP(hipMemsetAsync(d_max, 0, sizeof(unsigned int), s));
  float amax;
  memcpy(&amax, &bits, sizeof(amax));
  // scale = 2^e with max|w| * scale in [8192, 16384): hi never overflows f16
  // and lo = O(2^-11 * hi) stays in the f16 normal range for all but tiny w.
  float scale = 1.f;
  if (amax > 0.f && amax < 3.0e38f) {
    int e;
    frexpf(amax, &e);  // amax = f * 2^e, f in [0.5, 1)
    int shift = 14 - e;
    if (shift > 40) shift = 40;
    if (shift < -40) shift = -40;
    scale = ldexpf(1.f, shift);
  }
  MILAN_TRY(launch_f32_to_split(w, kp, dst, kp, n, kp, scale, s));
  *ws_inv = 1.f / scale;
  return 0;
}

int make_split_weight(milan_ctx* c, const float* w, int n, int kp, float** ws,
                      float* ws_inv, hipStream_t s) {
  if (kp % 32 != 0) { *ws = nullptr; *ws_inv = 1.f; return 0; }
  unsigned int* d_max = reinterpret_cast<unsigned int*>(c->zero) + 32;  // scratch
  MILAN_TRY(dev_alloc(c, (void**)ws, sizeof(float) * (size_t)n * kp));
  return split_weight_into(w, n, kp, *ws, ws_inv, d_max, s);
}

// dst = w with columns [0, c0) of every row multiplied by `f0` and columns [c0, c1) by `f1`
// (powers of two)
__global__ void scale_cols_kernel(const float* __restrict__ w, long n, int kp, int c0, int c1,
                                  float f0, float f1, float* __restrict__ dst) {
  const long total = n * kp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int col = (int)(i % kp);
    dst[i] = col < c0 ? w[i] * f0 : (col < c1 ? w[i] * f1 : w[i]);
  }
}

// The split copy of an LSTM's concatenated weight [W_ih | W_hh] again, its embedding columns
// [0, E) divided by the context's embedding scale and its feature columns [E, E + F) (the
// decoder's cell; F = 0 for the LM's layer 0) by the feature scale, written over the old
// copy; the layer's weight scale follows the new maximum.
static int resplit_cat(milan_ctx* c, LinearW& w, int E, int F, hipStream_t s) {
  if (!w.ws) return 0;
  float* tmp = nullptr;
  MILAN_CHECK_HIP(hipMalloc((void**)&tmp, sizeof(float) * (size_t)w.n * w.kp));
  const long total = (long)w.n * w.kp;
  const long blocks = (total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096;
  hipLaunchKernelGGL(scale_cols_kernel, dim3((int)blocks), dim3(256), 0, s, w.w, (long)w.n,
                     w.kp, E, E + F, 1.f / c->emb_scale, 1.f / c->feat_scale, tmp);
  unsigned int* d_max = reinterpret_cast<unsigned int*>(c->zero) + 32;  // scratch
  set_status_word(nullptr);  // (weight packing is not a saturation event of a call)
  int r = (int)hipGetLastError();
  if (r == 0) r = split_weight_into(tmp, w.n, w.kp, w.ws, &w.ws_inv, d_max, s);
  const hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(tmp);
  MILAN_TRY(r);
  MILAN_CHECK_HIP(e);
  return 0;
}

static int resplit_lstm_cats(milan_ctx* c, hipStream_t s) {
  MILAN_CHECK_HIP(hipSetDevice(c->device));
  // a captured decode graph holds the old scales in its kernel arguments
  for (auto& g : c->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  c->graphs.clear();
  MILAN_TRY(resplit_cat(c, c->lstm_cat, c->d.embedding_size, c->d.feature_size, s));
  if (!c->lm_cat.empty())
    MILAN_TRY(resplit_cat(c, c->lm_cat[0], c->d.lm_embedding_size, 0, s));
  return 0;
}

}  // namespace milan

using namespace milan;

extern "C" {

int milan_abi_version(void) { return MILAN_ABI_VERSION; }

const char* milan_last_error(void) { return g_err; }

int milan_create(milan_ctx** out, int device, const milan_dims* dims) {
  MILAN_REQUIRE(out && dims, MILAN_ERR_ARG, "milan_create: null argument");
  const milan_dims& d = *dims;
  MILAN_REQUIRE(d.trunk_kind >= MILAN_TRUNK_BOTTLENECK &&
                    d.trunk_kind <= MILAN_TRUNK_VGG,
                MILAN_ERR_ARG, "unknown trunk_kind %d", d.trunk_kind);
  if (d.trunk_kind == MILAN_TRUNK_NONE) {
    // features come from a foreign Encoder: only the decoder's GEMM alignment
    MILAN_REQUIRE(d.feature_size > 0 && d.feature_size % 4 == 0, MILAN_ERR_SHAPE,
                  "feature_size %d must be a positive multiple of 4",
                  d.feature_size);
  } else {
    MILAN_REQUIRE(d.trunk_width > 0 && d.trunk_width % 4 == 0, MILAN_ERR_SHAPE,
                  "trunk_width %d must be a positive multiple of 4", d.trunk_width);
    const int fmul = d.trunk_kind == MILAN_TRUNK_BOTTLENECK       ? 61
                     : d.trunk_kind == MILAN_TRUNK_BASIC          ? 16
                     : d.trunk_kind == MILAN_TRUNK_ALEXNET_PLACES ? 43
                     : d.trunk_kind == MILAN_TRUNK_VGG            ? 23
                                                                  : 18;
    MILAN_REQUIRE(d.feature_size == fmul * d.trunk_width, MILAN_ERR_SHAPE,
                  "feature_size %d != %d * trunk_width (pyramid of five taps, "
                  "trunk_kind %d)", d.feature_size, fmul, d.trunk_kind);
    for (int i = 0; i < 4 && d.trunk_kind != MILAN_TRUNK_ALEXNET &&
                    d.trunk_kind != MILAN_TRUNK_ALEXNET_PLACES &&
                    d.trunk_kind != MILAN_TRUNK_VGG; ++i)
      MILAN_REQUIRE(d.trunk_blocks[i] > 0, MILAN_ERR_SHAPE, "bad trunk_blocks");
  }
  MILAN_REQUIRE(d.hidden_size > 0 && d.hidden_size % 4 == 0 &&
                    d.embedding_size > 0 && d.embedding_size % 4 == 0 &&
                    d.attention_size > 0 && d.attention_size % 4 == 0,
                MILAN_ERR_SHAPE,
                "hidden/embedding/attention sizes must be positive multiples of 4");
  MILAN_REQUIRE(d.vocab_size > 4 && d.start_index >= 0 &&
                    d.start_index < d.vocab_size && d.stop_index >= 0 &&
                    d.stop_index < d.vocab_size,
                MILAN_ERR_SHAPE, "bad vocab_size / special indices");
  if (d.has_lm)
    MILAN_REQUIRE(d.lm_layers >= 1 && d.lm_hidden_size % 4 == 0 &&
                      d.lm_embedding_size % 4 == 0 && d.lm_hidden_size > 0 &&
                      d.lm_embedding_size > 0,
                  MILAN_ERR_SHAPE, "bad LM dimensions");
  MILAN_CHECK_HIP(hipSetDevice(device));
  milan_ctx* c = new milan_ctx();
  c->device = device;
  c->d = d;
  if (const char* e = getenv("MILAN_ACT_SCALE_LOG2")) {
    // activation scale of the split-f16 trunk (common.h, milan_ctx::act_scale); 0 = none
    int k = atoi(e);
    k = k < 0 ? 0 : (k > 10 ? 10 : k);
    c->act_scale = ldexpf(1.f, k);
    c->act_scale_log2 = k;
  }
  int r = dev_alloc(c, (void**)&c->zero, 256);
  if (r == 0) {
    hipError_t e = hipMemset(c->zero, 0, 256);
    if (e != hipSuccess) r = (int)e;
  }
  if (r == 0) {
    // status word (+ the calibration maximum next to it)
    r = dev_alloc(c, (void**)&c->status, 256);
    if (r == 0) {
      hipError_t e = hipMemset(c->status, 0, 256);
      if (e != hipSuccess) r = (int)e;
    }
  }
  if (r == 0) {
    // image sharing: the two device-side counters of milan_image_sharing_stats
    r = dev_alloc(c, (void**)&c->share_stats, 256);
    if (r == 0) {
      hipError_t e = hipMemset(c->share_stats, 0, 256);
      if (e != hipSuccess) r = (int)e;
    }
  }
  if (const char* e = getenv("MILAN_SHARE_HASH_BITS")) {
    // test knob: only that many low bits of the image hash select candidates (0: every pair
    // of slots goes through the byte comparison)
    const int k = atoi(e);
    c->share_hash_bits = k < 0 ? 0 : (k > 64 ? 64 : k);
  }
  if (r != 0) { milan_destroy(c); return r; }
  *out = c;
  return 0;
}

void milan_destroy(milan_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // (the thread-local status word must not outlive the context it points into: a later
  // ctx-less call -- milan_conv2d_nhwc -- would atomicOr into freed device memory)
  if (status_word() == c->status) set_status_word(nullptr);
  for (auto& g : c->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  for (void* p : c->owned) (void)hipFree(p);
  delete c;
}

int milan_set_weight(milan_ctx* c, const char* name, const float* data,
                     const int64_t* shape, int ndim) {
  MILAN_REQUIRE(c && name && data && (shape || ndim == 0) && ndim >= 0 && ndim <= 8,
                MILAN_ERR_ARG, "milan_set_weight: bad argument");
  MILAN_REQUIRE(!c->finalized, MILAN_ERR_STATE,
                "milan_set_weight after milan_finalize_weights");
  Tensor t;
  t.shape.assign(shape, shape + ndim);
  t.dev = data;
  c->raw[name] = t;
  return 0;
}

int milan_finalize_weights(milan_ctx* c, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(!c->finalized, MILAN_ERR_STATE, "weights already finalized");
  hipStream_t s = (hipStream_t)stream;
  MILAN_CHECK_HIP(hipSetDevice(c->device));
  set_status_word(nullptr);  // (weight packing is not a saturation event of a call)
  MILAN_TRY(encoder_finalize(c, s));
  MILAN_TRY(classify_finalize(c, s));
  MILAN_TRY(decoder_finalize(c, s));
  MILAN_REQUIRE(c->stem.w || c->lstm_ih.w || c->lm_out.w, MILAN_ERR_STATE,
                "no encoder, decoder or language-model weights were uploaded");
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  c->raw.clear();
  c->finalized = true;
  return 0;
}

size_t milan_workspace_bytes(const milan_ctx* c, int max_neurons, int k,
                             int image_size, int beam_size, int length) {
  if (!c || max_neurons <= 0 || k <= 0) return 0;
  size_t enc = 0, dec = 0;
  if (image_size > 0)
    enc = encoder_workspace(c, max_neurons * k, image_size, image_size);
  dec = decoder_workspace(c, max_neurons, k, beam_size < 1 ? 1 : beam_size,
                          length < 1 ? 1 : length);
  // + an internal features buffer for milan_describe + slack for alignment
  return (enc > dec ? enc : dec) +
         (size_t)max_neurons * k * c->d.feature_size * sizeof(float) + (1 << 16);
}

// Decoder.forward's decode stage behind a hipGraph: the ~450 launches of one
// (n, beam, length, strategy) decode are captured from the stream once (second
// time the same argument tuple -- pointers included -- is seen) and replayed
// with a single hipGraphLaunch afterwards.  Needs a non-default stream and
// pointer-stable buffers (the Python binding keeps them); falls back to direct
// launches while profiling, on the legacy stream, or if capture fails.
struct DecodeCall {
  const float* features; int n, k, strategy, length, beam, mi; float temperature;
  int group; int64_t* tokens; float* scores; float* predictions; float* attentions;
  int64_t* beam_tokens; float* beam_scores; int32_t* out_len; void* ws;
  size_t ws_bytes; hipStream_t stream; int precision; int beam_path;
};

static int decode_direct(milan_ctx* c, const DecodeCall& d) {
  Arena a;
  a.base = (char*)d.ws; a.size = d.ws_bytes; a.off = 0;
  return decoder_decode(c, d.features, d.n, d.k, d.strategy, d.length, d.beam,
                        d.mi, d.temperature, d.group, d.tokens, d.scores,
                        d.predictions, d.attentions, d.beam_tokens, d.beam_scores,
                        d.out_len, a, d.stream);
}

static int decode_maybe_graph(milan_ctx* c, const DecodeCall& d) {
  if (!c->graph_capture || d.stream == nullptr || gemm_profile_active())
    return decode_direct(c, d);
  std::vector<char> key(sizeof(DecodeCall), 0);
  {
    DecodeCall z;
    memset(&z, 0, sizeof(z));  // zero padding bytes before the field copy
    z.features = d.features; z.n = d.n; z.k = d.k; z.strategy = d.strategy;
    z.length = d.length; z.beam = d.beam; z.mi = d.mi;
    z.temperature = d.temperature; z.group = d.group; z.tokens = d.tokens;
    z.scores = d.scores; z.predictions = d.predictions;
    z.attentions = d.attentions; z.beam_tokens = d.beam_tokens;
    z.beam_scores = d.beam_scores; z.out_len = d.out_len; z.ws = d.ws;
    z.ws_bytes = d.ws_bytes; z.stream = d.stream; z.precision = c->precision;
    z.beam_path = c->beam_path;
    memcpy(key.data(), &z, sizeof(z));
  }
  milan_ctx::GraphEntry* e = nullptr;
  for (auto& g : c->graphs)
    if (g.key == key) { e = &g; break; }
  if (e && e->exec) {
    MILAN_CHECK_HIP(hipGraphLaunch(e->exec, d.stream));
    ++c->graph_replays;
    return 0;
  }
  if (!e) {  // first sight: run directly (also sets kernel attributes)
    if (c->graphs.size() >= 16) {
      if (c->graphs.front().exec) (void)hipGraphExecDestroy(c->graphs.front().exec);
      c->graphs.erase(c->graphs.begin());
    }
    milan_ctx::GraphEntry ne;
    ne.key = key; ne.seen = 1;
    c->graphs.push_back(ne);
    return decode_direct(c, d);
  }
  // second sight: capture, instantiate, launch
  hipGraph_t graph = nullptr;
  hipError_t err = hipStreamBeginCapture(d.stream, hipStreamCaptureModeRelaxed);
  if (err != hipSuccess) { (void)hipGetLastError(); return decode_direct(c, d); }
  const int r = decode_direct(c, d);
  err = hipStreamEndCapture(d.stream, &graph);
  if (r != 0 || err != hipSuccess || graph == nullptr) {
    (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
    if (r != 0) return r;
    return decode_direct(c, d);
  }
  hipGraphExec_t exec = nullptr;
  err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (err != hipSuccess || exec == nullptr) {
    (void)hipGetLastError();
    return decode_direct(c, d);
  }
  e->exec = exec;
  ++c->graph_captures;
  MILAN_CHECK_HIP(hipGraphLaunch(exec, d.stream));
  ++c->graph_replays;
  return 0;
}

static int make_arena(void* ws, size_t bytes, Arena* a) {
  MILAN_REQUIRE(ws != nullptr && ((uintptr_t)ws & 255) == 0, MILAN_ERR_WORKSPACE,
                "workspace must be a non-null 256-byte aligned device pointer");
  a->base = (char*)ws;
  a->size = bytes;
  a->off = 0;
  return 0;
}

int milan_encode(milan_ctx* c, const void* images, int image_dtype,
                 const void* masks, int mask_dtype, int n_images, int height,
                 int width, float* features, void* workspace,
                 size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && images && features, MILAN_ERR_ARG, "milan_encode: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_REQUIRE((image_dtype == MILAN_DTYPE_U8 || image_dtype == MILAN_DTYPE_F32) &&
                    (mask_dtype == MILAN_DTYPE_U8 || mask_dtype == MILAN_DTYPE_F32),
                MILAN_ERR_ARG, "bad dtype");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return encoder_run(c, images, image_dtype, masks, mask_dtype, n_images, height,
                     width, features, a, (hipStream_t)stream);
}

int milan_set_ablation(milan_ctx* c, const int32_t* levels, const int32_t* units, int count,
                       milan_stream stream) {
  MILAN_REQUIRE(c && count >= 0 && (count == 0 || (levels && units)), MILAN_ERR_ARG,
                "milan_set_ablation: bad argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_CHECK_HIP(hipSetDevice(c->device));
  return classify_set_ablation(c, levels, units, count, (hipStream_t)stream);
}

int milan_set_alexnet_head(milan_ctx* c, const float* fc6_weight, const float* fc6_bias, int fc6_out,
                           int fc6_in, const float* fc7_weight, const float* fc7_bias,
                           int fc7_out, int fc7_in, const float* linear8_weight,
                           const float* linear8_bias, int linear8_out, int linear8_in,
                           milan_stream stream) {
  MILAN_REQUIRE(c && fc6_weight && fc6_bias && fc7_weight && fc7_bias && linear8_weight &&
                    linear8_bias,
                MILAN_ERR_ARG, "milan_set_alexnet_head: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_CHECK_HIP(hipSetDevice(c->device));
  const float* w[3] = {fc6_weight, fc7_weight, linear8_weight};
  const float* b[3] = {fc6_bias, fc7_bias, linear8_bias};
  const int out[3] = {fc6_out, fc7_out, linear8_out}, in[3] = {fc6_in, fc7_in, linear8_in};
  return classify_set_head(c, *seq_family(MILAN_TRUNK_ALEXNET), w, b, out, in,
                           (hipStream_t)stream);
}

int milan_set_vgg_head(milan_ctx* c, const float* fc0_weight, const float* fc0_bias, int fc0_out,
                       int fc0_in, const float* fc3_weight, const float* fc3_bias, int fc3_out,
                       int fc3_in, const float* fc6_weight, const float* fc6_bias, int fc6_out,
                       int fc6_in, milan_stream stream) {
  MILAN_REQUIRE(c && fc0_weight && fc0_bias && fc3_weight && fc3_bias && fc6_weight && fc6_bias,
                MILAN_ERR_ARG, "milan_set_vgg_head: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_CHECK_HIP(hipSetDevice(c->device));
  const float* w[3] = {fc0_weight, fc3_weight, fc6_weight};
  const float* b[3] = {fc0_bias, fc3_bias, fc6_bias};
  const int out[3] = {fc0_out, fc3_out, fc6_out}, in[3] = {fc0_in, fc3_in, fc6_in};
  return classify_set_head(c, *seq_family(MILAN_TRUNK_VGG), w, b, out, in, (hipStream_t)stream);
}

int milan_vgg_trace(const milan_ctx* c, int32_t* launches, int32_t* split) {
  MILAN_REQUIRE(c && c->d.trunk_kind == MILAN_TRUNK_VGG, MILAN_ERR_ARG,
                "milan_vgg_trace: the context's trunk is not a VGG");
  for (int i = 0; i < 20; ++i) {
    if (launches) launches[i] = c->vgg_launches[i];
    if (split) split[i] = c->vgg_split[i];
  }
  return 0;
}

int milan_set_alexnet_lrn(milan_ctx* c, int local_size, float alpha, float beta) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "milan_set_alexnet_lrn: null argument");
  return classify_set_alexnet_lrn(c, local_size, alpha, beta);
}

int milan_lrn(const float* x, long long pixels, int channels, int split, int local_size,
              float alpha, float beta, float* y, unsigned* status, milan_stream stream) {
  return launch_lrn(x, pixels, channels, split != 0, local_size, alpha, beta, y, status,
                    (hipStream_t)stream);
}

size_t milan_linear_packed_bytes(int n_out, int n_in) {
  if (n_out < 1 || n_in < 1) return 0;
  return sizeof(float) * linear_packed_floats(n_out, n_in);
}

int milan_linear_pack(const float* weight, int n_out, int n_in, float* packed,
                      milan_stream stream) {
  return linear_pack(weight, n_out, n_in, packed, (hipStream_t)stream);
}

int milan_linear(const float* x, const float* packed, const float* bias, int rows, int n_in,
                 int n_out, int relu, float* y, milan_stream stream) {
  return linear_run(x, packed, bias, rows, n_in, n_out, relu != 0, y, (hipStream_t)stream);
}

int milan_linear_rowwise(const float* x, const float* weight, const float* bias, int rows,
                         int n_in, int n_out, float* y, milan_stream stream) {
  return linear_rowwise_run(x, weight, bias, rows, n_in, n_out, y, (hipStream_t)stream);
}

size_t milan_classify_workspace_bytes(const milan_ctx* c, int n_images, int height, int width,
                                      int sweep_units) {
  if (!c || !c->finalized) return 0;
  return classify_workspace(c, n_images, height, width, sweep_units) + 256;
}

int milan_classify(milan_ctx* c, const float* images, int n_images, int height, int width,
                   float* logits, int64_t* predictions, void* workspace, size_t workspace_bytes,
                   milan_stream stream) {
  MILAN_REQUIRE(c && images && (logits || predictions), MILAN_ERR_ARG,
                "milan_classify: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return classify_run(c, images, n_images, height, width, logits, predictions, a,
                      (hipStream_t)stream);
}

int milan_classify_sweep(milan_ctx* c, const float* images, int n_images, int height, int width,
                         const int32_t* levels, const int32_t* units, int count,
                         const int64_t* targets, int32_t* correct, int64_t* predictions,
                         void* workspace, size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && images && count >= 0 && (count == 0 || (levels && units)) &&
                    (correct || predictions) && ((correct != nullptr) == (targets != nullptr)),
                MILAN_ERR_ARG, "milan_classify_sweep: bad argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return classify_sweep(c, images, n_images, height, width, levels, units, count, targets,
                        correct, predictions, a, (hipStream_t)stream);
}

size_t milan_activations_workspace_bytes(const milan_ctx* c, int n_images, int height,
                                         int width) {
  if (!c || !c->finalized) return 0;
  return classify_workspace(c, n_images, height, width, 0) + 256;
}

int milan_activations(milan_ctx* c, const float* images, int n_images, int height, int width,
                      const int32_t* levels, int count, float* const* outputs, void* workspace,
                      size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && images && count >= 1 && levels && outputs, MILAN_ERR_ARG,
                "milan_activations: bad argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return activations_run(c, images, n_images, height, width, levels, count, outputs, a,
                         (hipStream_t)stream);
}

int milan_encode_spatial(milan_ctx* c, const void* images, int image_dtype,
                         const void* masks, int mask_dtype, int n_images,
                         int height, int width, float* out, void* workspace,
                         size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && images && out, MILAN_ERR_ARG,
                "milan_encode_spatial: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_REQUIRE((image_dtype == MILAN_DTYPE_U8 || image_dtype == MILAN_DTYPE_F32) &&
                    (mask_dtype == MILAN_DTYPE_U8 || mask_dtype == MILAN_DTYPE_F32),
                MILAN_ERR_ARG, "bad dtype");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return encoder_run_spatial(c, images, image_dtype, masks, mask_dtype, n_images,
                             height, width, out, a, (hipStream_t)stream);
}

int milan_init_state(milan_ctx* c, const float* features, int n, int k, float* h,
                     float* cc, void* workspace, size_t workspace_bytes,
                     milan_stream stream) {
  MILAN_REQUIRE(c && features && h && cc, MILAN_ERR_ARG, "null argument");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return decoder_init_state(c, features, n, k, h, cc, a, (hipStream_t)stream);
}

int milan_step(milan_ctx* c, const float* features, int rows, int k,
               const int64_t* tokens, const float* h, const float* cc,
               float* h_lm, float* c_lm, float temperature, float* predictions,
               float* attentions, float* h_out, float* c_out, void* workspace,
               size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && features && tokens && h && cc && predictions && h_out && c_out,
                MILAN_ERR_ARG, "milan_step: null argument");
  MILAN_REQUIRE(rows > 0, MILAN_ERR_SHAPE, "milan_step: empty batch");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return decoder_step(c, features, rows, k, tokens, h, cc, h_lm, c_lm,
                      temperature, predictions, attentions, h_out, c_out, a,
                      (hipStream_t)stream);
}

int milan_decode(milan_ctx* c, const float* features, int n, int k, int strategy,
                 int length, int beam_size, int mi, float temperature,
                 int group_size, int64_t* tokens, float* scores,
                 float* predictions, float* attentions, int64_t* beam_tokens,
                 float* beam_scores, int32_t* out_len, void* workspace,
                 size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && features, MILAN_ERR_ARG, "milan_decode: null argument");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  DecodeCall d{features, n, k, strategy, length, beam_size, mi, temperature,
               group_size, tokens, scores, predictions, attentions, beam_tokens,
               beam_scores, out_len, workspace, workspace_bytes,
               (hipStream_t)stream, c->precision};
  return decode_maybe_graph(c, d);
}

int milan_beam_merge(const float* cand_v, const int* cand_i, const float* last_lp, int n,
                     int beam_prev, int beam, int wide, float* new_lp, int* new_tok,
                     int* new_bp, void* workspace, size_t workspace_bytes,
                     milan_stream stream) {
  MILAN_REQUIRE(cand_v && cand_i && new_lp && new_tok && new_bp, MILAN_ERR_ARG,
                "milan_beam_merge: null argument");
  MILAN_REQUIRE(wide == 0 || wide == 1, MILAN_ERR_ARG, "milan_beam_merge: wide=%d", wide);
  (void)workspace; (void)workspace_bytes;  // neither kernel needs scratch
  return decoder_beam_merge(cand_v, cand_i, last_lp, n, beam_prev, beam, wide, new_lp,
                            new_tok, new_bp, (hipStream_t)stream);
}

int milan_row_select(const float* logits, const float* lm_logits, float lambda, int rows,
                     int V, int k, const int64_t* last_tok, int stop, float* cand_v,
                     int* cand_i, int path, milan_stream stream) {
  MILAN_REQUIRE(logits && cand_v && cand_i, MILAN_ERR_ARG, "milan_row_select: null argument");
  MILAN_REQUIRE(path >= 0 && path <= 3, MILAN_ERR_ARG, "milan_row_select: path=%d", path);
  return decoder_row_select(logits, lm_logits, lambda, rows, V, k, last_tok, stop, cand_v,
                            cand_i, path, (hipStream_t)stream);
}

int milan_set_beam_path(milan_ctx* c, int mode) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(mode == 0 || mode == 1, MILAN_ERR_ARG, "unknown beam path mode %d", mode);
  c->beam_path = mode;
  return 0;
}

int milan_get_beam_path(const milan_ctx* c) { return c ? c->beam_path : -1; }

int milan_set_graph_capture(milan_ctx* c, int enable) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  c->graph_capture = enable != 0;
  if (!enable) {
    for (auto& g : c->graphs)
      if (g.exec) (void)hipGraphExecDestroy(g.exec);
    c->graphs.clear();
  }
  return 0;
}

int milan_graph_stats(const milan_ctx* c, long long* captures, long long* replays) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  if (captures) *captures = c->graph_captures;
  if (replays) *replays = c->graph_replays;
  return 0;
}

int milan_lm_score(milan_ctx* c, const int64_t* seqs, int rows, int L,
                   const int32_t* seq_len, float* out, void* workspace,
                   size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && seqs && out, MILAN_ERR_ARG, "milan_lm_score: null argument");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return decoder_lm_score(c, seqs, rows, L, seq_len, out, a, (hipStream_t)stream);
}

int milan_lm_logprobs(milan_ctx* c, const int64_t* seqs, int rows, int L,
                      float* out, void* workspace, size_t workspace_bytes,
                      milan_stream stream) {
  MILAN_REQUIRE(c && seqs && out, MILAN_ERR_ARG,
                "milan_lm_logprobs: null argument");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  return decoder_lm_logprobs(c, seqs, rows, L, out, a, (hipStream_t)stream);
}

int milan_conv2d_nhwc(const float* x, int n, int h, int w, int cin,
                      const float* weight_oihw, const float* bias, int cout,
                      int kh, int kw, int stride, int pad, int relu,
                      const float* residual, float* y, int precision,
                      milan_stream stream) {
  MILAN_REQUIRE(x && weight_oihw && y, MILAN_ERR_ARG, "conv2d: null argument");
  set_status_word(nullptr);  // ctx-less entry point: nobody listens for saturation here
  // precision 3 (test hook only): split-f16 with the LDS-strip 3x3 kernel forced;
  // precision 4 (test hook only): split-f16 with k in tap-major order (GemmArgs::Wt unset);
  // precision 5 (test hook only): tap-inner, tiles in linear order (GemmArgs::tap_ncls = -1):
  // what MILAN_TAP_SKIP=0 runs
  const bool force_strip = precision == 3, tap_major = precision == 4, tap_linear = precision == 5;
  if (force_strip || tap_major || tap_linear) precision = MILAN_PRECISION_SPLIT_F16;
  MILAN_REQUIRE(!force_strip || MILAN_EXPERIMENTS, MILAN_ERR_ARG,
                "conv2d: the LDS-strip 3x3 kernel is only in an experiments build "
                "(make EXPERIMENTS=1)");
  MILAN_REQUIRE(precision == MILAN_PRECISION_F32 || cin % 32 == 0,
                MILAN_ERR_SHAPE, "conv2d: split-f16 needs cin %% 32 == 0");
  MILAN_REQUIRE(cin % 4 == 0 && n > 0 && cout > 0, MILAN_ERR_SHAPE,
                "conv2d: cin must be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  const int K = kh * kw * cin, Kp = (K + 31) / 32 * 32;
  float *wp = nullptr, *zero = nullptr, *xs = nullptr, *wsp = nullptr, *ws3 = nullptr, *wst = nullptr;
  MILAN_CHECK_HIP(hipMalloc((void**)&wp, sizeof(float) * (size_t)cout * Kp));
  MILAN_CHECK_HIP(hipMalloc((void**)&zero, 256));
  MILAN_CHECK_HIP(hipMemsetAsync(zero, 0, 256, s));
  int r = pack_conv_plain(weight_oihw, cout, cin, kh, kw, wp, s);
  if (r == 0) {
    GemmArgs g{};
    const int ho = (h + 2 * pad - kh) / stride + 1, wo = (w + 2 * pad - kw) / stride + 1;
    g.A = x; g.W = wp; g.bias = bias; g.aux = residual; g.C = y;
    g.M = n * ho * wo; g.N = cout; g.K = K; g.Kp = Kp; g.ldc = cout; g.ldaux = cout;
    g.H = h; g.Wd = w; g.Cin = cin; g.Ho = ho; g.Wo = wo; g.KH = kh; g.KW = kw;
    g.stride = stride; g.pad = pad; g.a_pix_stride = cin;
    g.a_img_stride = (long)h * w * cin;
    g.epilogue = residual ? EPI_BIAS_RES_RELU : (relu ? EPI_BIAS_RELU : EPI_BIAS);
    g.zero = zero;
    if (precision == MILAN_PRECISION_SPLIT_F16) {
      const long rows = (long)n * h * w;
      hipError_t e1 = hipMalloc((void**)&xs, sizeof(float) * (size_t)rows * cin);
      hipError_t e2 = hipMalloc((void**)&wsp, sizeof(float) * (size_t)cout * Kp);
      if (e1 != hipSuccess || e2 != hipSuccess) {
        set_error("conv2d: out of memory");
        r = (int)hipErrorOutOfMemory;
      } else {
        r = launch_f32_to_split(x, cin, xs, cin, rows, cin, 1.f, s);
        if (r == 0)
          r = split_weight_into(wp, cout, Kp, wsp, &g.acc_scale,
                                reinterpret_cast<unsigned int*>(zero) + 32, s);
        g.A = xs; g.W = wsp; g.a_split = 1;
        if (r == 0 && !tap_major && kh * kw > 1 && kh * kw <= 32 && K == Kp) {
          // the trunk's k x k convs run in (slice, tap, channel) order: test that one
          if (hipMalloc((void**)&wst, sizeof(float) * (size_t)cout * Kp) == hipSuccess) {
            r = make_slice_major(wsp, cout, kh * kw, cin, 4, 2, wst, s);
            g.Wt = wst;
            if (tap_linear) g.tap_ncls = -1;
          }
        }
        if (MILAN_EXPERIMENTS && r == 0 && kh == 3 && kw == 3 && stride == 1 &&
            pad == 1 && K == Kp) {
          // the trunk's 3x3 convs run on the LDS-strip kernel: test it the same way
          if (hipMalloc((void**)&ws3, sizeof(float) * (size_t)cout * Kp) == hipSuccess) {
            r = make_chunk_major(wsp, cout, cin, ws3, s);
            g.W3 = ws3;
            if (force_strip) g.tile_hint = 8;
          }
        }
      }
    }
    if (r == 0) r = launch_gemm(g, s);
  }
  hipError_t e = hipStreamSynchronize(s);
  (void)hipFree(wp);
  (void)hipFree(zero);
  if (xs) (void)hipFree(xs);
  if (wsp) (void)hipFree(wsp);
  if (ws3) (void)hipFree(ws3);
  if (wst) (void)hipFree(wst);
  if (r == 0 && e != hipSuccess) {
    set_error("conv2d: %s", hipGetErrorString(e));
    r = (int)e;
  }
  return r;
}

int milan_gemm_probe(const milan_gemm_probe_args* d, milan_stream stream) {
  MILAN_REQUIRE(d && d->A && d->weight && d->C, MILAN_ERR_ARG, "gemm_probe: null argument");
  MILAN_REQUIRE(!d->f16 && d->epilogue >= EPI_BIAS && d->epilogue <= EPI_BIAS_ADD, MILAN_ERR_ARG,
                "gemm_probe: fast mode and the LSTM / log-sum-exp epilogues are not probed "
                "(f16=%d epilogue=%d)", d->f16, d->epilogue);
  MILAN_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->groups >= 0 && d->groups <= 65535,
                MILAN_ERR_ARG, "gemm_probe: M=%d N=%d K=%d groups=%d", d->M, d->N, d->K, d->groups);
  set_status_word(nullptr);  // (weight packing is not a saturation event of the launch)
  hipStream_t s = (hipStream_t)stream;
  const int groups = d->groups > 1 ? d->groups : 1, taps = d->KH * d->KW;
  const int Kp = (d->K + 31) / 32 * 32;
  const long rows = (long)groups * d->N;
  const size_t wbytes = sizeof(float) * (size_t)rows * Kp;
  float *wp = nullptr, *zero = nullptr, *wsp = nullptr, *wst = nullptr;
  MILAN_CHECK_HIP(hipMalloc((void**)&wp, wbytes));
  int r = (int)hipMalloc((void**)&zero, 256);
  if (r == 0) r = (int)hipMemsetAsync(zero, 0, 256, s);
  // rows of K floats -> rows of Kp, zero padded
  if (r == 0) r = (int)hipMemsetAsync(wp, 0, wbytes, s);
  if (r == 0)
    r = (int)hipMemcpy2DAsync(wp, sizeof(float) * Kp, d->weight, sizeof(float) * d->K,
                              sizeof(float) * d->K, rows, hipMemcpyDeviceToDevice, s);
  if (r != 0) set_error("gemm_probe: %s", hipGetErrorString((hipError_t)r));
  GemmArgs g{};
  g.A = static_cast<const float*>(d->A); g.W = wp; g.bias = d->bias;
  g.aux = static_cast<const float*>(d->aux); g.C = static_cast<float*>(d->C);
  g.M = d->M; g.N = d->N; g.K = d->K; g.Kp = Kp; g.ldc = d->ldc; g.ldaux = d->ldaux;
  g.H = d->H; g.Wd = d->Wd; g.Cin = d->Cin; g.Ho = d->Ho; g.Wo = d->Wo; g.KH = d->KH; g.KW = d->KW;
  g.stride = d->stride; g.pad = d->pad;
  g.a_pix_stride = d->a_pix_stride; g.a_img_stride = d->a_img_stride;
  g.epilogue = d->epilogue; g.zero = zero;
  g.a_split = d->a_split; g.out_split = d->out_split; g.aux_split = d->aux_split;
  g.A2 = static_cast<const float*>(d->A2); g.K1 = d->K1; g.H2 = d->H2; g.W2d = d->W2d;
  g.stride2 = d->stride2; g.a2_pix_stride = d->a2_pix_stride; g.a2_img_stride = d->a2_img_stride;
  g.aniso = d->aniso; g.stride_w = d->stride_w; g.pad_w = d->pad_w;
  g.m_live = d->m_live; g.row_list = d->row_list; g.m_live_mul = d->m_live_mul;
  g.tap_ncls = d->tap_ncls;
  g.groups = d->groups;
  g.a_grp = d->a_grp; g.w_grp = (long)d->N * Kp; g.bias_grp = d->bias_grp; g.c_grp = d->c_grp;
  g.aux_grp = d->aux_grp;
  if (r == 0 && d->a_split) {
    // what pack_conv (encoder.hip) makes of a conv's packed rows
    r = (int)hipMalloc((void**)&wsp, wbytes);
    if (r != 0) set_error("gemm_probe: out of memory");
    if (r == 0)
      r = split_weight_into(wp, (int)rows, Kp, wsp, &g.acc_scale,
                            reinterpret_cast<unsigned int*>(zero) + 32, s);
    g.W = wsp;
    if (r == 0 && !d->no_wt && taps > 1 && taps <= 32 && d->K == Kp && d->Cin % 32 == 0) {
      r = (int)hipMalloc((void**)&wst, wbytes);
      if (r != 0) set_error("gemm_probe: out of memory");
      if (r == 0) r = make_slice_major(wsp, (int)rows, taps, d->Cin, 4, 2, wst, s);
      g.Wt = wst;
    }
  }
  if (r == 0) {
    set_status_word(d->status);
    r = launch_gemm(g, s);
  }
  hipError_t e = hipStreamSynchronize(s);
  // (the word is the caller's memory: a later ctx-less call must not report into it)
  set_status_word(nullptr);
  (void)hipFree(wp);
  if (zero) (void)hipFree(zero);
  if (wsp) (void)hipFree(wsp);
  if (wst) (void)hipFree(wst);
  if (r == 0 && e != hipSuccess) {
    set_error("gemm_probe: %s", hipGetErrorString(e));
    r = (int)e;
  }
  return r;
}

int milan_set_fusion(milan_ctx* c, int flags) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE((flags & ~(MILAN_FUSE_CHAIN | MILAN_FUSE_CHAIN_WIDE | MILAN_FUSE_STEM | MILAN_FUSE_CONV3 |
                           MILAN_FUSE_SKIP_EMPTY | MILAN_FUSE_BNECK | MILAN_FUSE_SPARSE_TAIL |
                           MILAN_FUSE_TAIL_LISTS)) == 0, MILAN_ERR_ARG,
                "unknown fusion flags %d", flags);
  MILAN_REQUIRE(!(flags & MILAN_FUSE_TAIL_LISTS) || (flags & MILAN_FUSE_SPARSE_TAIL), MILAN_ERR_ARG,
                "MILAN_FUSE_TAIL_LISTS needs MILAN_FUSE_SPARSE_TAIL (flags %d)", flags);
  c->fusion = flags;
  return 0;
}

int milan_set_image_sharing(milan_ctx* c, int enable) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  c->share_images = enable != 0;
  return 0;
}

int milan_get_image_sharing(const milan_ctx* c) { return c ? c->share_images : -1; }

int milan_image_sharing_stats(milan_ctx* c, long long* slots, long long* trunk_images, int clear,
                              milan_stream stream) {
  MILAN_REQUIRE(c && slots && trunk_images, MILAN_ERR_ARG,
                "milan_image_sharing_stats: null argument");
  hipStream_t s = (hipStream_t)stream;
  long long host[2] = {0, 0};
  MILAN_CHECK_HIP(hipMemcpyAsync(host, c->share_stats, sizeof(host), hipMemcpyDeviceToHost, s));
  if (clear) MILAN_TRY(launch_zero_fill(c->share_stats, sizeof(host), s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  *slots = host[0];
  *trunk_images = host[1];
  return 0;
}

int milan_set_precision(milan_ctx* c, int precision) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(precision == MILAN_PRECISION_F32 || precision == MILAN_PRECISION_SPLIT_F16 ||
                    precision == MILAN_PRECISION_F16,
                MILAN_ERR_ARG, "unknown precision mode %d", precision);
  // fast mode = split-f16 everywhere except layer3 / layer4 of a bottleneck trunk
  c->trunk_f16 = precision == MILAN_PRECISION_F16;
  c->precision = c->trunk_f16 ? MILAN_PRECISION_SPLIT_F16 : precision;
  return 0;
}

int milan_get_precision(const milan_ctx* c) {
  return c ? (c->trunk_f16 ? MILAN_PRECISION_F16 : c->precision) : -1;
}

int milan_profile_enable(int enable) { return gemm_profile_enable(enable); }

int milan_profile_read(double* gemm_ms, double* gemm_flops,
                       long long* gemm_launches) {
  return gemm_profile_read(gemm_ms, gemm_flops, gemm_launches);
}

int milan_profile_read_stages(double* table) {
  MILAN_REQUIRE(table, MILAN_ERR_ARG, "milan_profile_read_stages: null table");
  return profile_read_stages(table);
}

int milan_profile_read_kernels(double* table) {
  MILAN_REQUIRE(table, MILAN_ERR_ARG, "milan_profile_read_kernels: null table");
  return profile_read_kernels(table);
}

int milan_status(milan_ctx* c, uint32_t* flags, int clear, milan_stream stream) {
  MILAN_REQUIRE(c && flags, MILAN_ERR_ARG, "milan_status: null argument");
  hipStream_t s = (hipStream_t)stream;
  unsigned host = 0;
  MILAN_CHECK_HIP(hipMemcpyAsync(&host, c->status, sizeof(host), hipMemcpyDeviceToHost, s));
  if (clear) MILAN_CHECK_HIP(hipMemsetAsync(c->status, 0, sizeof(unsigned), s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  *flags = host;
  return 0;
}

int milan_set_act_scale_log2(milan_ctx* c, int k, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(k >= 0 && k <= 10, MILAN_ERR_ARG,
                "activation scale 2^%d outside 2^0 .. 2^10", k);
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  c->act_scale = ldexpf(1.f, k);
  c->act_scale_log2 = k;
  // captured decode graphs do not hold trunk launches; nothing else caches the scale
  return encoder_rescale(c, (hipStream_t)stream);
}

int milan_get_act_scale_log2(const milan_ctx* c) { return c ? c->act_scale_log2 : -1; }

int milan_set_feature_scale_log2(milan_ctx* c, int k, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(k >= -MILAN_FEATURE_SCALE_LOG2_MAX && k <= MILAN_FEATURE_SCALE_LOG2_MAX,
                MILAN_ERR_ARG, "feature scale 2^%d outside 2^-%d .. 2^%d", k,
                MILAN_FEATURE_SCALE_LOG2_MAX, MILAN_FEATURE_SCALE_LOG2_MAX);
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  if (k == c->feat_scale_log2) return 0;
  // (the operand scale and the weight copy move together: a failed resplit restores the old
  // scale and rebuilds the old copy)
  const int old = c->feat_scale_log2;
  c->feat_scale = ldexpf(1.f, k);
  c->feat_scale_log2 = k;
  const int r = resplit_lstm_cats(c, (hipStream_t)stream);
  if (r != 0) {
    c->feat_scale = ldexpf(1.f, old);
    c->feat_scale_log2 = old;
    (void)resplit_lstm_cats(c, (hipStream_t)stream);
  }
  return r;
}

int milan_get_feature_scale_log2(const milan_ctx* c) { return c ? c->feat_scale_log2 : 0; }

float milan_get_feature_absmax(const milan_ctx* c) { return c ? c->feat_absmax : 0.f; }

int milan_set_embedding_scale_log2(milan_ctx* c, int k, milan_stream stream) {
  MILAN_REQUIRE(c, MILAN_ERR_ARG, "null ctx");
  MILAN_REQUIRE(k >= -MILAN_FEATURE_SCALE_LOG2_MAX && k <= MILAN_FEATURE_SCALE_LOG2_MAX,
                MILAN_ERR_ARG, "embedding scale 2^%d outside 2^-%d .. 2^%d", k,
                MILAN_FEATURE_SCALE_LOG2_MAX, MILAN_FEATURE_SCALE_LOG2_MAX);
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  if (k == c->emb_scale_log2) return 0;
  const int old = c->emb_scale_log2;
  c->emb_scale = ldexpf(1.f, k);
  c->emb_scale_log2 = k;
  const int r = resplit_lstm_cats(c, (hipStream_t)stream);
  if (r != 0) {  // (as milan_set_feature_scale_log2)
    c->emb_scale = ldexpf(1.f, old);
    c->emb_scale_log2 = old;
    (void)resplit_lstm_cats(c, (hipStream_t)stream);
  }
  return r;
}

int milan_get_embedding_scale_log2(const milan_ctx* c) { return c ? c->emb_scale_log2 : 0; }

float milan_get_embedding_absmax(milan_ctx* c) {
  // largest |entry| of the decoder's and the LM's embedding table (legacy stream, synchronous)
  if (!c || !c->finalized) return 0.f;
  if (c->emb_absmax > 0.f) return c->emb_absmax;
  if (hipSetDevice(c->device) != hipSuccess) return 0.f;
  // (a word of its own next to the status word -- not the split conversion's scratch, which a
  // call on another stream may be using; the tables never change after finalize)
  unsigned int* d_max = c->status + 10;
  if (hipMemset(d_max, 0, sizeof(unsigned int)) != hipSuccess) return 0.f;
  const float* tables[2] = {c->embedding, c->lm_embedding};
  const long sizes[2] = {(long)c->d.vocab_size * c->d.embedding_size,
                         (long)c->d.vocab_size * c->d.lm_embedding_size};
  for (int i = 0; i < 2; ++i)
    if (tables[i])
      hipLaunchKernelGGL(absmax_kernel, dim3(256), dim3(256), 0, nullptr, tables[i], sizes[i],
                         d_max);
  unsigned bits = 0;
  if (hipMemcpy(&bits, d_max, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess) return 0.f;
  memcpy(&c->emb_absmax, &bits, sizeof(float));
  return c->emb_absmax;
}

int milan_encoder_absmax(milan_ctx* c, const void* images, int image_dtype, int n_images,
                         int height, int width, float* absmax, void* workspace,
                         size_t workspace_bytes, milan_stream stream) {
  MILAN_REQUIRE(c && images && absmax, MILAN_ERR_ARG, "milan_encoder_absmax: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_REQUIRE(c->d.trunk_kind == MILAN_TRUNK_BOTTLENECK || c->d.trunk_kind == MILAN_TRUNK_BASIC,
                MILAN_ERR_ARG, "calibration covers the ResNet trunks (the others keep scale 1)");
  hipStream_t s = (hipStream_t)stream;
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  float* feats = a.get<float>((size_t)n_images * c->d.feature_size);
  MILAN_REQUIRE(feats, MILAN_ERR_WORKSPACE, "absmax: workspace too small");
  Arena enc;
  enc.base = a.base + a.off; enc.size = a.size - a.off; enc.off = 0;
  unsigned* word = c->status + 8;   // [0] activations, [1] what bounds the features
  MILAN_CHECK_HIP(hipMemsetAsync(word, 0, 2 * sizeof(unsigned), s));
  const int saved = c->precision;
  c->precision = MILAN_PRECISION_F32;
  c->calib = word;
  set_status_word(nullptr);
  const int r = encoder_run(c, images, image_dtype, nullptr, MILAN_DTYPE_U8, n_images, height,
                            width, feats, enc, s);
  c->calib = nullptr;
  c->precision = saved;
  MILAN_TRY(r);
  // ... and next to it what bounds the FEATURES under any mask (the decoder's feature scale
  // is picked from it): a pooled feature is a mask-weighted mean of tap activations, so the
  // largest |value| of the five taps bounds it.  Taps 1..4 are activations counted above;
  // tap 0, the raw conv1 output, was folded into this word by the pass; the unmasked
  // features of the sample join for good measure.
  unsigned* fword = word + 1;
  {
    const long total = (long)n_images * c->d.feature_size;
    const long blocks = (total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024;
    hipLaunchKernelGGL(absmax_kernel, dim3((int)(blocks < 1 ? 1 : blocks)), dim3(256), 0, s,
                       feats, total, fword);
    MILAN_CHECK_HIP(hipGetLastError());
  }
  unsigned bits[2] = {0, 0};
  MILAN_CHECK_HIP(hipMemcpyAsync(bits, word, sizeof(bits), hipMemcpyDeviceToHost, s));
  MILAN_CHECK_HIP(hipStreamSynchronize(s));
  memcpy(absmax, &bits[0], sizeof(float));
  memcpy(&c->feat_absmax, &bits[1], sizeof(float));
  if (*absmax > c->feat_absmax) c->feat_absmax = *absmax;
  return 0;
}

int milan_describe(milan_ctx* c, const void* images, int image_dtype,
                   const void* masks, int mask_dtype, int n, int k, int height,
                   int width, int strategy, int length, int beam_size, int mi,
                   float temperature, int group_size, float* features_out,
                   int64_t* tokens, float* scores, float* predictions,
                   float* attentions, int64_t* beam_tokens, float* beam_scores,
                   int32_t* out_len, void* workspace, size_t workspace_bytes,
                   milan_stream stream) {
  MILAN_REQUIRE(c && images, MILAN_ERR_ARG, "milan_describe: null argument");
  MILAN_REQUIRE(c->finalized, MILAN_ERR_STATE, "weights not finalized");
  MILAN_REQUIRE(n > 0 && k > 0, MILAN_ERR_SHAPE, "milan_describe: empty batch");
  set_status_word(c->status);
  Arena a;
  MILAN_TRY(make_arena(workspace, workspace_bytes, &a));
  const size_t fcount = (size_t)n * k * c->d.feature_size;
  float* feats = features_out;
  if (!feats) {
    feats = a.get<float>(fcount);
    MILAN_REQUIRE(feats, MILAN_ERR_WORKSPACE, "describe: workspace too small");
  }
  // encoder and decoder scratch reuse the same region one after the other
  Arena enc;
  enc.base = a.base + a.off; enc.size = a.size - a.off; enc.off = 0;
  MILAN_TRY(encoder_run(c, images, image_dtype, masks, mask_dtype, n * k, height,
                        width, feats, enc, (hipStream_t)stream));
  DecodeCall d{feats, n, k, strategy, length, beam_size, mi, temperature,
               group_size, tokens, scores, predictions, attentions, beam_tokens,
               beam_scores, out_len, enc.base, enc.size, (hipStream_t)stream,
               c->precision};
  return decode_maybe_graph(c, d);
}

}  // extern "C"
