// Shared host-side declarations for libmilan_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <map>

#include "../../include/milan_hip.h"
// Epilogue, GemmArgs, shift_group, OutMode and the launch plan that reads them (gemm_plan.h);
// ConvW, Bottleneck, ChainArgs, Arena, the conv argument builders, the fused kernels' shape
// predicates and the schedule of an encoder pass (enc_plan.h)
#include "enc_plan.h"

// experiments build (make EXPERIMENTS=1): measured-and-rejected kernels and the
// knobs that force tile configurations; see gemm.hip and DESIGN.md section 5
#ifndef MILAN_EXPERIMENTS
#define MILAN_EXPERIMENTS 0
#endif

namespace milan {

// ---- error plumbing (no C++ exceptions cross the C ABI) --------------------
void set_error(const char* fmt, ...);
#define MILAN_CHECK_HIP(expr)                                              \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                \
      milan::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,       \
                       hipGetErrorString(_e));                             \
      return (int)_e;                                                      \
    }                                                                      \
  } while (0)
#define MILAN_REQUIRE(cond, code, ...)                                     \
  do {                                                                     \
    if (!(cond)) {                                                         \
      milan::set_error(__VA_ARGS__);                                       \
      return (code);                                                       \
    }                                                                      \
  } while (0)
#define MILAN_TRY(expr)                                                    \
  do {                                                                     \
    int _r = (expr);                                                       \
    if (_r != 0) return _r;                                                \
  } while (0)

// ---- implicit-GEMM (conv / linear): GemmArgs and the plan of a launch are in gemm_plan.h ----
int launch_gemm(const GemmArgs& g, hipStream_t s);
// whether launch_gemm() can run `g` on a row list (GemmArgs::row_list) with the bits of the
// dense launch: whether its plan names a pp32l form (gemm_plan.h)
bool row_list_supported(const GemmArgs& g);
// the knobs of the launch path, read once per process, with the current device's CU count
int gemm_env(GemmEnv* out);
// Status word of the context whose entry point is running on this thread (api.hip sets it
// on entry): every kernel that writes split format ORs MILAN_STATUS_SATURATED into it when
// its clamp to +-65504 was hit (split8_* below).  nullptr = nobody is listening.
void set_status_word(unsigned* word);
unsigned* status_word();
// kernel family of the GEMM-class launch being recorded (milan_profile_read_kernels)
void profile_tag_kernel(int family);
// rows x K fp32 (row stride ld_src) -> split format (row stride ld_dst), x scale
// Zero `bytes` (a multiple of 4, 4-byte aligned) on the stream with a KERNEL.  Not
// hipMemsetAsync: as a node of a captured graph (round 6: whole passes can be captured) the
// runtime's fill replayed a recycled 16-byte pattern from the second replay on (ROCm 7.2; the
// feature rows of empty-mask exemplars and the LM's initial state came back as garbage:
// tools/graph_describe.py, tests/test_gpu_skip_empty.py).
int launch_zero_fill(void* p, size_t bytes, hipStream_t s);
// A NaN crosses as an f16 NaN in `hi` (not a saturation); with `nanrow` it leaves as 0 and
// nanrow[row] = stamp marks its row instead.
int launch_f32_to_split(const float* src, long ld_src, float* dst, long ld_dst,
                        long rows, int K, float scale, hipStream_t s, int* nanrow = nullptr,
                        int stamp = 0);
int gemm_profile_enable(int enable);
// per-device launch state (gemm.hip): dynamic-LDS opt-in of a kernel, CU count in octets
int ensure_lds_attr(const void* kern, int bytes);
int device_cus8(int* out);
void* gemm_profile_begin(double flops, double bytes, hipStream_t s);
void gemm_profile_end(void* rec, hipStream_t s);

// ---- image sharing (share.hip; milan_set_image_sharing) ---------------------------------
// Classes of byte-identical uint8 images among the n slots of one encoder pass, all on the
// device: order[c] = root image of live class c (ascending), *count = live classes,
// class_of[i] = trunk slot of exemplar slot i (-1: nothing to pool), bbox_c[c] = union of the
// members' level-0 bounding boxes.
struct ShareArgs {
  const unsigned char* images;  // [n][bytes]
  long bytes;                   // 3 * H * W
  int n;
  int hash_bits;                // low bits of the hash that select candidates (MILAN_SHARE_HASH_BITS)
  int skip_empty;               // 0: every class is live
  const int* list_n;            // [n][5] (mask_pyramid_kernel)
  const int* bbox;              // [n][4]
  void* hash;                   // [n] 8 bytes each
  int *rep, *flag;              // [n] scratch
  int *order, *bbox_c, *count, *class_of;
};
int launch_image_classes(const ShareArgs& a, hipStream_t s);
// stats[0] += n, stats[1] += *live (n when live == nullptr); one thread, nothing read back
int launch_share_count(long long* stats, int n, const int* live, hipStream_t s);

// ---- fused expand -> reduce chain (chain.hip): ChainArgs and chain_supported() are in enc_plan.h
int launch_chain(const ChainArgs& a, hipStream_t s);
// ---- fused split-f16 stem (stem.hip): conv1 7x7/2 + bn1 + ReLU + maxpool 3x3/2 ----
struct StemArgs {
  const float* in;      // pixel-pair groups [n][H][G][hi x8 | lo x8] (encoder.hip)
  const float* ws;      // split weights [64][224] (pack_stem_pairs), scaled
  const float* bias;    // [64] or nullptr
  float acc_scale;      // 1 / weight scale
  const float* scale;   // bn1 folded: y = x * scale + shift
  const float* shift;
  float* raw;           // [n][h1][w1][64] fp32 conv1 output (pyramid level 0) or nullptr
  float* y;             // [n][hp][wp][64] split format
  const int* bbox;      // [n][4] = y0, y1, x0, x1 (inclusive) of the conv1 pixels the
                        // level-0 pooling reads, or nullptr = write every raw pixel
  const float* zero;    // >= 64 B of zeros
  int n, H, G, h1, w1, hp, wp;
  int tiles_y, tiles_x;  // filled by the launcher
  int debug;             // timing experiments: 1 no MFMA, 2 no store phase, 4 no DMA, 8 no staging
  unsigned* status;      // filled by the launcher (status_word())
  // uint8 images straight into the stem (round 5): when in_u8 != nullptr the kernel reads the
  // NCHW bytes of its input tile itself and turns them into pixel-pair groups through `lut`
  // (3 x 256 + 1 entries: hi | lo << 16 of the normalised value of byte v in channel c at
  // c * 256 + v, entry 768 = 0 for the padding) -- bit for bit what preprocess_pairs_kernel
  // writes, without the 32-bytes-per-pixel-pair tensor `in` (unused then)
  const unsigned char* in_u8;
  const unsigned* lut;
  const int* order;      // batch slot -> image number (encoder.hip, MILAN_FUSE_SKIP_EMPTY) or nullptr
  int W;
  const int* n_live;     // device-side image count (<= n) or nullptr, see GemmArgs::m_live
};
int launch_stem_fused(const StemArgs& a, hipStream_t s);
// ---- 3x3 / 1 / 1 convolution, 64 -> 64 channels, weights in registers (conv3.hip) ----
struct Conv3Args {
  const float* in;     // [n][h][w][64] split format
  const float* ws;     // split weights [64][576] (k = tap * 64 + channel), scaled
  const float* bias;   // [64] or nullptr
  float acc_scale;     // 1 / weight scale
  float* out;          // [n][h][w][64] split format: relu(conv + bias)
  const float* zero;   // >= 64 B of zeros
  int n, h, w;
  int tiles_y, tiles_x;  // filled by the launcher
  int debug;             // timing experiments: 1 no MFMA, 2 no epilogue, 4 no DMA, 8 no hand-over
  long long* prof;       // experiments build: per-phase cycle sums of workgroup 0 (16 values)
  unsigned* status;      // filled by the launcher (status_word())
  const int* n_live;     // device-side image count (<= n) or nullptr, see GemmArgs::m_live
};
int launch_conv3_p64(const Conv3Args& a, hipStream_t s);
bool gemm_profile_active();
int gemm_profile_read(double* ms, double* flops, long long* launches);
int profile_read_stages(double* table /* [MILAN_STAGE_COUNT][6] */);
int profile_read_kernels(double* table /* [MILAN_KERNEL_COUNT][4] */);
// RAII bracket of one stage region on a stream: labels the GEMM launches made
// inside it and, while profiling is on, times the region with two HIP events.
class StageScope {
 public:
  StageScope(int stage, hipStream_t s);
  ~StageScope();
  StageScope(const StageScope&) = delete;
  StageScope& operator=(const StageScope&) = delete;
 private:
  hipStream_t stream_;
  int prev_;
  long idx_;
};

// torch's LSTM cell, gate order i, f, g, o (one definition for the pointwise
// kernel and the fused GEMM epilogue, roundings spelled out, so that both give
// the same bits)
__device__ __forceinline__ void lstm_cell(float pi, float pf, float pg, float po,
                                          float c_in, float* h, float* c) {
  const float gi = 1.f / (1.f + expf(-pi));
  const float gf = 1.f / (1.f + expf(-pf));
  const float gg = tanhf(pg);
  const float go = 1.f / (1.f + expf(-po));
  const float c2 = __fmaf_rn(gi, gg, __fmul_rn(gf, c_in));
  *c = c2;
  *h = __fmul_rn(go, tanhf(c2));
}
// row of gate `gate` (0..3 = i, f, g, o), hidden unit u, in the gate-interleaved
// order EPI_LSTM expects: 64-row groups [i x16 | f x16 | g x16 | o x16]
__host__ __device__ inline int lstm_interleaved_row(int gate, int u) {
  return (u >> 4) * 64 + gate * 16 + (u & 15);
}


// ---- packed weights (ConvW, Bottleneck: enc_plan.h) ---------------------------
struct LinearW {
  float* w = nullptr;  // [N][Kp]
  float* ws = nullptr; // split-f16 copy (nullptr when K % 32 != 0)
  float ws_inv = 1.f;
  float* b = nullptr;
  int n = 0, k = 0, kp = 0;
  bool gate_interleaved = false;  // rows permuted for EPI_LSTM (cat weights)
};

struct Tensor {
  std::vector<int64_t> shape;
  const float* dev = nullptr;  // caller-owned device pointer (until finalize)
  int64_t numel() const {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    return n;
  }
};

// ---- device-side row / image counts (GemmArgs::m_live) --------------------------------
// min(bound, *live * mul) through a SCALAR load (constant address space: the word was
// written by an earlier kernel of the same stream and does not change while this one runs;
// the scalar cache is invalidated at every dispatch, as for the kernel arguments).
__device__ __forceinline__ int live_rows(const int* live, int mul, int bound) {
  if (live == nullptr) return bound;
  typedef const int __attribute__((address_space(4)))* KWord;
  const long v = (long)*(KWord)(uintptr_t)live * mul;
  return v < bound ? (int)v : bound;
}

// ---- split-f16 storage format, device side (one implementation for every kernel) -----
// 8 fp32 -> (hi, lo) f16x8 pair; hi saturates instead of overflowing to inf:
//   x = min(max(v, -65504), 65504);  hi = f16(x);  lo = f16(x - float(hi))
// spelled with the instructions that do two of these steps at once -- v_med3_f32 (the
// clamp), v_cvt_pk_f16_f32 (two roundings to f16, RNE), v_fma_mix_f32 (x - float(hi): the
// f16 -> f32 conversion inside it is exact, so the one rounding is the subtraction's) --
// 20 instructions per 8 values instead of 48, the same bits (tests/test_gpu_chain.py and
// the token hash of the bench workload pin that).  V4 = any 4 x 32-bit vector type.
__device__ __forceinline__ float cvt_pk_f16(float a, float b) {
  float r;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <int SEL>   // x - float(f16 half SEL of hpair)
__device__ __forceinline__ float mix_sub_f16(float x, float hpair) {
  float r;
  if constexpr (SEL == 0)
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(x));
  else
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hpair), "v"(x));
  return r;
}
template <int SEL>   // float(f16 half SEL of hpair) + float(f16 half SEL of lpair)
__device__ __forceinline__ float mix_add_f16(float hpair, float lpair) {
  float r;
  if constexpr (SEL == 0)
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(hpair), "v"(lpair));
  else
    asm("v_fma_mix_f32 %0, %1, 1.0, %2 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(hpair), "v"(lpair));
  return r;
}
// Saturation is LOUD (round 5): every thread keeps the running maximum `sat` of the clamped
// magnitudes it has split (four v_max3_f32 per 8 values, no compare, no scalar traffic);
// `sat >= 65504` at the end of the kernel means a value hit the clamp (or was exactly the
// largest f16) and the kernel ORs MILAN_STATUS_SATURATED into the context's status word
// (report_saturation).  The host raises / falls back to f32 (milan_amd/hip.py).
// NaN: v_med3_f32 returns min3 when an operand is NaN, so a NaN accumulator leaves as 0 (ReLU
// form) or -65504 (plain form).  A NaN cannot ARISE inside the trunk without a saturation
// first (|x| > 65504 / act_scale is flagged long before fp32 overflows to Inf - Inf), and a
// non-finite INPUT pixel poisons its whole image in the reference (every pyramid level pools
// NaN x mask) -- that is reproduced at image level: preprocess_* marks the image, the pooling
// / spatial read-out write NaN for it (encoder.hip, MILAN_STATUS_NONFINITE_INPUT).
__device__ __forceinline__ float max3_abs(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float sat_fold8(const float* x, float sat) {
  return max3_abs(max3_abs(x[0], x[1], x[2]), max3_abs(x[3], x[4], x[5]), max3_abs(x[6], x[7], sat));
}
__device__ __forceinline__ void report_saturation(unsigned* status, float sat) {
  if (status != nullptr && sat >= 65504.f) atomicOr(status, 1u /* MILAN_STATUS_SATURATED */);
}
template <typename V4>
__device__ __forceinline__ void split8_rne(const float* v, V4* hi_out, V4* lo_out, float* sat = nullptr) {
  V4 hi, lo;
  float x[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(x[2 * d]) : "v"(v[2 * d]), "v"(-65504.f), "v"(65504.f));
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(x[2 * d + 1]) : "v"(v[2 * d + 1]), "v"(-65504.f), "v"(65504.f));
    hi[d] = cvt_pk_f16(x[2 * d], x[2 * d + 1]);
    lo[d] = cvt_pk_f16(mix_sub_f16<0>(x[2 * d], hi[d]), mix_sub_f16<1>(x[2 * d + 1], hi[d]));
  }
  if (sat) *sat = sat_fold8(x, *sat);
  *hi_out = hi;
  *lo_out = lo;
}
// relu(v) and the clamp in one v_med3_f32: med3(v, 0, 65504) == min(max(max(v, 0), -65504),
// 65504) for every finite input (-0 -> +0 like v_max_f32; NaN -> 0, see above)
template <typename V4>
__device__ __forceinline__ void split8_relu_rne(const float* v, V4* hi_out, V4* lo_out, float* sat = nullptr) {
  V4 hi, lo;
  float x[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    asm("v_med3_f32 %0, %1, 0, %2" : "=v"(x[2 * d]) : "v"(v[2 * d]), "v"(65504.f));
    asm("v_med3_f32 %0, %1, 0, %2" : "=v"(x[2 * d + 1]) : "v"(v[2 * d + 1]), "v"(65504.f));
    hi[d] = cvt_pk_f16(x[2 * d], x[2 * d + 1]);
    lo[d] = cvt_pk_f16(mix_sub_f16<0>(x[2 * d], hi[d]), mix_sub_f16<1>(x[2 * d + 1], hi[d]));
  }
  if (sat) *sat = sat_fold8(x, *sat);
  *hi_out = hi;
  *lo_out = lo;
}
template <typename V4>   // (hi, lo) -> 8 fp32, v[e] = float(hi[e]) + float(lo[e])
__device__ __forceinline__ void join8_exact(V4 hi, V4 lo, float* v) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    v[2 * d] = mix_add_f16<0>(hi[d], lo[d]);
    v[2 * d + 1] = mix_add_f16<1>(hi[d], lo[d]);
  }
}

}  // namespace milan

struct milan_ctx {
  int device = 0;
  milan_dims d{};
  bool finalized = false;
  int precision = 0;  // MILAN_PRECISION_F32 / MILAN_PRECISION_SPLIT_F16 (also in fast mode:
                      // decoder, LM and the front of the trunk stay split)
  int trunk_f16 = 0;  // MILAN_PRECISION_F16: layer3 / layer4 of a bottleneck trunk on plain f16
  int fusion = MILAN_FUSE_CHAIN | MILAN_FUSE_CHAIN_WIDE | MILAN_FUSE_STEM | MILAN_FUSE_CONV3 |
               MILAN_FUSE_SKIP_EMPTY | MILAN_FUSE_BNECK | MILAN_FUSE_SPARSE_TAIL |
               MILAN_FUSE_TAIL_LISTS;  // milan_set_fusion
  // hipGraph cache of whole decode passes (milan_set_graph_capture)
  int graph_capture = 0;
  struct GraphEntry { std::vector<char> key; hipGraphExec_t exec = nullptr; int seen = 0; };
  std::vector<GraphEntry> graphs;
  long graph_replays = 0, graph_captures = 0;
  float* scratch = nullptr;   // per-call split-conversion scratch (workspace)
  size_t scratch_floats = 0;
  std::map<std::string, milan::Tensor> raw;  // named reference tensors
  // weight arena (library-owned, freed in milan_destroy)
  std::vector<void*> owned;
  float* zero = nullptr;
  // encoder
  milan::ConvW stem;
  milan::ConvW stem_pair;  // split-f16 stem over pixel-pair groups (encoder.hip)
  milan::ConvW alex[5];    // 'alexnet' config: features.0/3/6/8/10
  float *bn1_scale = nullptr, *bn1_shift = nullptr;
  // Split-f16 trunk: every activation tensor in split format is stored as x * act_scale
  // (an exact power of two; MILAN_ACT_SCALE_LOG2, default 5).  `lo = f16(x - f16(x))`
  // leaves the f16 normal range for |x| < 0.125, and its absolute floor (2^-24) then
  // costs accuracy relative to x; stored 32 x larger, the same happens only below 0.004,
  // while `hi` saturates at 2047 instead of 65504.  Scaling by a power of two commutes
  // with every fp32 operation of the epilogues, so the only places that know about it
  // are: the stem's folded bn1 (scale, shift) and every conv's folded bias (pre-multiplied
  // copies below / ConvW::bias_s), and the consumers that leave the split domain (the
  // mask-weighted pooling and the spatial read-out divide by it).
  float act_scale = 32.f;
  int act_scale_log2 = 5;
  float *bn1_scale_s = nullptr, *bn1_shift_s = nullptr;
  // Split-f16 decoder: the feature-carrying A operands (pooled features of init_h / init_c,
  // features of key_to_hidden, the gated context in [emb | ctx * gate | h]) are converted as
  // x * feat_scale, an exact power of two (milan_set_feature_scale_log2, default 2^0), for the
  // same reason as act_scale above: features far below 1 lose `lo` to the f16 subnormals.
  // Undone exactly: acc_scale / feat_scale for the three single-source products, and the
  // feature columns of lstm_cat's split copy hold W / feat_scale.  A property of the context,
  // never of a call's data.  Neither the exact-fp32 mode nor a layer without a split copy
  // knows about it.
  // emb_scale (milan_set_embedding_scale_log2): the same for the embedding columns of the two
  // LSTM inputs (decoder: [emb | ...] of lstm_cat, LM: layer 0 of lm_cat); the tables are
  // gathered as e * emb_scale and those weight columns hold W / emb_scale.
  float feat_scale = 1.f;
  int feat_scale_log2 = 0;
  float emb_scale = 1.f;
  int emb_scale_log2 = 0;
  float emb_absmax = 0.f;    // largest |entry| of the embedding tables (milan_get_embedding_absmax)
  float feat_absmax = 0.f;   // largest |feature| of the last milan_encoder_absmax sample
  unsigned* stem_lut = nullptr;  // byte -> split value table of the uint8 stem (StemArgs::lut), lazily
  // device status word (MILAN_STATUS_* bits, milan_status): ORed by the split epilogues when
  // a value hit the +-65504 clamp and by the input conversion when a pixel was not finite
  unsigned* status = nullptr;
  unsigned* calib = nullptr;   // != nullptr only inside milan_encoder_absmax
  // beam-search path (milan_set_beam_path): 0 = by beam width, 1 = the wide kernels wherever
  // they apply (an A/B and test knob; the two paths select the same beams, bit for bit)
  int beam_path = 0;
  // image sharing (milan_set_image_sharing; share.hip): off by default
  int share_images = 0;
  int share_hash_bits = 64;            // MILAN_SHARE_HASH_BITS at milan_create (a test knob)
  long long* share_stats = nullptr;    // device: exemplar slots seen, images through the trunk
  std::vector<milan::Bottleneck> blocks[4];
  float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  // decoder
  milan::LinearW init_h, init_c, q2h, k2h, gate, lstm_ih, lstm_hh, out;
  milan::LinearW lstm_cat;                   // [W_ih | W_hh] along K (split mode)
  float *att_w = nullptr, *att_b = nullptr;  // attend.output.0: [A], [1]
  float* embedding = nullptr;                // [V][E]
  // language model
  std::vector<milan::LinearW> lm_ih, lm_hh;  // per layer
  std::vector<milan::LinearW> lm_cat;        // [W_ih | W_hh] per layer
  milan::LinearW lm_out;
  float* lm_embedding = nullptr;
  // classifier head (<prefix>fc.weight / fc.bias, fp32 as uploaded) and the ablation set of
  // milan_set_ablation: 0/1 channel masks of the five levels (conv1, layer1..4) back to back in
  // one device array, ones until a set is installed; abl_count = distinct units per level
  float *fc_w = nullptr, *fc_b = nullptr;
  int fc_classes = 0, fc_in = 0;
  float* abl_mask = nullptr;
  int abl_off[5] = {0, 0, 0, 0, 0}, abl_ch[5] = {0, 0, 0, 0, 0}, abl_count[5] = {0, 0, 0, 0, 0};
  // AlexNet head (milan_set_alexnet_head; `installed` switches the classify family on for an
  // AlexNet context): fc6 / fc7 / linear8 in linear_mfma_kernel's packed order, biases as given
  struct AlexHead {
    bool installed = false;
    float* w[3] = {nullptr, nullptr, nullptr};
    float* b[3] = {nullptr, nullptr, nullptr};
    int out[3] = {0, 0, 0}, in[3] = {0, 0, 0};
  } ahead;
  // the Places365 AlexNet's optional LRN after pool1 and pool2 (milan_set_alexnet_lrn; 0: off)
  struct AlexLrn { int size = 0; float alpha = 1e-4f, beta = 0.75f; } lrn;
  // VGG (MILAN_TRUNK_VGG): block b's convs vgg[b][0 .. vgg_n[b] - 1], as the
  // uploaded keys `vgg.B.J` gave them; conv1_1 once more as vgg_w27, (27 taps in (kh, kw, c)
  // order) x cout fp32, for vgg_first_kernel.  Its head lives in `ahead` (milan_set_vgg_head).
  milan::ConvW vgg[5][4];
  int vgg_n[5] = {0, 0, 0, 0, 0};
  float* vgg_w27 = nullptr;
  // what the walks of the last classify-family call launched (milan_vgg_trace): slot 4 b + j
  mutable int vgg_launches[20] = {};
  mutable int vgg_split[20] = {};
};

namespace milan {
// ---- the two AlexNets ------------------------------------------
// What torchvision's AlexNet (MILAN_TRUNK_ALEXNET) and the Places365 one
// (MILAN_TRUNK_ALEXNET_PLACES) differ in when encoder_finalize packs conv1..conv5 into
// milan_ctx::alex; whatever runs them afterwards (alexnet_plan, SeqTrunk) reads alex[l].
struct AlexSpec {
  const char* key[5];  // conv l in the state dict, under the trunk's prefix
  int stride[5], pad[5];
  int mult[5];         // channels of conv l per unit of dims.trunk_width
  bool weight_groups;  // conv l's groups = its input's channels / its weight's second extent
  bool width8;         // dims.trunk_width has to be a multiple of 8
};
inline const AlexSpec& alex_spec(int trunk_kind) {
  static const AlexSpec spec[2] = {
      {{"features.0", "features.3", "features.6", "features.8", "features.10"},
       {4, 1, 1, 1, 1}, {2, 2, 1, 1, 1}, {1, 3, 6, 4, 4}, false, false},
      {{"conv1", "conv2", "conv3", "conv4", "conv5"},
       {4, 1, 1, 1, 1}, {0, 2, 1, 1, 1}, {3, 8, 12, 12, 8}, true, true}};
  return spec[trunk_kind == MILAN_TRUNK_ALEXNET_PLACES];
}

// ---- the sequential classifier trunks ---------------------------
// What the nets that classify.hip's SeqTrunk walks differ in outside their step plans: one row
// per trunk kind.  The message texts are the ones each family had when it was added.
//   vgg         the convs are milan_ctx::vgg (alex otherwise)
//   bins        the tail's bins each way: fc reads bins x bins features per channel
//   tail_lo/hi  pixels each way that pool5 has to leave for the head
//   levels      the five levels, for messages
//   setter, trunk, fc   the entry point that installs the head, what it calls the trunk it asks
//               for, and the three Linear layers
//   no_head     classify on a context without a head (nullptr: such a context is no classifier)
//   head_image  (H, W, fc in): an image that the head cannot take (nullptr: the pass refuses it,
//               SeqTrunk::check_geometry)
//   taps_call   what milan_activations' workspace and sub-batch messages call it
struct SeqFamily {
  bool vgg;
  int bins, tail_lo, tail_hi;
  const char *levels, *setter, *trunk, *fc[3], *no_head, *head_image, *taps_call;
};
inline const SeqFamily* seq_family(int trunk_kind) {
  static const SeqFamily alexnet = {
      false, 6, 1, 1 << 30, "conv1..conv5", "milan_set_alexnet_head", "AlexNet",
      {"fc6", "fc7", "linear8"}, nullptr, nullptr, "classify"};
  static const SeqFamily places = {
      false, 6, 6, 6, "conv1..conv5", "milan_set_alexnet_head", "AlexNet",
      {"fc6", "fc7", "linear8"},
      "this Places365 AlexNet context has no head: milan_set_alexnet_head installs fc6 / fc7 / "
      "fc8",
      "classify: image %dx%d does not leave 6x6 after pool5 of the Places365 AlexNet (227x227 "
      "does; fc6 reads %d features)",
      "classify"};
  static const SeqFamily vgg = {
      true, 7, 1, 1 << 30, "the last conv of blocks 1..5", "milan_set_vgg_head", "a VGG",
      {"classifier.0", ".3", ".6"},
      "this VGG context has no head: milan_set_vgg_head installs classifier.0 / .3 / .6",
      "classify: image %dx%d is too small for VGG (32x32 at least: five 2x2 pools)",
      "activations"};
  return trunk_kind == MILAN_TRUNK_ALEXNET          ? &alexnet
         : trunk_kind == MILAN_TRUNK_ALEXNET_PLACES ? &places
         : trunk_kind == MILAN_TRUNK_VGG            ? &vgg
                                                    : nullptr;
}

// Extents of conv1..conv5 (h, w) and of pool1, pool2, pool5 (hq, wq: 3 x 3 / 2 without padding,
// after conv1, conv2 and conv5) of an H x W image, from the packed convs.  C's division
// truncates: an image too small for a level leaves an extent below the 3 (1) pixels the next
// pool (conv) needs, which the callers refuse.
inline void alex_geometry(const milan_ctx* c, int H, int W, int* h, int* w, int* hq, int* wq) {
  for (int l = 0, q = 0; l < 5; ++l) {
    const ConvW& cw = c->alex[l];
    H = h[l] = conv_out(H, cw.kh, cw.stride, cw.pad);
    W = w[l] = conv_out(W, cw.kw, cw.stride, cw.pad);
    if (l == 2 || l == 3) continue;
    H = hq[q] = conv_out(H, 3, 2, 0);
    W = wq[q++] = conv_out(W, 3, 2, 0);
  }
}

int dev_alloc(milan_ctx* c, void** p, size_t bytes);
// api.hip: split-f16 copy of a packed [n][kp] fp32 weight; picks a power-of-two
// scale from max|w| (host sync) and returns its inverse.
int make_split_weight(milan_ctx* c, const float* w, int n, int kp, float** ws,
                      float* ws_inv, hipStream_t s);
// encoder.hip
int pack_conv_plain(const float* w_oihw, int cout, int cin, int kh, int kw,
                    float* wp, hipStream_t s);
int encoder_finalize(milan_ctx* c, hipStream_t s);
int encoder_rescale(milan_ctx* c, hipStream_t s);
// split 3x3 weights [n][tap][Cin] -> chunk-major [n][Cin/16][tap][16]
// packed conv rows [cout][taps][cin] -> [cout][cin / (8 gps)][taps][8 gps] in 8-channel groups of
// `gb` 16-byte pieces (2: split format, 1: plain f16) -- GemmArgs::Wt (gps 4 / 8)
int make_slice_major(const float* ws, int cout, int taps, int cin, int gps, int gb, float* dst,
                     hipStream_t s);
int make_chunk_major(const float* ws, int cout, int cin, float* dst,
                     hipStream_t s);
size_t encoder_workspace(const milan_ctx* c, int n_images, int H, int W);
int encoder_run_spatial(milan_ctx* c, const void* images, int image_dtype,
                        const void* masks, int mask_dtype, int n, int H, int W,
                        float* out, milan::Arena& ws, hipStream_t s);
int encoder_run(milan_ctx* c, const void* images, int image_dtype,
                const void* masks, int mask_dtype, int n_images, int H, int W,
                float* features, Arena& ws, hipStream_t s);
// ... the plain schedule's pieces, for classify.hip (the encode paths do not use them)
int encoder_sub_batch_size();
GemmArgs encoder_conv_args(const ConvW& cw, const float* in, int n, int H, int W, float* out,
                           int epi, const float* aux, const float* zero, int* Ho, int* Wo,
                           bool split, bool scaled_bias = true);
// 3x3 / stride 2 max-pool without padding over NHWC (the AlexNet trunk): fp32 -> fp32, or with
// `split` fp32 / split (`in_split`) -> split at scale 1
int launch_maxpool3s2(const float* x, int n, int H, int W, int C, int Ho, int Wo, bool split,
                      bool in_split, float* y, unsigned* status, hipStream_t s);
int launch_raw_input(const float* images, int n, int H, int W, bool pairs, float* out,
                     unsigned* status, hipStream_t s);
GemmArgs encoder_stem_args(const milan_ctx* c, const float* in4, int n, int H, int W, float* raw,
                           bool pair_stem);
int launch_stem_tail(const milan_ctx* c, const float* raw, int n, int h1, int w1, int hp, int wp,
                     bool split, float* y, hipStream_t s);
// classify.hip: classifier head and unit ablation on the ResNet trunks (milan_classify*)
int classify_finalize(milan_ctx* c, hipStream_t s);
int classify_set_ablation(milan_ctx* c, const int32_t* levels, const int32_t* units, int count,
                          hipStream_t s);
size_t classify_workspace(const milan_ctx* c, int n, int H, int W, int sweep_units);
int classify_run(milan_ctx* c, const float* images, int n, int H, int W, float* logits,
                 int64_t* predictions, Arena& ws, hipStream_t s);
int classify_sweep(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                   const int32_t* units, int count, const int64_t* targets, int32_t* correct,
                   int64_t* predictions, Arena& ws, hipStream_t s);
// milan_set_alexnet_head / milan_set_vgg_head: `asked` is a row of the family the entry point
// serves (fc6 / fc7 / linear8, or classifier.0 / 3 / 6, into the same storage)
int classify_set_head(milan_ctx* c, const SeqFamily& asked, const float* const* w,
                      const float* const* b, const int* out, const int* in, hipStream_t s);
int classify_set_alexnet_lrn(milan_ctx* c, int local_size, float alpha, float beta);
// conv1_1's OIHW weight (cout, 3, 3, 3) -> (27, cout), k = (kh * 3 + kw) * 3 + c (classify.hip)
int vgg_pack_first(const float* w_oihw, int cout, float* w27, hipStream_t s);
// across-channel LRN over (pixels, C) with a pixel's channels contiguous, fp32 or split at
// scale 1 in and out (classify.hip, lrn_kernel); x and y must not overlap
int launch_lrn(const float* x, long long pixels, int C, bool split, int local_size, float alpha,
               float beta, float* y, unsigned* status, hipStream_t s);
// y (M, N) = act(x (M, K) W^T + bias) on the fp32 MFMA; `packed` from linear_pack
size_t linear_packed_floats(int N, int K);
int linear_pack(const float* W, int N, int K, float* packed, hipStream_t s);
int linear_run(const float* x, const float* packed, const float* bias, int M, int K, int N,
               bool relu, float* y, hipStream_t s);
// the ResNet head's fc_kernel on caller-supplied operands (a measurement baseline)
int linear_rowwise_run(const float* x, const float* W, const float* bias, int M, int K, int N,
                       float* y, hipStream_t s);
// (milan_activations' scratch is classify_workspace(c, n, H, W, 0))
int activations_run(milan_ctx* c, const float* images, int n, int H, int W, const int32_t* levels,
                    int count, float* const* outputs, Arena& ws, hipStream_t s);
// decoder.hip
int decoder_finalize(milan_ctx* c, hipStream_t s);
size_t decoder_workspace(const milan_ctx* c, int n, int k, int beam, int length);
int decoder_init_state(milan_ctx* c, const float* features, int n, int k,
                       float* h, float* cc, Arena& ws, hipStream_t s);
int decoder_step(milan_ctx* c, const float* features, int rows, int k,
                 const int64_t* tokens, const float* h, const float* cc,
                 float* h_lm, float* c_lm, float temperature,
                 float* predictions, float* attentions, float* h_out,
                 float* c_out, Arena& ws, hipStream_t s);
int decoder_decode(milan_ctx* c, const float* features, int n, int k,
                   int strategy, int length, int beam, int mi,
                   float temperature, int group_size, int64_t* tokens,
                   float* scores, float* predictions, float* attentions,
                   int64_t* beam_tokens, float* beam_scores, int32_t* out_len,
                   Arena& ws, hipStream_t s);
int decoder_lm_logprobs(milan_ctx* c, const int64_t* seqs, int rows, int L,
                        float* out, milan::Arena& ws, hipStream_t s);
int decoder_lm_score(milan_ctx* c, const int64_t* seqs, int rows, int L,
                     const int32_t* seq_len, float* out, Arena& ws,
                     hipStream_t s);
// one merge step of the beam search on caller-supplied arrays (milan_beam_merge);
// wide = 0 picks the kernel by `beam` as decoder_decode does in auto mode
int decoder_beam_merge(const float* cand_v, const int* cand_i, const float* last_lp,
                       int n, int beam_prev, int beam, int wide, float* new_lp,
                       int* new_tok, int* new_bp, hipStream_t s);
// one per-row top-k on caller-supplied arrays (milan_row_select); path 0 picks the
// kernel as decoder_decode does in auto mode, 1 = wide, 2 = threshold, 3 = legacy rank
int decoder_row_select(const float* logits, const float* lm_logits, float lambda,
                       int rows, int V, int k, const int64_t* last_tok, int stop,
                       float* cand_v, int* cand_i, int path, hipStream_t s);
// beam_wide.hip: selection kernels for beams whose candidates do not fit LDS
int launch_beam_merge_wide(const float* cand_v, const int* cand_i,
                           const float* last_lp, int n, int beam_prev, int beam,
                           float* new_lp, int* new_tok, int* new_bp, hipStream_t s);
bool row_select_wide_ok(int V, int k);
int launch_row_select_wide(const float* logits, const float* lm_logits,
                           float lambda, int rows, int V, int k,
                           const int64_t* last_tok, int stop, float* cand_v,
                           int* cand_i, hipStream_t s);
}  // namespace milan
