// What one ResNet encoder pass launches, decided once.
//
// plan_encoder() is the only place that chooses: the pass-wide forms (stem, compaction, tail
// sets, pooling kernels) and the form of every block, with the arguments of every GEMM and
// chain launch filled in on the buffers the launch really uses.  encoder_run_batch()
// (encoder.hip) walks the schedule; it decides nothing.  Plain host C++ like gemm_plan.h: no
// HIP call, no getenv, no state -- tools/enc_plan_dump.cpp includes this file alone and prints
// the schedule on a machine without a GPU.
//
// A new block form is an EncForm value, a row of plan_block() and a case of the walker.
#pragma once
#include <math.h>

#include "gemm_plan.h"

namespace milan {

// ---- packed weights ----------------------------------------------------------
struct ConvW {
  float* w = nullptr;     // [Cout][Kp]
  float* ws = nullptr;    // same, split-f16 format, scaled by 1/ws_inv
  float* ws3 = nullptr;   // 3x3 only, experiments build: ws re-ordered chunk-major (gemm.hip)
  float ws_inv = 1.f;     // exact power of two
  float* bias = nullptr;  // folded BN shift, [Cout] (nullptr for raw stem)
  float* bias_s = nullptr;  // bias x activation scale (split-f16 trunk, see milan_ctx::act_scale)
  float* wf = nullptr;      // fast mode: the hi halves of `ws` as plain f16 rows [Cout][Kp] (2 B each)
  float* wst = nullptr;     // k x k convs: `ws` with k in (32-channel slice, tap, channel) order (GemmArgs::Wt)
  float* wft = nullptr;     // ... `wf` in (64-channel slice, tap, channel) order
  int cout = 0, cin = 0, kh = 0, kw = 0, stride = 1, pad = 0, K = 0, Kp = 0;
  int cin_real = 0;  // channels before padding to a multiple of 4
  // grouped conv: cout is the full width; cin, cin_real, K and Kp are those of ONE group (cin =
  // the weight's second extent, K = kh * kw * cin; an input pixel has cin * groups channels);
  // w, ws, wst hold the groups' rows back to back ([cout][Kp])
  int groups = 1;
};
struct Bottleneck {
  ConvW c1, c2, c3, down;
  ConvW c3d;  // [c3 | downsample] concatenated along K (split mode fusion)
  bool has_down = false;
  bool basic = false;  // torchvision BasicBlock: c1 3x3 (stride), c2 3x3, no c3
};

// bump allocator over a caller-provided workspace
struct Arena {
  char* base = nullptr;
  size_t size = 0, off = 0;
  bool dry = false;  // dry run: only count
  template <typename T>
  T* get(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
    size_t o = off;
    off += bytes;
    if (dry) return nullptr;
    if (off > size) return nullptr;
    return reinterpret_cast<T*>(base + o);
  }
};

inline int conv_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

// ---- fused expand -> reduce chain (chain.hip) --------------------------------
// One launch = a bottleneck's 1x1 expand conv c3 (+ residual + ReLU) AND the next
// bottleneck's 1x1 reduce conv c1 (+ ReLU): X = relu(T2 W3^T + b3 + R),
// T1 = relu(X W1^T + b1); all tensors split-format, dense rows.  P = planes.
// Optional second expand source (a bottleneck with a stride-1 downsample branch,
// layer1.0): X = relu([T2 | A2] W3^T + b3) with W3 = [c3 | downsample] along K, no
// residual (R == nullptr).
struct ChainArgs {
  const float* T2;     // [M][P]
  const float* W3;     // [4P][P] split weights (scaled), K contiguous
  const float* bias3;  // [4P]
  const float* R;      // [M][4P] residual
  float* X;            // [M][4P]
  const float* W1;     // [NR][4P] split weights (scaled)
  const float* bias1;  // [NR]
  float* T1;           // [M][NR]
  int M, P;
  const float* A2;     // [M][KD] or nullptr
  int KD;              // channels of A2 (0 without)
  float scale3, scale1;  // 1 / weight scale of W3, W1
  long long* prof;       // timing experiments: per-workgroup phase cycles (8 per WG)
  int NR;                // output channels of the reduce conv (0 = P; 2 P at a stage boundary)
  unsigned* status;      // filled by the launcher (status_word())
  const int* m_live;     // device-side row count, see GemmArgs::m_live (nullptr: M rows)
  int m_live_mul;
  // Round 6, the bottleneck's 3x3 conv c2 IN FRONT of the chain (chain_kernel<.., CONV>; planes
  // 64, stride 1, pad 1): when C2in != nullptr the t2 operand is not read from T2 but computed
  // in the kernel from c2's input C2in [M][64] (pixels (img, y, x) of ch x cw images, split
  // format) -- t2 = relu(conv3x3(C2in; W2) * scale2 + bias2) never exists in memory.
  const float* C2in;
  const float* W2;       // [64][576] split weights (scaled), k = tap * 64 + channel
  const float* bias2;    // [64]
  float scale2;          // 1 / weight scale of W2
  int ch, cw;            // image height / width of C2in (cw <= 56)
  // ... and the block's OWN 1x1 reduce conv c1 in front of that (chain_kernel<.., CONV, C1>;
  // layer1.0, whose input has 64 channels): when W0 != nullptr, C2in is the BLOCK INPUT x
  // [M][64] and t1 = relu(x W0^T * scale0 + bias0) is computed in place in the LDS copy of
  // the input region -- neither t1 nor t2 exists in memory (the whole bottleneck in one launch).
  const float* W0;       // [64][64] split weights (scaled)
  const float* bias0;    // [64]
  float scale0;
};

// ---- what the fused kernels cover: pure arithmetic, one definition each -------------------
// chain_kernel<.., CONV>: pixels of the 3x3 conv's input region in LDS -- 256 output pixels
// + (w + 1) before and after, w <= 56, rounded up to whole 4-pixel DMA pieces (chain.hip)
constexpr int kConvMaxW = 56;
constexpr int kTailMaxP = 1024;   // pixels of the last stage per image (7 x 7 = 49 at 224 x 224)
constexpr int kTailMaxP3 = 4096;  // pixels of the stage before per image (14 x 14 = 196 at 224 x 224)

inline bool chain_supported(int P, int KD, int NR = 0) {
  if (NR == 2 * P) return KD == 0 && P == 64;  // stage boundary layer1 -> layer2
  if (NR != P) return false;
  if (KD == 0) return P == 64 || P == 128 || P == 256;
  return P == 64 && KD == 64;
}
inline bool chain_conv_supported(int P, int KD, int NR, int h, int w) {
  return P == 64 && chain_supported(P, KD, NR) && h >= 1 && w >= 1 && w <= kConvMaxW;
}
inline bool chain_conv_c1_supported(int P, int KD, int NR, int h, int w) {
  return chain_conv_supported(P, KD, NR, h, w) && KD == 64 && NR == 64;   // layer1.0
}
inline bool conv3_p64_supported(int cin, int cout, int kh, int kw, int stride, int pad) {
  return cin == 64 && cout == 64 && kh == 3 && kw == 3 && stride == 1 && pad == 1;
}
inline bool stem_fused_supported(int cout, int Kp) { return cout == 64 && Kp == 224; }

// ---- GEMM arguments of the trunk's convs (pure) ------------------------------------------
inline GemmArgs linear_args(const float* A, long lda, const float* W,
                            const float* bias, float* C, int ldc, int M, int N,
                            int K, int epi, const float* zero,
                            const float* aux = nullptr, int ldaux = 0) {
  GemmArgs g{};
  g.A = A; g.W = W; g.bias = bias; g.aux = aux; g.C = C;
  g.M = M; g.N = N; g.K = K; g.Kp = (K + 31) / 32 * 32;
  g.ldc = ldc; g.ldaux = ldaux;
  g.H = 1; g.Wd = 1; g.Cin = K; g.Ho = 1; g.Wo = 1; g.KH = 1; g.KW = 1;
  g.stride = 1; g.pad = 0;
  g.a_pix_stride = lda; g.a_img_stride = lda;
  g.epilogue = epi; g.zero = zero;
  return g;
}

inline GemmArgs conv_args(const ConvW& cw, const float* in, int n, int H, int W,
                          float* out, int epi, const float* aux,
                          const float* zero, int* Ho, int* Wo,
                          bool split = false, bool scaled_bias = true) {
  GemmArgs g{};
  *Ho = conv_out(H, cw.kh, cw.stride, cw.pad);
  *Wo = conv_out(W, cw.kw, cw.stride, cw.pad);
  g.A = in; g.W = cw.w; g.bias = cw.bias; g.aux = aux; g.C = out;
  g.M = n * (*Ho) * (*Wo); g.N = cw.cout; g.K = cw.K; g.Kp = cw.Kp;
  g.ldc = cw.cout; g.ldaux = cw.cout;
  g.H = H; g.Wd = W; g.Cin = cw.cin; g.Ho = *Ho; g.Wo = *Wo;
  g.KH = cw.kh; g.KW = cw.kw; g.stride = cw.stride; g.pad = cw.pad;
  g.a_pix_stride = cw.cin;
  g.a_img_stride = (long)H * W * cw.cin;
  g.epilogue = epi; g.zero = zero;
  g.flop_k = cw.kh * cw.kw * cw.cin_real;
  if (cw.groups > 1) {
    // one group's product, the full rows as strides (GemmArgs::groups)
    const int ng = cw.cout / cw.groups;
    g.N = ng;
    g.a_pix_stride = (long)cw.cin * cw.groups;
    g.a_img_stride = (long)H * W * cw.cin * cw.groups;
    g.groups = cw.groups;
    g.a_grp = cw.cin; g.w_grp = (long)ng * cw.Kp;
    g.bias_grp = ng; g.c_grp = ng; g.aux_grp = ng;
  }
  if (split) {
    g.W = cw.ws; g.a_split = 1; g.out_split = 1; g.aux_split = aux != nullptr;
    g.acc_scale = cw.ws_inv;
    g.W3 = cw.ws3;
    g.Wt = cw.wst;
    // the ResNet trunks keep split activations in the context's activation scale
    if (scaled_bias && cw.bias_s) g.bias = cw.bias_s;
  }
  return g;
}

// fast mode (MILAN_PRECISION_F16): the same conv on plain f16 tensors -- every K-side
// quantity in 4-byte units (GemmArgs::f16), weights = the f16 rows of ConvW::wf
inline GemmArgs conv_args_f16(const ConvW& cw, const float* in, int n, int H, int W,
                              float* out, int epi, const float* aux, const float* zero,
                              int* Ho, int* Wo) {
  GemmArgs g = conv_args(cw, in, n, H, W, out, epi, aux, zero, Ho, Wo, true);
  g.W = cw.wf; g.W3 = nullptr; g.Wt = cw.wft;
  g.f16 = 1; g.out_split = 0; g.aux_split = 0;
  g.Cin = cw.cin / 2; g.K = cw.K / 2; g.Kp = cw.Kp / 2;
  g.a_pix_stride = cw.cin / 2;
  g.a_img_stride = (long)H * W * (cw.cin / 2);
  g.ldc = cw.cout / 2; g.ldaux = cw.cout / 2;
  return g;
}

// c3 and the downsample of a stage's first block as ONE GEMM over [t2 | x(strided)]; `f16`: the
// fast mode's form, the K-side quantities of both sources in 4-byte units
inline GemmArgs two_source_args(const Bottleneck& b, const float* t2, const float* xin, float* yo,
                                int n, int hh, int ww, int h2, int w2, const float* zero,
                                int* h3, int* w3, bool f16 = false) {
  GemmArgs g3 = f16 ? conv_args_f16(b.c3d, t2, n, h2, w2, yo, EPI_BIAS_RELU, nullptr, zero, h3, w3)
                    : conv_args(b.c3d, t2, n, h2, w2, yo, EPI_BIAS_RELU, nullptr, zero, h3, w3, true);
  const int u = f16 ? 2 : 1;
  g3.Cin = b.c3.cin / u;              // geometry of source 1 (t2)
  g3.a_pix_stride = b.c3.cin / u;
  g3.a_img_stride = (long)h2 * w2 * (b.c3.cin / u);
  g3.A2 = xin; g3.K1 = b.c3.K / u; g3.H2 = hh; g3.W2d = ww;
  g3.stride2 = b.down.stride;
  g3.a2_pix_stride = b.down.cin / u;
  g3.a2_img_stride = (long)hh * ww * (b.down.cin / u);
  g3.flop_k = b.c3.K + b.down.K;
  return g3;
}

// conv1 7x7/2 as the unfused stem launches it: raw fp32 output (n, h1, w1, width); the pair
// stem is KH=7 x KW=4 over pixel-pair groups, horizontal stride 1 / pad 1
inline GemmArgs stem_args(const ConvW& stem, const ConvW& stem_pair, const float* zero,
                          const float* in4, int n, int H, int W, float* raw, bool pair_stem) {
  int ho, wo;
  GemmArgs g = conv_args(stem, in4, n, H, W, raw, EPI_BIAS, nullptr, zero, &ho, &wo);
  if (pair_stem) {
    const int G = (W + 2) / 2;
    g = conv_args(stem_pair, in4, n, H, G, raw, EPI_BIAS, nullptr, zero, &ho, &wo, true);
    g.Ho = conv_out(H, 7, 2, 3); g.Wo = conv_out(W, 7, 2, 3);
    g.M = n * g.Ho * g.Wo;
    g.aniso = 1; g.stride_w = 1; g.pad_w = 1;
    g.out_split = 0;  // the raw fp32 output is pyramid tap 0
    g.flop_k = stem.kh * stem.kw * stem.cin_real;  // 7x7x3 = 147
  }
  return g;
}

// ---- the buffers of a pass -----------------------------------------------------------------
struct Levels {
  int h[5], w[5];
  long off[5];  // offset (entries) of level l inside one image's list
  long per_image;
};

struct EncBuffers {
  Levels lv;
  int h1, w1, hp, wp;
  size_t x_sz, t1_sz, t2_sz;  // per-image extents of x0/x1/ds, t1, t2 (floats)
  float *in4, *raw, *x0, *x1, *ds, *t1, *t2;
  int *list_idx, *list_n;
  float* list_w;
  int* bbox;  // [n][4]: level-0 bounding box of the listed pixels
  int* poison;  // [n]: 1 = the image holds a non-finite pixel (float inputs only)
  int *order, *bbox_c, *count;  // images with a non-empty mask (compact_images_kernel)
  // mask-aware tail of the last stage: per-slot pixel sets [3][n][P4], their counts / offsets
  // [3][n], the global row lists [3][n * P4] and row counts [3] (device)
  int *tail_loc, *tail_cnt, *tail_off, *tail_rows, *tail_U;
  // image sharing (share.hip): per-slot hash / rep / flag / class_of, and the union of the
  // members' level-4 lists per trunk slot as a byte map [n][P4]
  void* sh_hash;
  int *sh_rep, *sh_flag, *class_of;
  unsigned char* tail_s0;
  // MILAN_FUSE_TAIL_LISTS: sets V, W of the stage before the last (tail_sets3_kernel), laid
  // out like the tail_* arrays above with 2 sets of P3 pixels; byte map of the level-3 unions
  int *tail_loc3, *tail_cnt3, *tail_off3, *tail_rows3, *tail_U3;
  unsigned char* tail_s3;
};

// Level extents and buffer sizes of an H x W pass, and -- with an arena -- the buffers of n
// images.  The only place that computes either (classify.hip's ResNetTrunk asks without an
// arena and carves its own subset).
inline void enc_carve(int trunk_kind, int wd, int n, int H, int W, Arena* a, EncBuffers* pl) {
  pl->h1 = conv_out(H, 7, 2, 3); pl->w1 = conv_out(W, 7, 2, 3);
  pl->hp = conv_out(pl->h1, 3, 2, 1); pl->wp = conv_out(pl->w1, 3, 2, 1);
  Levels& lv = pl->lv;
  lv.h[0] = pl->h1; lv.w[0] = pl->w1;
  lv.h[1] = pl->hp; lv.w[1] = pl->wp;
  for (int l = 2; l < 5; ++l) {
    lv.h[l] = conv_out(lv.h[l - 1], 3, 2, 1);
    lv.w[l] = conv_out(lv.w[l - 1], 3, 2, 1);
  }
  long off = 0;
  for (int l = 0; l < 5; ++l) { lv.off[l] = off; off += (long)lv.h[l] * lv.w[l]; }
  lv.per_image = off;
  // Per-image extents of the activation buffers: the largest tensor each one
  // ever holds.  At 224x224 that is always the layer1 tensor, but once an image
  // is so small that the spatial size bottoms out at 1x1 the channel growth of
  // the later stages wins.
  const int exp = trunk_kind == MILAN_TRUNK_BASIC ? 1 : 4;
  size_t x_sz = (size_t)pl->hp * pl->wp * wd, t1_sz = 0, t2_sz = 0;
  for (int li = 0; li < 4; ++li) {
    const size_t planes = (size_t)wd << li;
    const size_t in_px = (size_t)lv.h[li == 0 ? 1 : li] * lv.w[li == 0 ? 1 : li];
    const size_t out_px = (size_t)lv.h[li + 1] * lv.w[li + 1];
    x_sz = x_sz > out_px * planes * exp ? x_sz : out_px * planes * exp;
    t1_sz = t1_sz > in_px * planes ? t1_sz : in_px * planes;   // c1 output
    t2_sz = t2_sz > out_px * planes ? t2_sz : out_px * planes; // c2 output
  }
  pl->x_sz = x_sz; pl->t1_sz = t1_sz; pl->t2_sz = t2_sz;
  if (a == nullptr) return;
  pl->in4 = a->get<float>((size_t)n * H * (W + 2) * 4);
  pl->raw = a->get<float>((size_t)n * pl->h1 * pl->w1 * wd);
  pl->x0 = a->get<float>((size_t)n * x_sz);
  pl->x1 = a->get<float>((size_t)n * x_sz);
  pl->ds = a->get<float>((size_t)n * x_sz);
  pl->t1 = a->get<float>((size_t)n * t1_sz);
  pl->t2 = a->get<float>((size_t)n * t2_sz);
  pl->list_idx = a->get<int>((size_t)n * lv.per_image);
  pl->list_w = a->get<float>((size_t)n * lv.per_image);
  pl->list_n = a->get<int>((size_t)n * 5);
  pl->bbox = a->get<int>((size_t)n * 4);
  pl->poison = a->get<int>((size_t)n);
  pl->order = a->get<int>((size_t)n);
  pl->bbox_c = a->get<int>((size_t)n * 4);
  pl->count = a->get<int>(4);
  const size_t P4 = (size_t)lv.h[4] * lv.w[4];
  pl->tail_loc = a->get<int>(3 * (size_t)n * P4);
  pl->tail_rows = a->get<int>(3 * (size_t)n * P4);
  pl->tail_cnt = a->get<int>(3 * (size_t)n);
  pl->tail_off = a->get<int>(3 * (size_t)n);
  pl->tail_U = a->get<int>(4);
  pl->sh_hash = a->get<unsigned long long>((size_t)n);
  pl->sh_rep = a->get<int>((size_t)n);
  pl->sh_flag = a->get<int>((size_t)n);
  pl->class_of = a->get<int>((size_t)n);
  pl->tail_s0 = a->get<unsigned char>(((size_t)n * P4 + 3) & ~(size_t)3);
  const size_t P3 = (size_t)lv.h[3] * lv.w[3];
  pl->tail_loc3 = a->get<int>(2 * (size_t)n * P3);
  pl->tail_rows3 = a->get<int>(2 * (size_t)n * P3);
  pl->tail_cnt3 = a->get<int>(2 * (size_t)n);
  pl->tail_off3 = a->get<int>(2 * (size_t)n);
  pl->tail_U3 = a->get<int>(4);
  pl->tail_s3 = a->get<unsigned char>(((size_t)n * P3 + 3) & ~(size_t)3);
}

// ---- everything the decision reads ---------------------------------------------------------
// The knobs of the encoder pass, read from the environment in one place (encoder.hip,
// read_enc_env).  The defaults are the knobs' defaults.
struct EncEnv {
  int stem_u8 = 1;     // MILAN_STEM_U8: 0 uint8 images through preprocess_pairs_kernel (same bits)
  int pool_vec = 1;    // MILAN_POOL_VEC: 0 the pooling with a lane per channel (rounds 1-4)
  int enc_sub = 9600;  // MILAN_ENC_SUB: images per encoder pass
  int taps_inner = 0;  // MILAN_TAPS_INNER, experiments build only: chunk-major 3x3 launches
};

struct EncAsk {
  int trunk_kind = 0, width = 0, feature_size = 0;
  const std::vector<Bottleneck>* blocks = nullptr;  // [4]
  const ConvW *stem = nullptr, *stem_pair = nullptr;
  int precision = 0, trunk_f16 = 0, fusion = 0;
  bool calib = false, share = false;
  float mean[3] = {0.f, 0.f, 0.f}, stdv[3] = {1.f, 1.f, 1.f};  // (norm_max < 60000: the uint8 stem)
  int n = 0, H = 0, W = 0, image_dtype = 0;
  bool images_aligned4 = false, masks = false;
  int mask_dtype = 0;
  bool spatial = false;
  const float* zero = nullptr;  // the context's zero line: an operand of every GEMM, not a choice
  GemmEnv genv;
  EncEnv env;
};

// ---- the schedule ----------------------------------------------------------------------------
// The forms of a block, in the order plan_block() tries them (TAIL_LISTS / TAIL_COPY are one
// test, LIST_FIRST / LIST_LAST3 are named by resolve_lists() from TWO_SOURCE / PLAIN records).
enum EncForm : int {
  EF_F16 = 0,      // fast mode, stages 3-4: c1, c2, c3 (residual or two-source) on plain f16
  EF_TAIL_LISTS,   // one of the last two blocks of the last stage on row sets kM / kO, as row lists
  EF_TAIL_COPY,    // ... on gathered copies of the rows (the raw conv1 tensor as scratch)
  EF_BASIC,        // BasicBlock: c1, [downsample], c2 + identity
  EF_LIST_FIRST,   // l4.0: c1 on V, c2 and c3 + downsample on tail set k0
  EF_LIST_LAST3,   // last block of stage 3: c1 dense, c2 and c3 on W
  EF_CHAIN_PLAIN,  // c3 + residual and the next block's c1 in one launch
  EF_CHAIN_DS,     // ... with the stride-1 downsample as second source (layer1.0)
  EF_TWO_SOURCE,   // c3 and the downsample as one GEMM over [t2 | x]
  EF_PLAIN,        // [downsample GEMM], c3 + residual
  EF_COUNT
};
enum EncC1 : int { C1_READY = 0, C1_LAUNCH, C1_FUSED, C1_LIST };
enum EncC2 : int { C2_NONE = 0, C2_CONV3, C2_GEMM, C2_LIST };
enum EncPool : int { POOL_F32 = 0, POOL_SPLIT, POOL_SPLIT8, POOL_F16 };
enum EncCompact : int { COMPACT_NONE = 0, COMPACT_SKIP_EMPTY, COMPACT_CLASSES };

inline const char* enc_form_name(int f) {
  static const char* const names[EF_COUNT] = {
      "F16", "TAIL_LISTS", "TAIL_COPY", "BASIC", "LIST_FIRST", "LIST_LAST3", "CHAIN_PLAIN",
      "CHAIN_DS", "TWO_SOURCE", "PLAIN"};
  return f >= 0 && f < EF_COUNT ? names[f] : "?";
}

struct EncBlock {
  int stage = 0, index = 0;
  int form = -1, c1 = C1_LAUNCH, c2 = C2_GEMM;
  int kM = -1, kO = -1;            // tail sets of c1 / of c2 and c3 (TAIL_*; LIST_FIRST: kO = k0)
  bool conv_front = false, c1_front = false;  // CHAIN_*: c2 / c2 and c1 inside the chain launch
  bool has_gd = false;             // BASIC / PLAIN: a downsample GEMM of its own
  const Bottleneck* b = nullptr;
  int h = 0, w = 0;                // input extent
  // the buffers: block input, block output, this block's c1 output, and where a chain launch
  // leaves the NEXT block's c1 output (nullptr: it leaves none)
  const float* X = nullptr;
  float *Y = nullptr, *T1 = nullptr, *T1_next = nullptr;
  // BASIC: g1 = c1, gd, g2 = c2 + identity.  TAIL_COPY: the three products on the gathered rows.
  GemmArgs g1{}, g2{}, g3{}, gd{};
  ChainArgs chain{};
};

struct EncSchedule {
  bool split = false, fast = false, pair_stem = false, stem_u8 = false, fused_stem = false;
  int compact = COMPACT_NONE;
  bool tail = false, lists = false, lists_l3 = false;
  int k0 = -1;
  int pool[5] = {0, 0, 0, 0, 0}, pool_C[5] = {0, 0, 0, 0, 0}, pool_col[5] = {0, 0, 0, 0, 0};
  const int* live = nullptr;       // device-side image count of a compacted pass
  GemmArgs stem{};                 // the unfused stem's conv1
  // fast mode: the residual stream leaves the split format in front of stage 3
  const float* f16_src = nullptr;
  long f16_groups = 0;
  std::vector<EncBlock> blocks;
  int first[5] = {0, 0, 0, 0, 0};  // blocks[first[li] .. first[li + 1]) are stage li's
  const float* out[4] = {nullptr, nullptr, nullptr, nullptr};  // stage outputs, h_out x w_out pixels
  int h_out[4] = {0, 0, 0, 0}, w_out[4] = {0, 0, 0, 0};
};

inline GemmArgs on_list(GemmArgs g, const int* rows, const int* U) {
  g.row_list = rows; g.m_live = U; g.m_live_mul = 1;
  return g;
}
inline bool list_ok(const GemmArgs& g, const GemmEnv& env) {
  const GemmPlan p = plan_gemm(g, env);
  return g.row_list != nullptr && p.err == 0 && p.list;
}
// every dense trunk launch carries the device-side image count (rows per image = Ho x Wo)
inline GemmArgs on_live(GemmArgs g, const int* live) {
  g.m_live = live; g.m_live_mul = g.Ho * g.Wo;
  return g;
}

// a bottleneck the tail forms cover
inline bool tail_block_ok(const Bottleneck& b) {
  return !b.basic && !b.has_down && b.c1.ws && b.c2.ws && b.c2.wst && b.c3.ws && b.c1.bias_s &&
         b.c2.bias_s && b.c3.bias_s && b.c1.kh == 1 && b.c1.kw == 1 && b.c1.stride == 1 &&
         b.c2.kh == 3 && b.c2.kw == 3 && b.c2.stride == 1 && b.c2.pad == 1 && b.c3.kh == 1 &&
         b.c3.kw == 1 && b.c3.stride == 1 && b.c1.K == b.c1.Kp && b.c2.K == b.c2.Kp &&
         b.c3.K == b.c3.Kp && b.c1.cout % 32 == 0 && b.c2.cin == b.c1.cout &&
         b.c2.cout == b.c1.cout && b.c3.cin == b.c1.cout && b.c3.cout == b.c1.cin &&
         b.c1.cin % 4 == 0;
}

// The walk of the stages: what plan_block() reads of the blocks in front and leaves to the
// ones behind.
struct EncWalk {
  float *x, *y;     // block input / output (ping-pong)
  int h, w;
  // t1_ready: t1buf already holds this block's c1 output -- the previous block's expand conv
  // and this block's reduce conv ran as one launch (chain.hip); survives the stage boundary
  // (the last block of layer1 chains into layer2.0's conv1)
  bool t1_ready;
  // c1 output of the current block.  A chain launch with the 3x3 conv in front (MILAN_FUSE_BNECK)
  // reads it WITH its neighbours' pixels while writing the next block's, so those launches
  // alternate between two buffers; ds is free for that in split mode (every downsample conv is
  // folded into its c3, and the fast mode borrows it from layer3 on only)
  float *t1buf, *t1alt;
};

// One block: its form and its launches' arguments on the walk's buffers; advances the walk.
inline EncBlock plan_block(const EncAsk& a, const EncBuffers& pl, const EncSchedule& sc, int li,
                           size_t bi, EncWalk& wk) {
  const std::vector<Bottleneck>& blocks = a.blocks[li];
  const Bottleneck& b = blocks[bi];
  const int n = a.n, h = wk.h, w = wk.w;
  const bool split = sc.split;
  float *const x = wk.x, *const y = wk.y;
  EncBlock r;
  r.stage = li; r.index = (int)bi; r.b = &b; r.h = h; r.w = w;
  r.X = x; r.Y = y; r.T1 = wk.t1buf;
  int h1, w1, h2, w2, h3, w3;
  auto next = [&](int ho, int wo) {
    wk.x = y; wk.y = x; wk.h = ho; wk.w = wo;
    return r;
  };
  auto live = [&](const GemmArgs& g) { return on_live(g, sc.live); };

  if (sc.fast && li >= 2) {
    r.form = EF_F16; r.T1 = pl.t1;
    r.g1 = live(conv_args_f16(b.c1, x, n, h, w, pl.t1, EPI_BIAS_RELU, nullptr, a.zero, &h1, &w1));
    r.g2 = live(conv_args_f16(b.c2, pl.t1, n, h1, w1, pl.t2, EPI_BIAS_RELU, nullptr, a.zero, &h2, &w2));
    r.g3 = live(b.has_down
                    ? two_source_args(b, pl.t2, x, y, n, h, w, h2, w2, a.zero, &h3, &w3, true)
                    : conv_args_f16(b.c3, pl.t2, n, h2, w2, y, EPI_BIAS_RES_RELU, x, a.zero, &h3, &w3));
    return next(h3, w3);
  }

  const int P4 = pl.lv.h[4] * pl.lv.w[4];
  if (sc.tail && li == 3 && bi >= 1 && bi + 2 >= blocks.size() && tail_block_ok(b) &&
      (bi + 1 == blocks.size() || tail_block_ok(blocks.back())) &&
      h == pl.lv.h[4] && w == pl.lv.w[4]) {
    // the last block is needed at the listed pixels (set 0) and its c1 at set 1; the block
    // before it at set 1 and its c1 at set 2
    r.kO = bi + 1 == blocks.size() ? 0 : 1;
    r.kM = r.kO + 1;
    const int* rowsM = pl.tail_rows + (long)r.kM * n * P4;
    const int* rowsO = pl.tail_rows + (long)r.kO * n * P4;
    const int *UM = pl.tail_U + r.kM, *UO = pl.tail_U + r.kO;
    // the three convs as the dense pass launches them, each over its set's rows of the DENSE
    // tensors -- no copy, no compact scratch
    r.g1 = on_list(conv_args(b.c1, x, n, h, w, wk.t1buf, EPI_BIAS_RELU, nullptr, a.zero, &h1, &w1, true), rowsM, UM);
    r.g2 = on_list(conv_args(b.c2, wk.t1buf, n, h1, w1, pl.t2, EPI_BIAS_RELU, nullptr, a.zero, &h2, &w2, true), rowsO, UO);
    r.g3 = on_list(conv_args(b.c3, pl.t2, n, h2, w2, y, EPI_BIAS_RES_RELU, x, a.zero, &h3, &w3, true), rowsO, UO);
    if (sc.lists && list_ok(r.g1, a.genv) && list_ok(r.g2, a.genv) && list_ok(r.g3, a.genv)) {
      r.form = EF_TAIL_LISTS; r.c1 = C1_LIST; r.c2 = C2_LIST;
      return next(h, w);
    }
    // ... or on copies: c1 at set kM (the 3x3 neighbourhoods of set kO) of the gathered rows,
    // c2 over an im2col of set kO, c3 with the gathered residual; the scratch is the raw conv1
    // tensor (dead after the level-0 pooling)
    r.form = EF_TAIL_COPY;
    const long rows_all = (long)n * P4;
    const int Cin = b.c1.cin, P = b.c1.cout, Cout = b.c3.cout;
    float* xg = pl.raw;
    float* t1c = xg + rows_all * Cin;
    float* acol = t1c + rows_all * P;
    float* t2c = acol + rows_all * 9 * P;
    float* rg = t2c + rows_all * P;
    float* yc = rg + rows_all * Cin;
    auto lin = [&](const float* A, int K, const ConvW& cw, const float* W, float* C, int N, int epi,
                   const float* aux, const int* U) {
      GemmArgs g = linear_args(A, K, W, cw.bias_s, C, N, (int)rows_all, N, K, epi, a.zero, aux, N);
      g.a_split = 1; g.out_split = 1; g.aux_split = aux != nullptr;
      g.acc_scale = cw.ws_inv;
      g.flop_k = cw.kh * cw.kw * cw.cin_real;
      g.m_live = U; g.m_live_mul = 1;
      return g;
    };
    r.g1 = lin(xg, Cin, b.c1, b.c1.ws, t1c, P, EPI_BIAS_RELU, nullptr, UM);
    r.g2 = lin(acol, 9 * P, b.c2, b.c2.wst, t2c, P, EPI_BIAS_RELU, nullptr, UO);
    r.g3 = lin(t2c, P, b.c3, b.c3.ws, yc, Cout, EPI_BIAS_RES_RELU, rg, UO);
    return next(h, w);
  }

  if (b.basic) {
    // BasicBlock (resnet18/34): relu(bn2(conv2(relu(bn1(conv1(x))))) + id)
    r.form = EF_BASIC; r.T1 = pl.t1;
    r.g1 = live(conv_args(b.c1, x, n, h, w, pl.t1, EPI_BIAS_RELU, nullptr, a.zero, &h1, &w1, split));
    const float* identity = x;
    if (b.has_down) {
      int hd, wdn;
      r.has_gd = true;
      r.gd = live(conv_args(b.down, x, n, h, w, pl.ds, EPI_BIAS, nullptr, a.zero, &hd, &wdn, split));
      identity = pl.ds;
    }
    r.g2 = live(conv_args(b.c2, pl.t1, n, h1, w1, y, EPI_BIAS_RES_RELU, identity, a.zero, &h3, &w3, split));
    return next(h3, w3);
  }

  float* const t1buf = wk.t1buf;
  r.g1 = live(conv_args(b.c1, x, n, h, w, t1buf, EPI_BIAS_RELU, nullptr, a.zero, &h1, &w1, split));
  const bool c1_pending = !wk.t1_ready;
  wk.t1_ready = false;
  r.g2 = conv_args(b.c2, t1buf, n, h1, w1, pl.t2, EPI_BIAS_RELU, nullptr, a.zero, &h2, &w2, split);
  // MILAN_TAPS_INNER=1 (experiments build): 3x3 convs of layer2..4 with the nine taps of a
  // 16-channel chunk in consecutive k-tiles (each pixel crosses the fabric once, not once per
  // tap; NOT the same bits; measured: no gain, profiles/r3_experiments.txt L)
  if (a.env.taps_inner && split && b.c2.ws3 && b.c2.cin >= 128 && b.c2.cout > 64) {
    r.g2.W = b.c2.ws3;
    r.g2.chunk_major = 1;
    r.g2.W3 = nullptr;  // not the LDS-strip kernel
  }
  r.g2 = live(r.g2);
  // the next block: in this stage, or the first one of the next stage (its conv1
  // is a 1x1 / stride 1 over this stage's output; the stride sits on its conv2)
  const bool last_of_stage = bi + 1 == blocks.size();
  const Bottleneck* nbp = !last_of_stage ? &blocks[bi + 1]
                          : (li + 1 < 4 && !a.blocks[li + 1].empty()) ? &a.blocks[li + 1][0] : nullptr;
  // chain launch of this block (expand conv + the next block's reduce conv): shapes
  bool chain_plain = false, chain_ds = false;
  int chain_P = 0, chain_NR = 0;
  if (split && nbp != nullptr && !(sc.fast && last_of_stage && li + 1 >= 2) && !b.basic &&
      (a.fusion & (b.c3.cin >= 256 ? MILAN_FUSE_CHAIN_WIDE : MILAN_FUSE_CHAIN))) {
    const Bottleneck& nb = *nbp;
    chain_P = b.c3.cin;
    chain_NR = last_of_stage ? 2 * chain_P : chain_P;
    const bool shapes = !nb.basic && nb.has_down == last_of_stage && nb.c1.ws &&
                        b.c3.ws && b.c3.kh == 1 && b.c3.kw == 1 && b.c3.stride == 1 &&
                        b.c3.K == b.c3.Kp && b.c3.cout == 4 * chain_P &&
                        nb.c1.kh == 1 && nb.c1.kw == 1 && nb.c1.stride == 1 &&
                        nb.c1.cin == 4 * chain_P && nb.c1.cout == chain_NR &&
                        nb.c1.K == nb.c1.Kp && b.c3.bias && nb.c1.bias;
    chain_plain = shapes && !b.has_down && chain_supported(chain_P, 0, chain_NR);
    chain_ds = shapes && b.has_down && b.c3d.ws && b.down.kh == 1 &&
               b.down.kw == 1 && b.down.stride == 1 && h2 == h &&
               w2 == w && chain_supported(chain_P, b.down.cin, chain_NR);
  }
  // round 6 (MILAN_FUSE_BNECK): layer1's 3x3 conv runs in front of that chain launch --
  // t2 never exists in memory (chain.hip, chain_kernel<.., CONV>)
  const bool conv_front =
      (chain_plain || chain_ds) && (a.fusion & MILAN_FUSE_BNECK) && b.c2.K == b.c2.Kp &&
      b.c2.bias_s && conv3_p64_supported(b.c2.cin, b.c2.cout, b.c2.kh, b.c2.kw, b.c2.stride,
                                         b.c2.pad) &&
      chain_conv_supported(chain_P, chain_ds ? b.down.cin : 0, chain_NR, h1, w1);
  // ... and for the stage's first block (64-channel input, no t1 yet) the block's own c1
  // as well: the whole bottleneck in one launch (chain_kernel<.., CONV, C1>)
  const bool c1_front =
      conv_front && c1_pending && chain_ds && b.c1.ws && b.c1.bias_s && b.c1.kh == 1 &&
      b.c1.kw == 1 && b.c1.stride == 1 && b.c1.cin == 64 && b.c1.cout == 64 &&
      b.c1.K == b.c1.Kp && h1 == h && w1 == w &&
      chain_conv_c1_supported(chain_P, b.down.cin, chain_NR, h1, w1);
  r.c1 = !c1_pending ? C1_READY : C1_LAUNCH;
  // layer1's 3x3: weights in registers, input tile staged once (conv3.hip)
  r.c2 = split && (a.fusion & MILAN_FUSE_CONV3) && b.c2.K == b.c2.Kp &&
                 conv3_p64_supported(b.c2.cin, b.c2.cout, b.c2.kh, b.c2.kw, b.c2.stride, b.c2.pad)
             ? C2_CONV3 : C2_GEMM;

  // Expand conv of this block + reduce conv of the next one in ONE launch: the
  // 4P-channel block output is written once and not read back by the next c1.
  if (chain_plain || chain_ds) {
    r.form = chain_plain ? EF_CHAIN_PLAIN : EF_CHAIN_DS;
    r.conv_front = conv_front; r.c1_front = c1_front;
    if (c1_front) r.c1 = C1_FUSED;
    if (conv_front) r.c2 = C2_NONE;
    const Bottleneck& nb = *nbp;
    ChainArgs& ca = r.chain;
    ca.T2 = pl.t2; ca.X = y; ca.W1 = nb.c1.ws; ca.bias1 = nb.c1.bias_s;
    ca.T1 = t1buf; ca.M = n * h2 * w2; ca.P = chain_P; ca.scale1 = nb.c1.ws_inv;
    ca.NR = chain_NR;
    ca.m_live = sc.live; ca.m_live_mul = h2 * w2;
    if (conv_front) {
      // c2's input is this block's t1; the next block's t1 goes to the OTHER buffer
      // (workgroups read their neighbours' input pixels while those write their output)
      ca.C2in = t1buf; ca.W2 = b.c2.ws; ca.bias2 = b.c2.bias_s; ca.scale2 = b.c2.ws_inv;
      ca.ch = h1; ca.cw = w1;
      ca.T2 = nullptr; ca.T1 = wk.t1alt;
      if (c1_front) {   // the region is the block INPUT; t1 is made in LDS
        ca.C2in = x; ca.W0 = b.c1.ws; ca.bias0 = b.c1.bias_s; ca.scale0 = b.c1.ws_inv;
      }
      wk.t1buf = wk.t1alt; wk.t1alt = t1buf;
    }
    if (chain_plain) {
      ca.W3 = b.c3.ws; ca.bias3 = b.c3.bias_s; ca.R = x; ca.scale3 = b.c3.ws_inv;
    } else {
      ca.W3 = b.c3d.ws; ca.bias3 = b.c3d.bias_s; ca.A2 = x; ca.KD = b.down.cin;
      ca.scale3 = b.c3d.ws_inv;
    }
    r.T1_next = ca.T1;
    wk.t1_ready = true;
    return next(h2, w2);
  }
  if (b.has_down && split && b.c3d.ws && b.c3d.cout > 64) {
    r.form = EF_TWO_SOURCE;
    r.g3 = live(two_source_args(b, pl.t2, x, y, n, h, w, h2, w2, a.zero, &h3, &w3));
    return next(h3, w3);
  }
  r.form = EF_PLAIN;
  const float* identity = x;
  if (b.has_down) {
    int hd, wdn;
    r.has_gd = true;
    r.gd = live(conv_args(b.down, x, n, h, w, pl.ds, EPI_BIAS, nullptr, a.zero, &hd, &wdn, split));
    identity = pl.ds;
  }
  r.g3 = live(conv_args(b.c3, pl.t2, n, h2, w2, y, EPI_BIAS_RES_RELU, identity, a.zero, &h3, &w3, split));
  return next(h3, w3);
}

// MILAN_FUSE_TAIL_LISTS extended downwards: the first block of the last stage feeds nothing but
// the tail blocks, which read it at tail set k0 -- its c2 and c3 + downsample run over that set,
// its c1 over the pixels V its strided c2 reads there; and the last block of the stage before
// feeds nothing but that block and its own stage's pooling: its c2 / c3 run over W
// (tail_sets3_kernel).  Both are TWO_SOURCE / PLAIN records whose launches all have a list form:
// asked of the arguments the records hold, which then go on the lists.  (Neither form changes
// what the block leaves to the next one, so the records behind stay as they are.)
inline void resolve_lists(const EncAsk& a, const EncBuffers& pl, EncSchedule& sc) {
  // (experiments build: MILAN_TAPS_INNER re-orders the 3x3 launches of the stage loop, which
  // have no list form then -- those blocks keep the dense path)
  const std::vector<Bottleneck>& b4 = a.blocks[3];
  const int n = a.n, h3l = pl.lv.h[3], w3l = pl.lv.w[3], P3 = h3l * w3l;
  const long P4 = (long)pl.lv.h[4] * pl.lv.w[4];
  if (!sc.lists || a.env.taps_inner || b4.size() < 2 || b4.size() > 3 || P3 > kTailMaxP3) return;
  EncBlock& fr = sc.blocks[sc.first[3]];
  const Bottleneck& f = b4[0];
  bool ok = true;
  for (size_t bi = 1; bi < b4.size(); ++bi) ok = ok && tail_block_ok(b4[bi]);   // they run on sets
  ok = ok && !f.basic && f.has_down && f.c3d.ws && f.c3d.cout > 64 && f.c1.kh == 1 && f.c1.kw == 1 &&
       f.c1.stride == 1 && f.c1.pad == 0 && f.c3.kh == 1 && f.c3.kw == 1 && f.c3.stride == 1 &&
       f.c3.pad == 0 && f.down.kh == 1 && f.down.kw == 1 && f.down.pad == 0 && f.c2.wst &&
       f.c1.bias_s && f.c2.bias_s && f.c3d.bias_s &&
       conv_out(h3l, f.c2.kh, f.c2.stride, f.c2.pad) == pl.lv.h[4] &&
       conv_out(w3l, f.c2.kw, f.c2.stride, f.c2.pad) == pl.lv.w[4] &&
       conv_out(h3l, 1, f.down.stride, 0) == pl.lv.h[4] &&
       conv_out(w3l, 1, f.down.stride, 0) == pl.lv.w[4] &&
       !(f.down.stride == 1 && (a.fusion & (f.c3.cin >= 256 ? MILAN_FUSE_CHAIN_WIDE : MILAN_FUSE_CHAIN))) &&
       fr.form == EF_TWO_SOURCE && fr.h == h3l && fr.w == w3l;
  if (!ok) return;
  const int k0 = (int)b4.size() - 1;
  const int* rows0 = pl.tail_rows + (long)k0 * n * P4;
  const int* rowsV = pl.tail_rows3;
  const int* rowsW = pl.tail_rows3 + (long)n * P3;
  const GemmArgs g1 = on_list(fr.g1, rowsV, pl.tail_U3);
  const GemmArgs g2 = on_list(fr.g2, rows0, pl.tail_U + k0), g3 = on_list(fr.g3, rows0, pl.tail_U + k0);
  if (!list_ok(g1, a.genv) || !list_ok(g2, a.genv) || !list_ok(g3, a.genv)) return;
  sc.k0 = k0;
  fr.form = EF_LIST_FIRST; fr.kO = k0;
  if (fr.c1 == C1_LAUNCH) { fr.c1 = C1_LIST; fr.g1 = g1; }
  fr.c2 = C2_LIST; fr.g2 = g2; fr.g3 = g3;

  const std::vector<Bottleneck>& b3 = a.blocks[2];
  if (b3.size() < 2) return;
  EncBlock& lr = sc.blocks[sc.first[3] - 1];
  const Bottleneck& l = b3.back();
  const bool ok3 = !l.basic && !l.has_down && l.c2.wst && l.c2.bias_s && l.c3.bias_s && l.c2.stride == 1 &&
                   l.c3.kh == 1 && l.c3.kw == 1 && l.c3.stride == 1 && l.c3.pad == 0 &&
                   conv_out(h3l, l.c2.kh, 1, l.c2.pad) == h3l && conv_out(w3l, l.c2.kw, 1, l.c2.pad) == w3l &&
                   lr.form == EF_PLAIN && lr.h == h3l && lr.w == w3l;
  if (!ok3) return;
  const GemmArgs l2 = on_list(lr.g2, rowsW, pl.tail_U3 + 1), l3 = on_list(lr.g3, rowsW, pl.tail_U3 + 1);
  if (!list_ok(l2, a.genv) || !list_ok(l3, a.genv)) return;
  // c1 as ever (dense), c2 and c3 at W
  sc.lists_l3 = true;
  lr.form = EF_LIST_LAST3;
  lr.c2 = C2_LIST; lr.g2 = l2; lr.g3 = l3;
}

inline EncSchedule plan_encoder(const EncAsk& a, const EncBuffers& pl) {
  EncSchedule sc;
  const int wd = a.width, n = a.n;
  const bool bottleneck = a.trunk_kind == MILAN_TRUNK_BOTTLENECK;
  const bool u8 = a.image_dtype == MILAN_DTYPE_U8;

  // split-f16 mode needs every bottleneck conv to have a split weight copy
  bool split = a.precision == MILAN_PRECISION_SPLIT_F16 && wd % 8 == 0;
  for (int li = 0; li < 4 && split; ++li)
    for (const Bottleneck& b : a.blocks[li])
      split = split && b.c1.ws && b.c2.ws && (b.basic || b.c3.ws) &&
              (!b.has_down || b.down.ws);
  // fast mode: layer3 / layer4 of a bottleneck trunk on plain f16 (needs every conv's f16 rows)
  bool fast = split && a.trunk_f16 && !a.spatial && bottleneck;
  for (int li = 2; li < 4 && fast; ++li)
    for (const Bottleneck& b : a.blocks[li])
      fast = fast && !b.basic && b.c1.wf && b.c2.wf && (b.has_down ? b.c3d.wf != nullptr : b.c3.wf != nullptr);
  sc.split = split; sc.fast = fast;
  sc.pair_stem = split && a.stem_pair->ws != nullptr;

  // images with an all-zero mask stay out of the trunk pass (MILAN_FUSE_SKIP_EMPTY; uint8
  // images only -- a float image may hold a NaN pixel, whose image the reference turns into
  // NaN even under a zero mask); image sharing generalises it to classes of equal images
  if (!a.spatial && u8 && !a.calib && a.share) sc.compact = COMPACT_CLASSES;
  else if (!a.spatial && a.masks && u8 && !a.calib && (a.fusion & MILAN_FUSE_SKIP_EMPTY))
    sc.compact = COMPACT_SKIP_EMPTY;
  sc.live = sc.compact != COMPACT_NONE ? pl.count : nullptr;

  // the stem: conv1 + bn1 + ReLU + maxpool in one launch (stem.hip), which can read uint8
  // images itself (StemArgs::in_u8) when the byte -> split value table does not saturate
  sc.fused_stem = sc.pair_stem && (a.fusion & MILAN_FUSE_STEM) &&
                  stem_fused_supported(a.stem_pair->cout, a.stem_pair->Kp);
  float norm_max = 0.f;  // largest normalised pixel magnitude
  for (int ch = 0; ch < 3; ++ch) {
    const float a0 = fabsf((0.f - a.mean[ch]) / a.stdv[ch]), a1 = fabsf((1.f - a.mean[ch]) / a.stdv[ch]);
    norm_max = fmaxf(norm_max, fmaxf(a0, a1));
  }
  sc.stem_u8 = a.env.stem_u8 && sc.fused_stem && !a.spatial && u8 && norm_max < 60000.f &&
               a.W % 4 == 0 && a.images_aligned4;
  sc.stem = on_live(stem_args(*a.stem, *a.stem_pair, a.zero, pl.in4, n, a.H, a.W, pl.raw, sc.pair_stem),
                    sc.live);

  // the pooling kernel of every level: fp32 taps, split taps with a lane per channel or per
  // 8-channel group, plain f16 taps (fast mode, levels 3-4)
  for (int l = 0, col = 0; l < 5; ++l) {
    const int C = l == 0 ? wd : (bottleneck ? wd * 4 : wd) << (l - 1);
    const int G = C / 8;
    sc.pool_C[l] = C; sc.pool_col[l] = col;
    sc.pool[l] = fast && l >= 3 ? POOL_F16
                 : !(split && l > 0) ? POOL_F32
                 : a.env.pool_vec && C % 8 == 0 && (G % 64 == 0 || (G < 64 && 64 % G == 0)) && col % 4 == 0
                     ? POOL_SPLIT8 : POOL_SPLIT;
    col += C;
  }

  // mask-aware tail of the last stage (MILAN_FUSE_SPARSE_TAIL): the last two bottlenecks run on
  // the row sets the level-4 pooling needs; MILAN_FUSE_TAIL_LISTS: as row lists in the GEMM tile
  const int P4 = pl.lv.h[4] * pl.lv.w[4];
  bool tail = split && !fast && !a.spatial && a.masks && !a.calib &&
              (a.fusion & MILAN_FUSE_SPARSE_TAIL) && bottleneck &&
              a.blocks[3].size() >= 2 && P4 >= 1 && P4 <= kTailMaxP;
  if (tail) {
    const Bottleneck& lb = a.blocks[3].back();
    // scratch of a sparse block = the raw conv1 tensor (dead after the level-0 pooling)
    const size_t need = (size_t)P4 * ((size_t)2 * lb.c1.cin + lb.c3.cout + (size_t)11 * lb.c1.cout);
    tail = need <= (size_t)pl.h1 * pl.w1 * wd;
  }
  sc.tail = tail;
  sc.lists = tail && (a.fusion & MILAN_FUSE_TAIL_LISTS);

  EncWalk wk{pl.x0, pl.x1, pl.hp, pl.wp, false, pl.t1, pl.ds};
  for (int li = 0; li < 4; ++li) {
    sc.first[li] = (int)sc.blocks.size();
    if (fast && li == 2) {
      // the residual stream leaves the split format: f16(hi + lo) into the spare buffer
      sc.f16_src = wk.x;
      sc.f16_groups = (long)n * wk.h * wk.w * ((wd * 4) << 1) / 8;   // layer2's output channels
      wk.y = wk.x; wk.x = pl.ds;
    }
    for (size_t bi = 0; bi < a.blocks[li].size(); ++bi)
      sc.blocks.push_back(plan_block(a, pl, sc, li, bi, wk));
    sc.out[li] = wk.x; sc.h_out[li] = wk.h; sc.w_out[li] = wk.w;
  }
  sc.first[4] = (int)sc.blocks.size();
  resolve_lists(a, pl, sc);
  return sc;
}

// ---- what a schedule launches, by kernel family (milan_profile_read_kernels) ---------------
inline int chain_family(const ChainArgs& c) {
  return c.P == 256 ? MILAN_KERNEL_CHAIN_WIDE : c.C2in ? MILAN_KERNEL_BNECK : MILAN_KERNEL_CHAIN;
}
// the GEMM-class launches of one block, in launch order: family[i] (MILAN_KERNEL_*), and for a
// launch_gemm call gemm[i] = its arguments (nullptr: chain / conv3_p64).  Returns the count.
inline int block_launches(const EncBlock& r, const GemmEnv& env, int family[5], const GemmArgs* gemm[5]) {
  int k = 0;
  auto add = [&](const GemmArgs* g, int fam) { gemm[k] = g; family[k++] = g ? plan_gemm(*g, env).family : fam; };
  if (r.form == EF_BASIC) {
    add(&r.g1, 0);
    if (r.has_gd) add(&r.gd, 0);
    add(&r.g2, 0);
    return k;
  }
  if (r.c1 == C1_LAUNCH || r.c1 == C1_LIST) add(&r.g1, 0);
  if (r.c2 == C2_CONV3) add(nullptr, MILAN_KERNEL_CONV3);
  else if (r.c2 != C2_NONE) add(&r.g2, 0);
  if (r.form == EF_CHAIN_PLAIN || r.form == EF_CHAIN_DS) {
    add(nullptr, chain_family(r.chain));
    return k;
  }
  if (r.has_gd) add(&r.gd, 0);
  add(&r.g3, 0);
  return k;
}

}  // namespace milan
