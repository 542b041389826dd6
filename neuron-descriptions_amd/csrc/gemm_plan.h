// Which kernel a GemmArgs runs on, decided once.
//
// plan_gemm() is the only place that chooses: the kernel, its grid, its LDS, the fields the
// launcher fills into the kernel's copy of the arguments, the profiler's family, and whether a
// grouped conv is one launch or one launch per group.  launch_gemm() (gemm.hip) runs the plan;
// row_list_supported() asks it a question.  Plain host C++: no HIP call, no getenv, no state
// -- tools/gemm_plan_dump.cpp includes this file alone and runs on a machine without a GPU.
//
// A new kernel form is one line of MILAN_GEMM_KERNELS (enum entry, name and launch-table entry
// come from it) and one row of plan_launch().
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../include/milan_hip.h"

#ifndef MILAN_EXPERIMENTS
#define MILAN_EXPERIMENTS 0
#endif
#if defined(__HIPCC__)
#define MILAN_HOST_DEVICE __host__ __device__
#else
#define MILAN_HOST_DEVICE
#endif

namespace milan {

// ---- implicit-GEMM (conv / linear) -----------------------------------------
enum Epilogue : int {
  EPI_BIAS = 0,           // C = acc + bias
  EPI_BIAS_RELU = 1,      // C = relu(acc + bias)
  EPI_BIAS_RES_RELU = 2,  // C = relu(acc + bias + aux)
  EPI_BIAS_TANH = 3,      // C = tanh(acc + bias)
  EPI_BIAS_SIGMUL = 4,    // C = sigmoid(acc + bias) * aux
  EPI_BIAS_ADD = 5,       // C = acc + bias + aux
  EPI_LSTM = 6,           // acc + bias = an LSTM's gate pre-activations, columns
                          // gate-interleaved per 16 units ([i16 f16 g16 o16] per 64):
                          // C = h' (ldc), C2 = c' (ldc), aux = c (ldaux), Cs =
                          // optional split-format copy of h' (ldc); N = 4 H
  EPI_LSE = 7,            // x = acc + bias is NOT written: per row m and 64-column block cb,
                          // C[m * ldc + 2 cb] = { max x, sum exp(x - max) } (ldc = 2 ceil(N / 64)),
                          // and lse_x[m] = x[m][lse_tgt[m * lse_tgt_stride]] -- what a log-softmax
                          // read at one target column needs (the LM's rerank pass, decoder.hip)
};

// C[M][N] (row stride ldc) = epi( A (*) W^T + bias ), fp32 MFMA, exact f32.
// A is an NHWC activation tensor addressed as an implicit im2col matrix:
//   row m = (img, ho, wo), column kk = (kh, kw, cin) with cin fastest.
// A plain linear layer is the 1x1 case with H = W = 1 and `a_pix_stride`
// the row stride of the (possibly strided) input matrix.
constexpr int MILAN_TAP_CLASSES = 9;  // 3 y-ranges x 3 x-ranges (GemmArgs::tap_cls)
struct GemmArgs {
  const float* A;
  const float* W;     // packed [N][Kp], Kp = round_up(K, 32), zero padded
  const float* bias;  // [N] or nullptr
  const float* aux;   // residual / multiplicand, row stride ldaux, or nullptr
  float* C;
  int M, N, K, Kp;
  int ldc, ldaux;
  // conv geometry
  int H, Wd, Cin, Ho, Wo, KH, KW, stride, pad;
  long a_pix_stride;  // floats between consecutive input pixels (>= Cin)
  long a_img_stride;  // floats between consecutive images
  int epilogue;
  const float* zero;  // >= 64 B of zeros (device)
  int flop_k;         // algorithmic K for FLOP accounting (0 = K)
  // split-f16 mode (see gemm.hip): A and W hold (hi,lo) f16 pairs
  int a_split;        // 1: run the 3xf16 MFMA main loop
  int out_split;      // 1: write C in split format (N % 8 == 0)
  int aux_split;      // 1: aux is in split format
  float acc_scale;    // accumulators are multiplied by this (1 / weight scale)
  int out_mode;       // filled by the launcher (OUT_*)
  // optional second operand source (split16 kernels only): k >= K1 reads a
  // 1x1 / stride `stride2` convolution input A2 (H2 x W2d pixels, no padding).
  // Used to fold a bottleneck's downsample conv into its c3 (K-concatenation).
  const float* W3;    // 3x3 convs: split weights packed chunk-major
                      // [N][Cin/16][9 taps][16 slots] (conv3x3_split16_kernel)
  const float* A2;
  int K1, H2, W2d, stride2;
  long a2_pix_stride, a2_img_stride;
  // anisotropic geometry (general igemm path only): when aniso != 0 the
  // horizontal stride / padding are stride_w / pad_w instead of stride / pad.
  // Used by the pixel-pair stem (encoder.hip).
  int aniso, stride_w, pad_w;
  int debug;          // MILAN_ABLATE timing experiments (0 in production): 1 no MFMA,
                      // 2 no DMA (igemm_kernel); 4 epilogue only, 8 main loop only (split16)
  int tile_hint;      // 0 auto (the kernel follows from the layer's N, K, kernel size);
                      // experiments: 1 / 2 the round-1 256x128x3 / 128x128x2 kernels, 3 / 4 / 5
                      // split16 256x256x4 / 256x128x3 / 128x256x3, 6 / 10 N <= 64 on / off the
                      // 64x64-wave-tile split16 kernel, 8 the LDS-strip 3x3 kernel
  int stagger;        // experiments build: half of the first-round workgroups of an expand conv
                      // start this many microseconds late (MILAN_STAGGER)
  long long* prof;    // experiments build: per-phase cycle sums over all workgroups (16 counters)
  int chunk_major;    // experiments build, split16 kernels, k x k convs: k runs (16-channel chunk,
                      // tap) with the taps INNER -- the KH*KW pieces of a pixel are requested in
                      // consecutive k-tiles and hit L2 -- and W is packed to match (ConvW::ws3)
  float* C2;          // EPI_LSTM: new cell state
  float* Cs;          // EPI_LSTM: h' once more in split format, or nullptr
  unsigned* status;   // device status word (MILAN_STATUS_* bits) or nullptr; filled by the
                      // launcher from the calling context (set_status_word)
  int f16;            // fast mode (MILAN_PRECISION_F16): A, W, aux and C hold PLAIN f16 values, 2
                      // bytes per element.  Every K-side quantity above (Cin, K, Kp, K1, pixel /
                      // image strides, ldc, ldaux) is then given in 4-byte units, i.e. HALF the
                      // element count: a row of C f16 channels is addressed exactly like a
                      // split-format row of C / 2 channels, and the ping-pong kernel multiplies
                      // "hi . hi + lo . lo" of that pretended row = one f16 MFMA per 16 real k
  const float* Wt;    // k x k convs, Cin % 32 == 0: the rows of W with k running (32-channel slice, tap,
                      // channel) instead of (tap, channel) -- ConvW::wst.  The ping-pong kernel then
                      // asks for the KH * KW shifted copies of a slice in CONSECUTIVE k-tile pairs:
                      // they hit L2 instead of crossing the fabric once per tap (gemm.hip, TAPI)
  int tap_inner;      // filled by the launcher: this launch runs in that order
  const long long* lse_tgt;  // EPI_LSE: target column of row m at lse_tgt[m * lse_tgt_stride]
  long lse_tgt_stride;
  float* lse_x;              // EPI_LSE: [M] the target column's x
  // Row count known only on the DEVICE (round 6; encoder.hip, MILAN_FUSE_SKIP_EMPTY): when
  // m_live != nullptr the launch is sized for M rows but only the first min(M, *m_live *
  // m_live_mul) hold work -- the kernel reads the word with a scalar load, workgroups whose
  // tiles lie beyond it exit, the tile that straddles it masks its rows as for a ragged M.
  // No host read-back, no hipStreamSynchronize (live_rows() below).
  const int* m_live;
  // Row list (gemm.hip, split16_pp32_tile<.., LIST>; encoder.hip, MILAN_FUSE_TAIL_LISTS): when
  // row_list != nullptr the launch computes only the output rows row_list[0 .. *m_live)
  // (m_live_mul = 1) -- ascending rows (slot * Ho + ho) * Wo + wo of the DENSE tensors: tile
  // row r of tile tm is entry 256 * tm + r, its operand rows are read and its output row is
  // written in place, unlisted rows are not touched.  256 consecutive entries must span at
  // most 256 slots (the caller's guarantee; the plan's list row checks the offset range of
  // that many images).  Same products, same order, same roundings per output value as the
  // dense launch.
  const int* row_list;
  int m_live_mul;
  // Border-class tiles of a tap-inner launch (gemm_plan.h, tap_classes(); MILAN_TAP_SKIP).  The
  // output pixels of an image are grouped by WHICH taps fall inside the input: class c is the
  // rectangle y0 <= ho < y0 + ny, x0 <= wo < x0 + nx with tap mask (bit kh * KW + kw).  A tile
  // holds 256 pixels of one class (image-major) and runs only the taps of its mask.  Filled by
  // the launcher, classes by descending tap count; 0 = linear tile order (all taps).  A caller
  // sets tap_ncls = -1 to keep a launch on the linear order (test hook).
  int tap_ncls;
  int tap_cls[MILAN_TAP_CLASSES][5];  // y0, ny, x0, nx, mask
  // Grouped convolution: `groups` > 1 runs that many independent products of
  // the SAME geometry in one launch, the group a grid dimension (blockIdx.y).  Every field
  // above describes ONE group (N, Cin, K, Kp are per-group; ldc and a_pix_stride the full
  // rows); group q reads A + q * a_grp, W (Wt) + q * w_grp, bias + q * bias_grp, aux +
  // q * aux_grp and writes C + q * c_grp (floats).  A grouped kernel shifts its copy of the
  // arguments at entry (shift_group) and runs unchanged; groups <= 1 is the plain launch.
  int groups;
  long a_grp, w_grp, bias_grp, c_grp, aux_grp;
};
static_assert(sizeof(GemmArgs) % 4 == 0, "GemmArgs is reloaded word by word");

// group `q` of a grouped launch as a plain launch on offset pointers: what a grouped kernel
// does to its arguments at entry, and what the per-group baseline (MILAN_GROUP_LAUNCH=0)
// launches one by one
MILAN_HOST_DEVICE inline void shift_group(GemmArgs& g, int q) {
  g.A += (long)q * g.a_grp;
  g.W += (long)q * g.w_grp;
  if (g.Wt) g.Wt += (long)q * g.w_grp;
  if (g.bias) g.bias += (long)q * g.bias_grp;
  if (g.aux) g.aux += (long)q * g.aux_grp;
  g.C += (long)q * g.c_grp;
  g.groups = 1;
}

enum OutMode : int { OUT_SCALAR = 0, OUT_VEC4 = 1, OUT_SPLIT8 = 2, OUT_F16 = 3 };

// ---- everything the decision reads besides the arguments -------------------------------
// The knobs of the launch path (README / DESIGN 5), read from the environment in one place
// (gemm.hip, read_gemm_env), and the device.  The defaults are the knobs' defaults.
struct GemmEnv {
  int pp = 1;            // MILAN_PP: 0 the round-3 lockstep kernels, 2 the 16-slot ping-pong form
  int pp128 = 1;         // MILAN_PP128: 0 the round-3 lockstep 256 x 128 kernel
  int pp_persist = 0;    // MILAN_PP_PERSIST: 1 persistent walk, 2 only the K <= 512 launches
  int tap_inner = 1;     // MILAN_TAP_INNER: 0 tap-major k x k convs (the round-4 bits)
  int tap_skip = 1;      // MILAN_TAP_SKIP: 0 linear tile order, every tap
  int group_launch = 1;  // MILAN_GROUP_LAUNCH: 0 one plain launch per group
  int ablate = 0;        // MILAN_ABLATE -> GemmArgs::debug
  // experiments build only (left at their defaults by the product build)
  int tile_hint = 0;               // MILAN_TILE_HINT
  std::vector<int> tile_override;  // MILAN_TILE_OVERRIDE="N:K:hint,...": (N, K, hint) triples
  int sched = 0;                   // MILAN_SCHED: 1 the issue-slot shaped loop (SHAPE 1)
  int conv3x3 = 0;                 // MILAN_CONV3X3: 1 the LDS-strip 3x3 kernel
  int linear_kernel = 1;           // MILAN_LINEAR_KERNEL: 0 no loop variant for 1x1 layers
  int persist_lin = 1;             // MILAN_PERSIST_LIN: 0 no persistent linp launches
  int persist = 0;                 // MILAN_PERSIST=<workgroups>: persistent split16 grid
  int stagger = 0, stagger_all = 0;  // MILAN_STAGGER, MILAN_STAGGER_ALL
  int cus = 256;                   // CUs of the device in whole XCD octets (device_cus8)
  bool experiments = MILAN_EXPERIMENTS != 0;
};

// ---- the kernel forms --------------------------------------------------------------------
// One line per instantiation the plan can name: X = both builds, XE = the experiments build
// only (gemm.hip makes its launch table from the same list, XE behind MILAN_EXPERIMENTS).
// The four SHAPEs of an igemm_split16_kernel tile are consecutive (0: k x k, 1: issue-slot
// shaped, 2: chunk-major, 3: 1x1 / Linear without tap arithmetic).
#define MILAN_GEMM_KERNELS(X, XE)                                                  \
  X(GK_IGEMM_256x64_C4, igemm_kernel<256, 64, 2, false, false>)                    \
  X(GK_IGEMM_256x64_C32, igemm_kernel<256, 64, 2, true, false>)                    \
  X(GK_IGEMM_128x128_C4, igemm_kernel<128, 128, 2, false, false>)                  \
  X(GK_IGEMM_128x128_C32, igemm_kernel<128, 128, 2, true, false>)                  \
  X(GK_IGEMM_256x64_C4_GROUPED, igemm_kernel<256, 64, 2, false, false, true>)      \
  X(GK_IGEMM_256x64_C32_GROUPED, igemm_kernel<256, 64, 2, true, false, true>)      \
  X(GK_IGEMM_128x128_C4_GROUPED, igemm_kernel<128, 128, 2, false, false, true>)    \
  X(GK_IGEMM_128x128_C32_GROUPED, igemm_kernel<128, 128, 2, true, false, true>)    \
  X(GK_IGEMM_256x64_C8_SPLIT, igemm_kernel<256, 64, 2, false, true>)               \
  X(GK_IGEMM_256x64_C32_SPLIT, igemm_kernel<256, 64, 2, true, true>)               \
  XE(GK_IGEMM_256x128x3_C32, igemm_kernel<256, 128, 3, true, false>)               \
  XE(GK_IGEMM_256x128x3_C32_SPLIT, igemm_kernel<256, 128, 3, true, true>)          \
  XE(GK_IGEMM_128x128_C32_SPLIT, igemm_kernel<128, 128, 2, true, true>)            \
  X(GK_TM2, igemm_split16_tm2_kernel<256, 64, 3>)                                  \
  X(GK_TM2_GROUPED, igemm_split16_tm2_kernel<256, 64, 3, true>)                    \
  X(GK_S16_256x256x5, igemm_split16_kernel<256, 256, 5, 0>)                        \
  XE(GK_S16_256x256x5_S1, igemm_split16_kernel<256, 256, 5, 1>)                    \
  XE(GK_S16_256x256x5_S2, igemm_split16_kernel<256, 256, 5, 2>)                    \
  X(GK_S16_256x256x5_S3, igemm_split16_kernel<256, 256, 5, 3>)                     \
  X(GK_S16_256x128x3, igemm_split16_kernel<256, 128, 3, 0>)                        \
  XE(GK_S16_256x128x3_S1, igemm_split16_kernel<256, 128, 3, 1>)                    \
  XE(GK_S16_256x128x3_S2, igemm_split16_kernel<256, 128, 3, 2>)                    \
  X(GK_S16_256x128x3_S3, igemm_split16_kernel<256, 128, 3, 3>)                     \
  XE(GK_S16_256x256x4, igemm_split16_kernel<256, 256, 4, 0>)                       \
  XE(GK_S16_256x256x4_S1, igemm_split16_kernel<256, 256, 4, 1>)                    \
  XE(GK_S16_256x256x4_S2, igemm_split16_kernel<256, 256, 4, 2>)                    \
  XE(GK_S16_256x256x4_S3, igemm_split16_kernel<256, 256, 4, 3>)                    \
  XE(GK_S16_128x256x3, igemm_split16_kernel<128, 256, 3, 0>)                       \
  XE(GK_S16_128x256x3_S1, igemm_split16_kernel<128, 256, 3, 1>)                    \
  XE(GK_S16_128x256x3_S2, igemm_split16_kernel<128, 256, 3, 2>)                    \
  XE(GK_S16_128x256x3_S3, igemm_split16_kernel<128, 256, 3, 3>)                    \
  X(GK_LINP, igemm_split16_linp_kernel<5>)                                         \
  X(GK_PP, igemm_split16_pp_kernel)                                                \
  X(GK_PP32, igemm_split16_pp32_kernel)                                            \
  X(GK_PP32N_128, igemm_split16_pp32n_kernel<128>)                                 \
  X(GK_PP32N_256, igemm_split16_pp32n_kernel<256>)                                 \
  X(GK_PP32T_128, igemm_split16_pp32t_kernel<128>)                                 \
  X(GK_PP32T_256, igemm_split16_pp32t_kernel<256>)                                 \
  X(GK_GROUPED_PP32N, igemm_grouped_pp32n_kernel)                                  \
  X(GK_GROUPED_PP32T, igemm_grouped_pp32t_kernel)                                  \
  X(GK_PP32L, igemm_split16_pp32l_kernel<false>)                                   \
  X(GK_PP32L_TAPI, igemm_split16_pp32l_kernel<true>)                               \
  X(GK_F16_PP32_128, igemm_f16_pp32_kernel<128, false>)                            \
  X(GK_F16_PP32_128_TAPI, igemm_f16_pp32_kernel<128, true>)                        \
  X(GK_F16_PP32_256, igemm_f16_pp32_kernel<256, false>)                            \
  X(GK_F16_PP32_256_TAPI, igemm_f16_pp32_kernel<256, true>)                        \
  XE(GK_CONV3X3_128, conv3x3_split16_kernel<128>)                                  \
  XE(GK_CONV3X3_256, conv3x3_split16_kernel<256>)

enum GemmKernel : int {
  GK_NONE = 0,
#define MILAN_GK_ENUM(id, ...) id,
  MILAN_GEMM_KERNELS(MILAN_GK_ENUM, MILAN_GK_ENUM)
#undef MILAN_GK_ENUM
  GK_COUNT
};

// plan_launch() picks the grouped igemm_kernel and the SHAPE of a split16 tile by offset
static_assert(GK_IGEMM_256x64_C32_GROUPED - GK_IGEMM_256x64_C32 == GK_IGEMM_256x64_C4_GROUPED - GK_IGEMM_256x64_C4 &&
                  GK_IGEMM_128x128_C4_GROUPED - GK_IGEMM_128x128_C4 == GK_IGEMM_256x64_C4_GROUPED - GK_IGEMM_256x64_C4 &&
                  GK_IGEMM_128x128_C32_GROUPED - GK_IGEMM_128x128_C32 == GK_IGEMM_256x64_C4_GROUPED - GK_IGEMM_256x64_C4,
              "the grouped igemm_kernel ids follow the plain ones in the same order");
static_assert(GK_S16_256x256x5_S3 == GK_S16_256x256x5 + 3 && GK_S16_256x128x3_S3 == GK_S16_256x128x3 + 3 &&
                  GK_S16_256x256x4_S3 == GK_S16_256x256x4 + 3 && GK_S16_128x256x3_S3 == GK_S16_128x256x3 + 3 &&
                  GK_S16_256x256x5_S2 == GK_S16_256x256x5 + 2 && GK_S16_256x128x3_S2 == GK_S16_256x128x3 + 2 &&
                  GK_S16_256x256x4_S2 == GK_S16_256x256x4 + 2 && GK_S16_128x256x3_S2 == GK_S16_128x256x3 + 2,
              "the four SHAPEs of a split16 tile are consecutive");

inline const char* gemm_kernel_name(int id) {
  static const char* const names[] = {
      "none",
#define MILAN_GK_NAME(id, ...) #__VA_ARGS__,
      MILAN_GEMM_KERNELS(MILAN_GK_NAME, MILAN_GK_NAME)
#undef MILAN_GK_NAME
  };
  return id >= 0 && id < GK_COUNT ? names[id] : "?";
}

// ---- the plan ------------------------------------------------------------------------------
struct GemmPlan {
  int err;        // 0, or the MILAN_ERR_* code of the refusal ...
  char msg[256];  // ... and its text
  int kernel;     // GemmKernel
  int grid_x, grid_y, threads, lds;
  int tiles_m, tiles_n;  // the kernel's two scalar arguments
  int bm, bn;            // block tile
  int family;            // MILAN_KERNEL_* (milan_profile_read_kernels)
  bool list;             // a row-list form (pp32l)
  bool per_group;        // a grouped conv that runs as `groups` plain launches; the plan then
                         // describes group 0's (launch_gemm plans each group on its own pointers)
  // what the launcher fills into the kernel's copy of the arguments
  int tile_hint, debug, stagger, out_mode, tap_inner, tap_ncls;
  int tap_cls[MILAN_TAP_CLASSES][5];
  float acc_scale;
  bool w_from_wt;        // the kernel's W is the caller's Wt (tap-inner k order)
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// per-launch limits of the ping-pong kernel's 32-bit buffer offsets: a tile's rows span
// less than 2 GB of the input, the weight panel of a tile less than 2 GB
inline bool pp_eligible(const GemmArgs& g) {
  if (g.Cin % 16 != 0 || g.aniso) return false;
  if (g.A2 && (g.K1 % 16 != 0)) return false;
  const long howo = (long)g.Ho * g.Wo;
  const long imgs = 256 / (howo > 0 ? howo : 1) + 2;  // images a 256-row tile can touch
  const long a_span = imgs * g.a_img_stride * 4 + 64;
  const long a2_span = g.A2 ? imgs * g.a2_img_stride * 4 + 64 : 0;
  const long w_span = 256L * g.Kp * 4;
  return a_span < 0x7fffffffL && a2_span < 0x7fffffffL && w_span < 0x7fffffffL;
}

// ... and of the pair-staged form of that tile (pp32*): whole 32-slot k-tile pairs per source,
// image coordinates that fit the 16-bit halves of a packed row descriptor
inline bool pair_staged_ok(const GemmArgs& g) {
  return pp_eligible(g) && g.Cin % 32 == 0 && (!g.A2 || g.K1 % 32 == 0) &&
         ((long)g.H + g.pad) < 32768 && ((long)g.Wd + g.pad) < 32768;
}

// k x k convs whose weights exist in (slice, tap, channel) order run in that order
// (MILAN_TAP_INNER=0: tap-major, the round-4 bits; A/B timing and traffic)
inline bool tap_inner_wanted(const GemmArgs& g, const GemmEnv& env) {
  // (Cin in 4-byte units: whole 32-slot slices, which is what slice_major_kernel packed)
  return env.tap_inner && g.Wt && !g.A2 && g.KH * g.KW > 1 && g.KH * g.KW <= 32 && g.K == g.Kp &&
         g.Cin % 32 == 0;
}

// A launch whose group strides are set is a grouped conv or ONE group of it (shift_group
// leaves the strides in place): the plan gives both the same tile and the same k order --
// every row below that reads `groups` reads it only to pick the grouped instantiation of the
// kernel it would have named anyway (tests/test_gemm_plan_host.py).
inline bool group_part(const GemmArgs& g) { return g.groups > 1 || g.c_grp != 0; }

// The experiments build's kernel-forcing knobs.  Like a tile hint they leave a launch neither a
// list form nor, in split mode, a grouped one -- also where they would not have changed the
// kernel: that is how the two predicates this plan replaced answered.
inline bool knob_forced(const GemmEnv& env) { return env.experiments && (env.conv3x3 || env.sched); }

// Border classes of a tap-inner launch (GemmPlan::tap_cls) and its grid.  Along one axis the
// taps k with 0 <= o * stride - pad + k < size form a set per output coordinate o; runs of equal
// sets are ranges (a few leading coordinates, the middle, a few trailing ones), a class is a
// (y-range, x-range) rectangle and its tap mask the product of the two sets.  A 3 x 3 kernel
// gives at most 9.  The launch keeps the linear tile order (tap_ncls = 0, all taps, the grid
// of tiles_m x tiles_n) when MILAN_TAP_SKIP=0, when the caller asked for it, when the geometry
// has more classes than the table holds (5 x 5 / pad 2: 25), when some pixel has no tap inside
// the image at all, or when a class tile -- up to 256 images for a one-pixel class -- would
// span more input than a 32-bit buffer offset reaches.
inline int tap_classes(const GemmArgs& t, const GemmEnv& env, GemmPlan& p) {
  const int linear = p.tiles_m * p.tiles_n;
  const bool wanted = env.tap_skip && t.tap_ncls >= 0;
  p.tap_ncls = 0;
  const int howo = t.Ho * t.Wo;
  if (!wanted || howo <= 0 || t.M % howo != 0 || (t.m_live && t.m_live_mul % howo != 0))
    return linear;
  struct Run { int o0, n; unsigned set; };
  auto runs = [](int size, int out, int k, int stride, int pad, Run* r) {
    int n = 0;
    for (int o = 0; o < out; ++o) {
      unsigned set = 0;
      for (int i = 0; i < k; ++i)
        if (o * stride - pad + i >= 0 && o * stride - pad + i < size) set |= 1u << i;
      if (n > 0 && r[n - 1].set == set) { ++r[n - 1].n; continue; }
      if (n == MILAN_TAP_CLASSES) return MILAN_TAP_CLASSES + 1;
      r[n++] = Run{o, 1, set};
    }
    return n;
  };
  Run ry[MILAN_TAP_CLASSES], rx[MILAN_TAP_CLASSES];
  const int nry = runs(t.H, t.Ho, t.KH, t.stride, t.pad, ry);
  const int nrx = runs(t.Wd, t.Wo, t.KW, t.stride, t.pad, rx);
  if (nry * nrx > MILAN_TAP_CLASSES) return linear;
  int cls[MILAN_TAP_CLASSES][5], n = 0, min_pix = howo;
  for (int a = 0; a < nry; ++a)
    for (int b = 0; b < nrx; ++b, ++n) {
      unsigned mask = 0;
      for (int kh = 0; kh < t.KH; ++kh)
        for (int kw = 0; kw < t.KW; ++kw)
          if ((ry[a].set >> kh & 1u) && (rx[b].set >> kw & 1u)) mask |= 1u << (kh * t.KW + kw);
      if (mask == 0) return linear;
      const int c[5] = {ry[a].o0, ry[a].n, rx[b].o0, rx[b].n, (int)mask};
      // insertion by descending tap count (stable): the long tiles are dispatched first
      int at = n;
      while (at > 0 && __builtin_popcount((unsigned)cls[at - 1][4]) < __builtin_popcount(mask)) {
        memcpy(cls[at], cls[at - 1], sizeof(c));
        --at;
      }
      memcpy(cls[at], c, sizeof(c));
      if (ry[a].n * rx[b].n < min_pix) min_pix = ry[a].n * rx[b].n;
    }
  if ((256L / min_pix + 2) * t.a_img_stride * 4 + 64 >= 0x7fffffffL) return linear;
  const long imgs = t.M / howo;
  long grid = 0;
  for (int c = 0; c < n; ++c)
    grid += ((imgs * cls[c][1] * cls[c][3] + 255) / 256 * p.tiles_n + 7) / 8 * 8;
  if (grid >= 0x7fffffffL) return linear;
  p.tap_ncls = n;
  memcpy(p.tap_cls, cls, sizeof(int) * 5 * n);
  return (int)grid;
}

#define MILAN_PLAN_REQUIRE(cond, code, ...)            \
  do {                                                 \
    if (!(cond)) {                                     \
      p.err = (code);                                  \
      snprintf(p.msg, sizeof(p.msg), __VA_ARGS__);     \
      return p;                                        \
    }                                                  \
  } while (0)

// The decision for ONE launch of `a` as it stands (a grouped conv: as one grouped launch; a
// leaf without a grouped instantiation leaves grid_y at 1).  plan_gemm() below adds the two
// questions that span launches.
inline GemmPlan plan_launch(const GemmArgs& a, const GemmEnv& env) {
  GemmPlan p{};
  GemmArgs g = a;
  const bool cin32 = (g.Cin % 32 == 0);
  const bool one_by_one = g.KH == 1 && g.KW == 1;
  p.grid_y = 1;
  p.tap_inner = a.tap_inner;
  p.tap_ncls = a.tap_ncls;
  p.family = g.a_split ? MILAN_KERNEL_SPLIT_OTHER : MILAN_KERNEL_F32;

  // ---- what the launcher fills in ----
  if (env.experiments) {
    if (g.tile_hint == 0) g.tile_hint = env.tile_hint;
    for (size_t i = 0; i + 2 < env.tile_override.size(); i += 3)
      if (env.tile_override[i] == g.N && env.tile_override[i + 1] == g.K) {
        if (env.tile_override[i + 2]) g.tile_hint = env.tile_override[i + 2];
        break;
      }
  }
  p.tile_hint = g.tile_hint;
  p.debug = env.ablate;  // 1: skip MFMA phase, 2: skip DMA (timing experiments only)
  // MILAN_STAGGER: the expand convs (residual / two-source, epilogue-heavy launches)
  p.stagger = !env.experiments ? a.stagger
              : (env.stagger_all || (g.out_split && g.N >= 256 && g.KH == 1 && g.H > 1 &&
                                     (g.aux || g.A2))) ? env.stagger : 0;

  // ---- the epilogue form ----
  if (g.epilogue == EPI_LSE) {
    MILAN_PLAN_REQUIRE(!g.out_split && !g.aux_split && !g.f16 && g.aux == nullptr && g.N % 4 == 0 &&
                           g.ldc == 2 * ((g.N + 63) / 64) && g.C && g.lse_tgt && g.lse_x &&
                           (g.bias == nullptr || aligned16(g.bias)),
                       MILAN_ERR_SHAPE, "gemm: bad log-sum-exp epilogue geometry (N=%d ldc=%d)",
                       g.N, g.ldc);
    p.out_mode = OUT_VEC4;
  } else if (g.epilogue == EPI_LSTM) {
    MILAN_PLAN_REQUIRE(!g.out_split && !g.aux_split && g.N % 64 == 0 && g.ldc % 8 == 0 &&
                           g.ldaux % 4 == 0 && g.C && g.C2 && g.aux && aligned16(g.C) &&
                           aligned16(g.C2) && aligned16(g.aux) &&
                           (g.Cs == nullptr || aligned16(g.Cs)) &&
                           (g.bias == nullptr || aligned16(g.bias)),
                       MILAN_ERR_SHAPE, "gemm: bad LSTM epilogue geometry (N=%d ldc=%d)", g.N,
                       g.ldc);
    p.out_mode = OUT_VEC4;
  } else if (g.f16) {
    // fast mode: plain f16 operands through the ping-pong tile only (K-side quantities in
    // 4-byte units, see GemmArgs::f16)
    MILAN_PLAN_REQUIRE(g.a_split && !g.out_split && !g.aux_split && g.N % 8 == 0 &&
                           g.ldc % 4 == 0 && aligned16(g.C) &&
                           (g.bias == nullptr || aligned16(g.bias)) &&
                           (g.aux == nullptr || (g.ldaux % 4 == 0 && aligned16(g.aux))) &&
                           (g.epilogue == EPI_BIAS || g.epilogue == EPI_BIAS_RELU ||
                            g.epilogue == EPI_BIAS_RES_RELU) &&
                           g.Cin % 32 == 0 && (!g.A2 || g.K1 % 32 == 0) && g.N >= 128 &&
                           !g.chunk_major && ((long)g.H + g.pad) < 32768 &&
                           ((long)g.Wd + g.pad) < 32768,
                       MILAN_ERR_SHAPE,
                       "gemm: unsupported fast-mode (f16) layer N=%d Cin=%d epi=%d", g.N, g.Cin,
                       g.epilogue);
    p.out_mode = OUT_F16;
  } else if (g.out_split || g.aux_split) {
    MILAN_PLAN_REQUIRE(g.out_split && g.N % 8 == 0 && g.ldc % 8 == 0 && aligned16(g.C) &&
                           (g.bias == nullptr || aligned16(g.bias)) &&
                           (g.aux == nullptr ||
                            ((g.aux_split || g.epilogue == EPI_BIAS_SIGMUL) && g.ldaux % 8 == 0 &&
                             aligned16(g.aux))) &&
                           (g.epilogue == EPI_BIAS || g.epilogue == EPI_BIAS_RELU ||
                            g.epilogue == EPI_BIAS_RES_RELU || g.epilogue == EPI_BIAS_ADD ||
                            (g.epilogue == EPI_BIAS_SIGMUL && !g.aux_split)),
                       MILAN_ERR_SHAPE,
                       "gemm: unsupported split-format epilogue (N=%d ldc=%d epi=%d)", g.N, g.ldc,
                       g.epilogue);
    p.out_mode = OUT_SPLIT8;
  } else {
    const bool vec_ok = (g.N % 4 == 0) && (g.ldc % 4 == 0) && aligned16(g.C) &&
                        (g.bias == nullptr || aligned16(g.bias)) &&
                        (g.aux == nullptr || ((g.ldaux % 4 == 0) && aligned16(g.aux)));
    p.out_mode = vec_ok ? OUT_VEC4 : OUT_SCALAR;
  }
  MILAN_PLAN_REQUIRE(g.A2 == nullptr || (g.a_split && g.N > 64 && one_by_one && g.K1 % 16 == 0 &&
                                         (g.tile_hint == 0 || g.tile_hint >= 3)),
                     MILAN_ERR_SHAPE, "gemm: two-source A needs the split16 kernels");
  p.acc_scale = g.a_split && g.acc_scale == 0.f ? 1.f : g.acc_scale;

  // ---- the leaves: each names a kernel, its tile, its grid and its LDS ----
  auto tiles = [&](int bm, int bn) {
    p.bm = bm; p.bn = bn;
    p.tiles_m = (g.M + bm - 1) / bm; p.tiles_n = (g.N + bn - 1) / bn;
    p.grid_x = p.tiles_m * p.tiles_n;
  };
  // (every tile's epilogue stages through LDS: 32 x 68 floats per wave)
  auto ring_lds = [&](int stages, int slots) {
    const int ring = stages * (p.bm + p.bn) * slots * 4, stage = p.threads / 64 * 32 * 68 * 4;
    p.lds = ring < stage ? stage : ring;
  };
  // igemm_kernel: 64 x 64 per wave, 32-slot k-tiles
  auto igemm = [&](int kernel, int bm, int bn, int stages) {
    p.kernel = kernel;
    tiles(bm, bn);
    p.threads = (bm / 64) * (bn / 64) * 64;
    ring_lds(stages, 32);
    return p;
  };
  // igemm_split16_kernel<BM, BN, STAGES, shape>: 128 x 64 per wave, 16-slot k-tiles
  auto split16 = [&](int kernel_shape0, int bm, int bn, int stages, int shape) {
    p.kernel = kernel_shape0 + shape;
    tiles(bm, bn);
    p.threads = (bm / 128) * (bn / 64) * 64;
    ring_lds(stages, 16);
    // MILAN_PERSIST=<workgroups>: persistent grid (a multiple of 8; 4-wave tiles run two
    // workgroups per CU)
    const int pgrid = env.persist / 8 * 8 * (p.threads == 256 ? 2 : 1);
    if (env.experiments && env.persist >= 8 && p.grid_x > pgrid) p.grid_x = pgrid;
    return p;
  };
  // the pair-staged ping-pong tile, 256 x BNW: A ring 3 x 32 KB + W ring 2 x 32 KB
  auto pp32 = [&](int bnw, int kernel) {
    p.kernel = kernel;
    p.threads = 512;
    p.lds = 5 * 256 * 32 * 4;
    if (p.bn != bnw) tiles(256, bnw);
  };
  auto tap_inner = [&]() {
    p.w_from_wt = true;
    p.tap_inner = 1;
  };

  if (!g.a_split) {
    // fp32.  (The 8-wave 3-stage tile measured 4% slower than 128x128x2 in F32 mode, where one
    // k-tile is 4096 MFMA cycles and latency is already hidden: experiments, tile_hint 1.)
    // A grouped conv: the same tiles, the group as grid.y.
    if (g.groups > 1) p.grid_y = g.groups;
    const int grp = g.groups > 1 ? GK_IGEMM_256x64_C4_GROUPED - GK_IGEMM_256x64_C4 : 0;
    if (g.N <= 64) return igemm((cin32 ? GK_IGEMM_256x64_C32 : GK_IGEMM_256x64_C4) + grp, 256, 64, 2);
    if (env.experiments && cin32 && g.tile_hint == 1 && g.groups <= 1)
      return igemm(GK_IGEMM_256x128x3_C32, 256, 128, 3);
    return igemm((cin32 ? GK_IGEMM_128x128_C32 : GK_IGEMM_128x128_C4) + grp, 128, 128, 2);
  }

  if (g.f16) {
    MILAN_PLAN_REQUIRE(pp_eligible(g), MILAN_ERR_SHAPE,
                       "gemm: fast-mode layer exceeds the 32-bit buffer offsets of the ping-pong "
                       "kernel");
    const int bnw = g.N % 256 == 0 ? 256 : 128;
    const bool tapi = tap_inner_wanted(g, env);
    pp32(bnw, bnw == 256 ? (tapi ? GK_F16_PP32_256_TAPI : GK_F16_PP32_256)
                         : (tapi ? GK_F16_PP32_128_TAPI : GK_F16_PP32_128));
    p.family = MILAN_KERNEL_F16;
    if (tapi) {
      tap_inner();
      p.grid_x = tap_classes(g, env, p);
    }
    return p;
  }

  if (!cin32) {
    // per-lane taps (8-slot groups): only the narrow-N tile is built for it
    MILAN_PLAN_REQUIRE(g.Cin % 8 == 0 && g.N <= 64 && !g.A2, MILAN_ERR_SHAPE,
                       "gemm: split-f16 operands with Cin %% 32 != 0 need "
                       "Cin %% 8 == 0 and N <= 64 (Cin=%d N=%d)", g.Cin, g.N);
    return igemm(GK_IGEMM_256x64_C8_SPLIT, 256, 64, 2);
  }
  if (g.N <= 64) {
    // (N <= 64 on the split16 pipeline -- 512x64x3 / 256x64x4 tiles -- measured
    // 10-20 % SLOWER in round 2: these layers are bound by the L2 -> LDS operand
    // traffic of a 64-column tile, not by the pipeline depth.)
    // The k x k convs (layer1's 3x3) run on the split16 pipeline with 64 x 64 wave tiles
    // (256x64 block, 3-deep ring, 2 blocks per CU): round 2, same-box A/B: l1.x.c2 10.6 ->
    // 9.7 ms per pass.  The 1x1 layers measured 3-8 % SLOWER on it (and a 128x64 block slower
    // still), so they stay on the 2-stage kernel; tile_hint 6 / 10 force either.
    if (g.tile_hint != 10 && !g.A2 && (g.tile_hint == 6 || (g.tile_hint == 0 && !one_by_one))) {
      p.kernel = g.groups > 1 ? GK_TM2_GROUPED : GK_TM2;
      if (g.groups > 1) p.grid_y = g.groups;
      tiles(256, 64);
      p.threads = 256;
      ring_lds(3, 16);
      return p;
    }
    return igemm(GK_IGEMM_256x64_C32_SPLIT, 256, 64, 2);
  }
  MILAN_PLAN_REQUIRE(!g.chunk_major ||
                         (env.experiments && g.tile_hint == 0 && !g.A2 && g.Cin % 16 == 0),
                     MILAN_ERR_SHAPE,
                     "gemm: chunk-major k order: experiments build, split16 kernels");
  // Experiments: 3x3 / stride 1 with the chunk-major weight copy, input strip in LDS.  OFF by
  // default (MILAN_CONV3X3=1 or tile_hint 8 turn it on).  MEASURED in round 2
  // (profiles/r2_conv3x3_strip_experiment.txt): it cuts the HBM fetch of layer3's 3x3 convs
  // from 6.4 GB to under 1 GB per launch and the A-side DMA instructions by 4x, results pass
  // the same parity tests -- and the layers run 8-13 % SLOWER (l3.x.c2 51.8 vs 46.7 ms per
  // pass): the generic kernel's loop-invariant fragment addresses keep its MFMA / ds_read
  // stream tighter than the per-tap address arithmetic here, and the L2/MALL absorbs the
  // re-reads well enough that the saved traffic was not on the critical path.
  if (env.experiments && g.W3 && g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && !g.A2 &&
      g.Cin % 16 == 0 && g.a_pix_stride == g.Cin && g.Ho == g.H && g.Wo == g.Wd &&
      g.a_img_stride == (long)g.H * g.Wd * g.Cin && g.Wd + 1 <= 64 &&
      (g.tile_hint == 8 || (g.tile_hint == 0 && env.conv3x3)) && g.N % 128 == 0) {
    const int bn = g.N % 256 == 0 ? 256 : 128;
    p.kernel = bn == 256 ? GK_CONV3X3_256 : GK_CONV3X3_128;
    tiles(256, bn);
    p.threads = 2 * (bn / 64) * 64;
    const int strip = 4 * (4 * bn * 16 + 2 * 384 * 16 + 16 + (p.threads / 64) * 256);
    const int stage = p.threads / 64 * 32 * 68 * 4;
    p.lds = strip < stage ? stage : strip;
    return p;
  }
  if (env.experiments && g.tile_hint == 1) return igemm(GK_IGEMM_256x128x3_C32_SPLIT, 256, 128, 3);
  if (env.experiments && g.tile_hint == 2) return igemm(GK_IGEMM_128x128_C32_SPLIT, 128, 128, 2);

  // ---- the tile of an N > 64 split layer ----
  // Measured on the 4096-neuron workload (profiles/): the 4-wave 256x128 tile with 16-slot
  // k-tiles, a 3-deep ring and DMA pieces interleaved with the MFMA groups (2 workgroups per
  // CU) is the fastest split-mode configuration for every N > 64 layer; the others stay
  // reachable through tile_hint for experiments.
  // The kernel is chosen from the LAYER (N, K) only, never from the number of rows: different
  // tile configurations accumulate in different orders, and a description must not depend on
  // how many neurons shared its launch (chunk size, world size).  Short M just leaves tile rows
  // masked.
  int s16 = GK_S16_256x128x3, bm = 256, bn = 128, stages = 3;
  auto wide = [&]() { s16 = GK_S16_256x256x5; bn = 256; stages = 5; };
  const int pad256 = (g.N + 255) / 256 * 256 - g.N, pad128 = (g.N + 127) / 128 * 128 - g.N;
  if (env.experiments && g.tile_hint == 3) { s16 = GK_S16_256x256x4; bn = 256; stages = 4; }
  else if (env.experiments && g.tile_hint == 7) wide();
  else if (env.experiments && g.tile_hint == 4) {}
  else if (env.experiments && g.tile_hint == 5) { s16 = GK_S16_128x256x3; bm = 128; bn = 256; }
  // a grouped conv, or one group of it, stays on the 128-column tile at every width: the tile
  // that has a grouped form, so that both forms of the launch give the same bits
  else if (group_part(g)) {}
  // 256x256 tile, 5-deep ring = all 160 KB of LDS, four k-tiles in flight (round 3, same-box
  // A/B against the 4-deep ring: +0.5 % end to end, same bits)
  else if (g.N % 256 == 0) wide();
  // wide outputs that are not a multiple of 256 (the vocabulary GEMMs, N = 5004): the
  // 256-column tile when it pads no more than the 128-column one would (same-box A/B: decode
  // stage -0.5 ms; N = 3904 pads 4.9 % vs 1.6 % and is slower on it)
  else if (g.N > 2048 && pad256 <= pad128) wide();
  tiles(bm, bn);

  // ---- the ping-pong forms of the 256 x 128 x 3 and 256 x 256 x 5 tiles ----
  // MILAN_PP128=0 / MILAN_PP=0: the round-3 lockstep kernels instead (same bits; A/B timing).
  // MILAN_PP=2: the 16-slot ping-pong form (4-slot ring: 128 KB of LDS) everywhere.
  const bool pp_tile = (s16 == GK_S16_256x128x3 ? env.pp128 != 0 : s16 == GK_S16_256x256x5 && env.pp) &&
                       !g.chunk_major && pp_eligible(g);
  if (pp_tile && (bn == 128 || env.pp != 2) && pair_staged_ok(g)) {
    const bool tapi = tap_inner_wanted(g, env);
    if (g.row_list != nullptr) {
      // Row lists: the 256-column tile in the dense launch's k order (a k x k conv: tap-inner),
      // split rows written in place, when 256 + 2 images of either source lie within a 32-bit
      // byte offset and 257 images' pixels count exactly in fp32.  Anything else that carries
      // a row list is refused (plan_gemm).
      const long howo = (long)g.Ho * g.Wo;
      if (bn != 256 || g.tile_hint != 0 || knob_forced(env) || env.pp != 1 || g.N % 256 != 0 ||
          g.m_live == nullptr || g.m_live_mul != 1 ||
          !g.out_split || g.K != g.Kp || (!one_by_one && !tapi) || howo <= 0 ||
          g.M % howo != 0 || 257 * howo >= (1L << 24) ||
          258 * g.a_img_stride * 4 + 64 >= 0x7fffffffL ||
          (g.A2 && 258 * g.a2_img_stride * 4 + 64 >= 0x7fffffffL))
        return p;  // (no kernel named: not a list form)
      pp32(256, tapi ? GK_PP32L_TAPI : GK_PP32L);
      p.list = true;
      p.family = tapi ? MILAN_KERNEL_PP32T_256 : MILAN_KERNEL_PP32_256;
      if (tapi) tap_inner();
      p.tap_ncls = 0;
      return p;
    }
    if (g.groups > 1 && bn == 128) {
      // grouped convs: the 128-column tile only (group_part above; a forced 256-column tile
      // runs per group), one tile per workgroup, the group as grid.y; the k order is the
      // plain launch's
      pp32(128, tapi ? GK_GROUPED_PP32T : GK_GROUPED_PP32N);
      p.family = MILAN_KERNEL_PP32_128;
      p.grid_y = g.groups;
      if (tapi) {
        tap_inner();
        p.grid_x = tap_classes(g, env, p);
      }
      return p;
    }
    if (tapi) {
      pp32(bn, bn == 256 ? GK_PP32T_256 : GK_PP32T_128);
      p.family = bn == 256 ? MILAN_KERNEL_PP32T_256 : MILAN_KERNEL_PP32_128;
      tap_inner();
      p.grid_x = tap_classes(g, env, p);
      return p;
    }
    // MILAN_PP_PERSIST=1: persistent workgroups with the next tile's first pairs prefetched
    // under the epilogue (=2: only the K <= 512 launches).  Measured slower in every form --
    // static walk, short-K only, dynamic tile queue (profiles/r4_experiments.txt B, H, K): one
    // tile per workgroup (hardware dispatch) is the default.  The walk runs the same tiles in
    // the same k order: the same bits whichever M makes it start.
    const bool walk = env.pp_persist && (env.pp_persist != 2 || g.K <= 512) && p.grid_x > env.cus;
    pp32(bn, bn == 256 ? (walk ? GK_PP32N_256 : GK_PP32) : GK_PP32N_128);
    p.family = bn == 256 ? MILAN_KERNEL_PP32_256 : MILAN_KERNEL_PP32_128;
    if (walk) p.grid_x = env.cus;
    return p;
  }
  if (pp_tile && bn == 256) {
    p.kernel = GK_PP;
    p.threads = 512;
    p.lds = 4 * (256 + 256) * 16 * 4;  // (>= 8 waves x 32 x 68 floats: the epilogue stages through the ring)
    return p;
  }

  // ---- the lockstep split16 kernels ----
  if (env.experiments && env.sched == 1) return split16(s16, bm, bn, stages, 1);
  if (env.experiments && g.chunk_major) return split16(s16, bm, bn, stages, 2);
  if (env.experiments && !env.linear_kernel) return split16(s16, bm, bn, stages, 0);
  // 1x1 convolutions and Linear layers: the loop variant without tap arithmetic
  if (one_by_one && g.pad == 0 && g.A2 == nullptr) {
    // more tiles than CUs on the 256 x 256 x 5 tile: persistent workgroups, the next tile's A
    // rows prefetched under the epilogue (igemm_split16_linp_kernel).  The same tile function
    // in the same k order as SHAPE 3: the same bits whichever M makes it start.
    if (s16 == GK_S16_256x256x5 && (!env.experiments || env.persist_lin) &&
        g.Kp / 16 >= stages - 1 && p.grid_x > env.cus) {
      p.kernel = GK_LINP;
      p.threads = 512;
      p.lds = stages * (bm + bn) * 16 * 4;
      p.grid_x = env.cus;
      return p;
    }
    return split16(s16, bm, bn, stages, 3);
  }
  return split16(s16, bm, bn, stages, 0);
}

// The plan of launch_gemm(a): plan_launch() and the two questions that span launches.
//   Row lists: a launch that carries one has a pp32l plan or is refused.
//   Grouped convs: one launch when the leaf has a grouped instantiation (the general fp32
//   kernel, the 64-column split tile of the k x k convs, the 128-column pair-staged tile);
//   everything else -- MILAN_GROUP_LAUNCH=0 (the baseline), a forced tile or (split) kernel,
//   MILAN_PP128=0, the 1x1 convs with N <= 64, a layer beyond the pair-staged tile's 32-bit
//   offsets -- runs as one plain launch per group on offset pointers, the same kernel per group
//   as the grouped launch would run (group_part).
inline GemmPlan plan_gemm(const GemmArgs& a, const GemmEnv& env) {
  GemmPlan p = plan_launch(a, env);
  if (a.row_list != nullptr && (p.err != 0 || !p.list)) {
    p = GemmPlan{};
    p.err = MILAN_ERR_SHAPE;
    snprintf(p.msg, sizeof(p.msg), "gemm: no row-list form of this launch (N=%d Cin=%d %dx%d)",
             a.N, a.Cin, a.KH, a.KW);
    return p;
  }
  if (a.groups > 1 && p.err == 0) {
    const bool forced = p.tile_hint != 0 || (a.a_split && knob_forced(env));
    if (!env.group_launch || forced || p.grid_y == 1) {
      GemmArgs t = a;
      shift_group(t, 0);
      p = plan_launch(t, env);
      p.per_group = true;
    }
  }
  return p;
}
#undef MILAN_PLAN_REQUIRE

}  // namespace milan
