/* libmilan_hip -- C ABI of the MI355X-native MILAN inference path.
 *
 * The reference (evandez/neuron-descriptions) is pure Python and has no FFI
 * of its own; the seam this library sits behind is the Python class contract
 * of `src.milan.Decoder`.  Each entry point below is the
 * native counterpart of one reference method; the Python mirror in
 * neuron-descriptions_amd/milan_amd/ binds them with ctypes (INTEGRATION.md
 * shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Every data pointer is a DEVICE pointer owned by the caller (the Python
 *     side passes torch tensors' data_ptr()).  The library owns only its packed
 *     weight arena, freed by milan_destroy().
 *   - All work is enqueued on `stream` (a hipStream_t); no implicit sync except
 *     where documented (milan_finalize_weights).
 *   - Return 0 on success; negative = MILAN_ERR_*; positive = hipError_t.
 *     milan_last_error() returns a thread-local message for the last failure.
 *   - float = IEEE binary32 everywhere (the reference computes in fp32); token
 *     ids are int64 like torch.long.
 *   - One ctx per device; a ctx is not thread-safe.
 */
#ifndef MILAN_HIP_H
#define MILAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the prototypes of this header
 * are its whole dynamic symbol table (tests/test_host.py checks `nm -D`). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MILAN_ABI_VERSION 11

enum {
  MILAN_OK = 0,
  MILAN_ERR_ARG = -1,       /* bad argument (-> ValueError in Python)        */
  MILAN_ERR_SHAPE = -2,     /* shape/dim mismatch (-> ValueError)            */
  MILAN_ERR_STATE = -3,     /* call order (weights missing / not finalized)  */
  MILAN_ERR_WORKSPACE = -4, /* workspace too small                           */
  MILAN_ERR_NO_LM = -5,     /* MI / rerank requested without an LM
                               (src/milan/decoders.py:397-398)               */
  MILAN_ERR_INDEX = -6      /* a unit index beyond its layer's channel count
                               (-> IndexError, as `mask[:, units] = 0` raises
                               in src/utils/ablations.py:39)                 */
};

enum { MILAN_DTYPE_U8 = 0, MILAN_DTYPE_F32 = 1 };

/* src/milan/decoders.py:217-221; MILAN_FORCED = `strategy=<tensor>` (teacher
 * forcing, decoders.py:444-445). */
enum { MILAN_GREEDY = 0, MILAN_FORCED = 1, MILAN_BEAM = 2, MILAN_RERANK = 3 };

typedef struct milan_ctx milan_ctx;
typedef void* milan_stream; /* hipStream_t */

/* Model geometry.  Mirrors the constructor arguments of
 * src/milan/decoders.py:233-244, src/milan/lms.py:20-25 and the encoder
 * config of src/milan/encoders.py:326-351: all four pyramid configs --
 * 'resnet50'/'resnet101' (bottleneck blocks), 'resnet18' (basic blocks) and
 * 'alexnet'. */
enum {
  MILAN_TRUNK_BOTTLENECK = 0, /* taps conv1 + layer1..4, F = 61 * width      */
  MILAN_TRUNK_BASIC = 1,      /* same taps, expansion 1,   F = 16 * width      */
  MILAN_TRUNK_ALEXNET = 2,    /* taps features.0/3/6/8/10, F = 18 * width      */
  MILAN_TRUNK_NONE = 3,       /* decoder-only context (a foreign `Encoder`):
                                 any feature_size % 4 == 0, trunk_* ignored   */
  MILAN_TRUNK_ALEXNET_PLACES = 4, /* the Places365 AlexNet: conv1..conv5 with grouped
                                 convs, width / 32 x (96, 256, 384, 384, 256) channels,
                                 F = 43 * width.  Classify / ablate / activations
                                 only: the encoder entry points refuse it      */
  MILAN_TRUNK_VGG = 5         /* torchvision's VGG-11/13/16/19 without batch norm: five
                                 blocks of 3x3 convs, width x (1, 2, 4, 8, 8) channels,
                                 F = 23 * width; the block structure follows from the
                                 uploaded keys.  Classify / ablate / activations only   */
};
typedef struct milan_dims {
  int32_t trunk_width;      /* 64 for the torchvision models                */
  int32_t trunk_blocks[4];  /* {3,4,23,3} = resnet101 (unused for alexnet)   */
  int32_t feature_size;     /* 61 / 16 / 18 * trunk_width by trunk_kind      */
  int32_t hidden_size;      /* 512                                           */
  int32_t embedding_size;   /* 128                                           */
  int32_t attention_size;   /* min(hidden, feature) = 512 (decoders.py:50)   */
  int32_t vocab_size;       /* len(indexer) = |vocab| + 4                    */
  int32_t start_index;      /* |vocab|     (src/utils/lang.py:242-245)       */
  int32_t stop_index;       /* |vocab| + 1                                   */
  int32_t pad_index;        /* |vocab| + 2                                   */
  int32_t has_lm;           /* 0/1                                           */
  int32_t lm_hidden_size;   /* 512                                           */
  int32_t lm_embedding_size;/* 128                                           */
  int32_t lm_layers;        /* 2                                             */
  int32_t trunk_kind;       /* MILAN_TRUNK_* (0 = bottleneck ResNet)         */
} milan_dims;

int milan_abi_version(void);
const char* milan_last_error(void);

/* Lifetime.  Replaces Decoder.__init__ / Decoder.to(device). */
int milan_create(milan_ctx** out, int device, const milan_dims* dims);
void milan_destroy(milan_ctx* ctx);

/* Weight upload.  `name` is the key in the reference's Decoder.state_dict()
 * (src/utils/serialize.py:188-204), e.g. "lstm.weight_ih",
 * "attend.key_to_hidden.weight", "lm.lstm.weight_hh_l1",
 * "encoder.encoder.model.layer3.7.bn2.running_var".  `data` is a device float*
 * that must stay valid until milan_finalize_weights() returns.  Unknown names
 * ("...num_batches_tracked") are accepted and ignored; "...fc.weight" / "...fc.bias" of a
 * ResNet trunk are kept for milan_classify (the describe path never reads them).  Replaces load_state_dict
 * (src/utils/serialize.py:222-252). */
int milan_set_weight(milan_ctx* ctx, const char* name, const float* data,
                     const int64_t* shape, int ndim);
/* Folds eval-mode BatchNorm into the convolutions, repacks every matrix into
 * the kernels' layout inside a library-owned arena, then synchronises
 * `stream` (after which the caller may free the uploaded tensors). */
int milan_finalize_weights(milan_ctx* ctx, milan_stream stream);

/* Bytes of scratch the calls below need for at most `max_neurons` neurons of
 * `k` exemplars at image_size x image_size, `beam_size` beams, `length` steps. */
size_t milan_workspace_bytes(const milan_ctx* ctx, int max_neurons, int k,
                             int image_size, int beam_size, int length);

/* Decoder.encode / PyramidConvEncoder.forward
 * (src/milan/decoders.py:525-546, src/milan/encoders.py:286-320).
 * images: (n_images,3,H,W) NCHW, uint8 (0..255, converted exactly like
 * src/milannotations/datasets.py:191-197) or float in [0,1];
 * masks: (n_images,1,H,W) uint8 {0,1} or float, or NULL (= all ones).
 * features: (n_images, feature_size) float out. */
int milan_encode(milan_ctx* ctx, const void* images, int image_dtype,
                 const void* masks, int mask_dtype, int n_images, int height,
                 int width, float* features, void* workspace,
                 size_t workspace_bytes, milan_stream stream);

/* SpatialConvEncoder.forward (src/milan/encoders.py:158-230, config
 * 'resnet18'): the image is normalised, THEN multiplied by its mask (NULL =
 * ones), run through the ResNet trunk, and the last stage's output is returned
 * position-major: out (n_images, h4*w4, C4) = layer4.permute(0,2,3,1), i.e.
 * (n, 49, 512) for 224x224 / resnet18.  ResNet trunks only. */
int milan_encode_spatial(milan_ctx* ctx, const void* images, int image_dtype,
                         const void* masks, int mask_dtype, int n_images,
                         int height, int width, float* out, void* workspace,
                         size_t workspace_bytes, milan_stream stream);

/* Unit ablation and classification on the ResNet trunks: src/utils/ablations.py (`zero`,
 * `ablated`, ImageClassifier.predict) over torchvision's ResNet._forward_impl in eval mode.
 * The head comes from the state dict: when `<prefix>fc.weight` (classes, C4) and
 * `<prefix>fc.bias` were uploaded, milan_finalize_weights keeps them (fp32, as they are); the
 * class count is fc.weight's first extent.  A context without them behaves as before and the
 * classify calls return MILAN_ERR_STATE; an AlexNet context gets MILAN_ERR_ARG until
 * milan_set_alexnet_head (below) has installed its head.
 *
 * The five places an edit can sit are the reference's LAYERS.RESNET18 (src/exemplars/models.py:
 * 48-52), edited as nethook edits a module's OUTPUT: level 0 = `conv1`, the raw stem conv
 * output before bn1 / ReLU / maxpool; level L = `layerL`, the post-ReLU output of the stage's
 * last block.
 *   milan_set_ablation  installs the set {(levels[i], units[i])} (HOST arrays; count == 0
 *     clears it) as 0/1 channel masks in device memory owned by the context.  Order and
 *     duplicates do not matter.  A level outside 0..4 is MILAN_ERR_ARG, a unit outside the
 *     level's channels MILAN_ERR_INDEX.  Synchronises `stream`; the other calls do not.  Only
 *     the classify calls read the set: milan_encode* / milan_describe ignore it.
 *   milan_classify  images (n,3,H,W) float NCHW, fed AS THEY ARE (the reference's classifier
 *     gets normalised tensors: the context's mean / std are not applied); logits (n,classes)
 *     and predictions (n) int64 = argmax by torch's rule (lowest index among equal maxima, a
 *     NaN counts as the maximum); either may be NULL, not both.  Every level's tensor is
 *     multiplied by its mask before anything reads it.  Runs in MILAN_PRECISION_F32 or
 *     MILAN_PRECISION_SPLIT_F16 (MILAN_PRECISION_F16 is refused: MILAN_ERR_ARG); the head
 *     (average pool, fc) is exact fp32 in both, in a fixed summation order that depends on
 *     neither n nor the launch grid, so a batch gives the bits of its parts.  Saturation of
 *     the split format is reported through the status word.  Sub-batches of MILAN_ENC_SUB.
 *   milan_classify_sweep  for every listed unit j (HOST arrays levels / units) the result of
 *     milan_classify under the set `current + {(levels[j], units[j])}`, bit for bit: the same
 *     kernels on the same operands.  predictions (count,n) int64 or NULL; correct (count) int32
 *     = #{i : predictions[j][i] == targets[i]} or NULL (then targets, (n) int64, is NULL
 *     too); not both NULL.  Units are grouped by level: the forward up to and including the
 *     level runs once per sub-batch and is held, each unit costs one masked copy of the held
 *     tensor plus the rest of the network; level-4 units run the head alone.
 *   milan_classify_workspace_bytes  scratch for n_images at H x W; sweep_units = the largest
 *     `count` of a milan_classify_sweep call (0: milan_classify only).
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
int milan_set_ablation(milan_ctx* ctx, const int32_t* levels, const int32_t* units,
                       int count, milan_stream stream);
size_t milan_classify_workspace_bytes(const milan_ctx* ctx, int n_images, int height,
                                      int width, int sweep_units);
int milan_classify(milan_ctx* ctx, const float* images, int n_images, int height,
                   int width, float* logits, int64_t* predictions, void* workspace,
                   size_t workspace_bytes, milan_stream stream);
int milan_classify_sweep(milan_ctx* ctx, const float* images, int n_images, int height,
                         int width, const int32_t* levels, const int32_t* units, int count,
                         const int64_t* targets, int32_t* correct, int64_t* predictions,
                         void* workspace, size_t workspace_bytes, milan_stream stream);

/* Activation taps on the ResNet trunks: what nethook.retain_layers hands out for the five
 * layers above, computed by the walk of milan_classify.
 *   milan_activations  images (n,3,H,W) float NCHW, fed as they are (milan_classify's
 *     contract).  levels: a HOST array of `count` >= 1 distinct levels in 0..4, in any order;
 *     outputs[i]: a DEVICE pointer to (n, C_level, h_level, w_level) fp32 NCHW for levels[i]
 *     (the layout the exemplar kernels read), `outputs` itself a HOST array.  The tensor is the
 *     module's OUTPUT after the installed ablation set's mask: what the next layer reads.
 *     Level 0 is the raw stem conv output (negative values included; a zero is always handed
 *     out as +0, also where the mask's product with a negative value was -0).  The walk runs once per
 *     sub-batch (MILAN_ENC_SUB) up to the highest requested level and no further; no head
 *     runs, so a context without fc.weight is accepted.  Each requested level is converted
 *     from the trunk's layout (NHWC, fp32 or split f16 at the activation scale, which is
 *     removed exactly) when it is produced.  Runs in MILAN_PRECISION_F32 or
 *     MILAN_PRECISION_SPLIT_F16; MILAN_PRECISION_F16 and a headless AlexNet: MILAN_ERR_ARG, as is a level
 *     outside 0..4 or one listed twice.  Saturation goes to the status word; no host
 *     synchronisation.
 *   milan_activations_workspace_bytes  scratch for n_images at H x W.
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
size_t milan_activations_workspace_bytes(const milan_ctx* ctx, int n_images, int height,
                                         int width);
int milan_activations(milan_ctx* ctx, const float* images, int n_images, int height, int width,
                      const int32_t* levels, int count, float* const* outputs,
                      void* workspace, size_t workspace_bytes, milan_stream stream);

/* The same calls on AlexNet: `alexnet_seq` (conv1..conv5, fc6, fc7, linear8) in eval mode, the
 * second CNN of the reference's editing experiment.  An AlexNet context (features.0/3/6/8/10)
 * answers milan_set_ablation / milan_classify* / milan_activations* with MILAN_ERR_ARG, as
 * described above, until this call has installed its three Linear layers; `classifier.1/4/6`
 * keys of the state dict switch nothing on.
 *   milan_set_alexnet_head  DEVICE fp32 pointers: row-major weights (out, in) and biases (out).
 *     fc6_in must be C5 x 36 (C5 = features.10's channels), fc7_in == fc6_out, linear8_in ==
 *     fc7_out (MILAN_ERR_SHAPE otherwise); linear8_out is the class count.  The weights are
 *     packed into memory the context owns; the call synchronises `stream`, and the caller's
 *     tensors may go afterwards.  Calling it again with the same widths replaces the values.
 * From then on: levels 0..4 are conv1..conv5, each tensor relu(conv + bias) x mask, which is
 * what the next layer reads and what milan_activations hands out (level 0 too: post-ReLU, fp32
 * in both precision modes).  The tail -- 3x3/2 max-pool, AdaptiveAvgPool2d((6, 6)), flatten in
 * (C, h, w) order -- and the three Linear layers are exact fp32 in both modes; dropout is the
 * identity.  Images are fed as they are and must be at least 63 x 63 (MILAN_ERR_SHAPE).
 * milan_encode* on the context is unchanged.
 *
 * The Linear layer itself, without a context: y (rows, n_out) = act(x (rows, n_in) W^T + bias)
 * on the fp32 MFMA, act = ReLU when `relu` != 0, bias may be NULL.  The summation order of an
 * output depends on n_in alone (zero-padded to a multiple of 8; chunks of 256 each summed from
 * zero by one k-ordered fmaf chain; chunks j, j + 4, ... added in order into four totals;
 * (t0 + t1) + (t2 + t3), then the bias): a batch gives the bits of its rows.
 *   milan_linear_packed_bytes / milan_linear_pack  the packed copy of a row-major (n_out, n_in)
 *     weight that milan_linear reads, once per weight.
 *   milan_linear_rowwise  the ResNet head's kernel (one wavefront per output and row) on a
 *     row-major weight: kept callable as the baseline of tools/bench_alexnet.py.
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
int milan_set_alexnet_head(milan_ctx* ctx, const float* fc6_weight, const float* fc6_bias,
                           int fc6_out, int fc6_in, const float* fc7_weight,
                           const float* fc7_bias, int fc7_out, int fc7_in,
                           const float* linear8_weight, const float* linear8_bias,
                           int linear8_out, int linear8_in, milan_stream stream);
size_t milan_linear_packed_bytes(int n_out, int n_in);
int milan_linear_pack(const float* weight, int n_out, int n_in, float* packed,
                      milan_stream stream);
int milan_linear(const float* x, const float* packed, const float* bias, int rows, int n_in,
                 int n_out, int relu, float* y, milan_stream stream);
int milan_linear_rowwise(const float* x, const float* weight, const float* bias, int rows,
                         int n_in, int n_out, float* y, milan_stream stream);

/* The same calls on the Places365 AlexNet (MILAN_TRUNK_ALEXNET_PLACES; the reference's
 * src/deps/alexnet.py): conv1 11x11 / 4 / pad 0, pool 3/2 [, LRN], conv2 5x5 / pad 2 in 2 groups,
 * pool 3/2 [, LRN], conv3 3x3 dense, conv4 and conv5 3x3 in 2 groups, pool 3/2, flatten in
 * (C, h, w) order, fc6 / fc7 / fc8 with ReLU after the first two.  Channels are width / 32 x
 * (96, 256, 384, 384, 256), width a multiple of 8.  The state dict's keys are
 * `<prefix>conv1.weight` .. `<prefix>conv5.bias`; a conv's group count follows from its weight
 * shape (cout, cin / groups, kh, kw), so dense weights (groups of 1) run as well.  A grouped
 * conv is ONE launch with the group as a grid dimension (MILAN_GROUP_LAUNCH=0: one launch per
 * group on offset pointers, the same bits).  A level whose per-group input width is not a
 * multiple of 32 runs in fp32 in both precision modes.
 *   Levels 0..4 are conv1..conv5 with the AlexNet semantics above: relu(conv + bias) x mask,
 * before the pool and the LRN; a zero is handed out as +0.  The head is installed with
 * milan_set_alexnet_head (its third layer is fc8 here).  milan_classify* needs an image that
 * leaves 6 x 6 after pool5 (227 x 227, the reference's size, up to 258; MILAN_ERR_SHAPE
 * otherwise: there is no adaptive pool); milan_activations needs no head and takes any image
 * that leaves 3 x 3 before every pool it has to cross (35 x 35 reaches every level).  MILAN_PRECISION_F16 and the milan_encode* calls: MILAN_ERR_ARG.
 *   milan_set_alexnet_lrn  the optional across-channel LRN after pool1 and pool2:
 *     y = x / (1 + alpha * S / local_size)^beta, S = the sum of squares over the local_size
 *     neighbouring channels, zero-padded (the divisor is always local_size).  local_size odd
 *     and at most 17, 0 = off (the default); a context of another trunk kind or any other
 *     size: MILAN_ERR_ARG.  beta == 0.75 is computed as sqrt(d) * sqrt(sqrt(d)), other values by powf.
 *   milan_lrn  the LRN kernel alone on a DEVICE tensor (pixels, channels) with the channels of
 *     a pixel contiguous, channels % 8 == 0, 16-byte aligned, x and y apart: fp32, or with
 *     `split` != 0 split f16 groups at scale 1, in and out.  `status`: a device status word or NULL.
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
int milan_set_alexnet_lrn(milan_ctx* ctx, int local_size, float alpha, float beta);
int milan_lrn(const float* x, long long pixels, int channels, int split, int local_size,
              float alpha, float beta, float* y, unsigned* status, milan_stream stream);

/* The same calls on torchvision's VGG-11 / 13 / 16 / 19 without batch norm (MILAN_TRUNK_VGG):
 * five blocks of 3x3 / pad 1 / stride 1 convs with bias and ReLU, a 2x2 / 2 max-pool after each
 * block, AdaptiveAvgPool2d((7, 7)), flatten in (C, h, w) order and three Linear layers with ReLU
 * after the first two (dropout is the identity).  milan_dims::trunk_blocks has four entries and
 * a VGG five blocks, so the structure follows from the uploaded keys: `<prefix>vgg.B.J.weight` /
 * `.bias` with block B = 1..5 and conv J = 0..3, contiguous from 0, one to four convs per
 * block (the caller renames torchvision's `features.N`).  Block B has width x min(2^(B-1), 8)
 * output channels, width a multiple of 8; anything else is MILAN_ERR_SHAPE at
 * milan_finalize_weights.
 *   Levels 0..4 are the last conv of blocks 1..5 (the reference's LAYERS.VGG11 .. VGG19) with
 * the AlexNet semantics above: relu(conv + bias) x mask, which is what the pool reads and what
 * milan_activations hands out; a zero is handed out as +0.  Every extent is floor(x / 2) per
 * pool: reaching level l needs H, W >= 2^l, a classify call H, W >= 32 (MILAN_ERR_SHAPE before
 * anything is launched).  In MILAN_PRECISION_SPLIT_F16 a conv multiplies split operands when its
 * input width is a multiple of 32 and its input was written in split format (by a pool, by the
 * first conv's kernel or by a split conv); the others run in exact fp32.  The tail and the
 * Linear layers are exact fp32 in both modes, each adaptive-pool bin summed from zero in
 * row-major order and divided by its count.  A headless context taps and ablates; classifying
 * without a head is MILAN_ERR_STATE.  MILAN_PRECISION_F16 and the milan_encode* calls:
 * MILAN_ERR_ARG.
 *   milan_set_vgg_head  milan_set_alexnet_head's contract for classifier.0 / .3 / .6; fc0_in
 *     must be C5 x 49.  On a context of another kind, and milan_set_alexnet_head on this one:
 *     MILAN_ERR_ARG.
 *   milan_vgg_trace  what the walks of the context's last classify / classify_sweep /
 *     activations call did, per conv slot 4 (B - 1) + J (HOST arrays of 20 entries):
 *     launches[slot] = how often the conv was launched, split[slot] = 1 when its last launch
 *     multiplied split operands.  Either may be NULL.
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
int milan_set_vgg_head(milan_ctx* ctx, const float* fc0_weight, const float* fc0_bias,
                       int fc0_out, int fc0_in, const float* fc3_weight, const float* fc3_bias,
                       int fc3_out, int fc3_in, const float* fc6_weight, const float* fc6_bias,
                       int fc6_out, int fc6_in, milan_stream stream);
int milan_vgg_trace(const milan_ctx* ctx, int32_t* launches, int32_t* split);

/* Decoder.init_state (src/milan/decoders.py:548-574).
 * features (n,k,F) -> h,c (n,hidden). */
int milan_init_state(milan_ctx* ctx, const float* features, int n, int k,
                     float* h, float* c, void* workspace,
                     size_t workspace_bytes, milan_stream stream);

/* Decoder.step (src/milan/decoders.py:576-634), eval mode.
 * features (rows,k,F); tokens (rows) int64; h,c (rows,hidden) in;
 * h_lm,c_lm (lm_layers,rows,lm_hidden) in/out or NULL (no MI);
 * predictions (rows,V), attentions (rows,k), h_out,c_out (rows,hidden) out. */
int milan_step(milan_ctx* ctx, const float* features, int rows, int k,
               const int64_t* tokens, const float* h, const float* c,
               float* h_lm, float* c_lm, float temperature, float* predictions,
               float* attentions, float* h_out, float* c_out, void* workspace,
               size_t workspace_bytes, milan_stream stream);

/* Decoder.forward on features (src/milan/decoders.py:335-523), eval mode.
 *   strategy MILAN_GREEDY: tokens (n,length), scores (n); predictions
 *     (n,length,V) and attentions (n,length,k) optional (may be NULL);
 *     beam_* must be NULL.  mi = use the LM per step (decoders.py:624-630).
 *   strategy MILAN_FORCED: as MILAN_GREEDY but the token fed to step t+1 is
 *     tokens[:, t] -- `tokens` (n,length) is an INPUT holding the forced ids
 *     (0 <= id < V, validated by the caller) and is left unchanged, scores
 *     accumulate predictions[b, t, tokens[b, t]] (what Decoder.score sums,
 *     decoders.py:636-711); predictions is required.
 *   strategy MILAN_BEAM / MILAN_RERANK: allennlp-2.10 BeamSearch semantics
 *     (decoders.py:467-484) then best-of-beam / LM rerank (decoders.py:492-512).
 *     beam_tokens (n,beam,length) int64, beam_scores (n,beam),
 *     tokens (n,length), scores (n).  The search always runs `length` steps;
 *     out_len[g] receives T' (the length allennlp would have returned for
 *     neuron group g, groups of `group_size` consecutive neurons = the
 *     reference's forward batch), positions >= T' hold stop_index.  Rerank LM
 *     scores use only the first T' tokens, as the reference does.
 *     out_len is a DEVICE int32 array of ceil(n/group_size) entries. */
int milan_decode(milan_ctx* ctx, const float* features, int n, int k,
                 int strategy, int length, int beam_size, int mi,
                 float temperature, int group_size, int64_t* tokens,
                 float* scores, float* predictions, float* attentions,
                 int64_t* beam_tokens, float* beam_scores, int32_t* out_len,
                 void* workspace, size_t workspace_bytes, milan_stream stream);

/* Beam width.  1 <= beam_size <= min(vocab_size, 1024); above 256 beams vocab_size must not
 * exceed 36864 (the wide per-row top-k holds the row in LDS), else MILAN_ERR_ARG.  While a neuron's beam_size^2
 * summed candidates fit 64 KiB of LDS (beam_size <= 124) they are merged there, exactly as
 * before wide beams existed; from there on the merge reads them from
 * global memory (every parent's list is sorted, so a threshold bisection with a binary
 * search per parent finds the winners), and above 256 the per-row top-k runs its own
 * kernels too (csrc/beam_wide.hip).  Both paths select by one rule -- value
 * descending, ties to the lowest flat candidate index -- and give the same bits.
 *   milan_set_beam_path  mode 0 (default): by width, as above.  mode 1: the wide merge at
 *     every beam_size >= 2 and the wide per-row top-k wherever it applies.  An A/B and
 *     test knob; results do not depend on it.
 *   milan_beam_merge  one merge step on caller-supplied DEVICE arrays: per neuron the
 *     `beam` best of cand_v[n][p][j] + last_lp[n][p] (last_lp NULL = zeros) over
 *     p < beam_prev, j < beam.  Every list cand_v[n][p][:] must be sorted descending, as
 *     the per-row top-k emits it.  new_lp (n,beam) is sorted by (value descending, flat
 *     index p * beam + j ascending), new_tok = cand_i at the winner, new_bp = its p.
 *     1 <= beam_prev <= beam <= 1024.  wide: 0 = the kernel milan_decode picks for this
 *     `beam` in mode 0, 1 = the wide kernel.  workspace may be NULL (no scratch is used).
 *   milan_row_select  one per-row top-k on caller-supplied DEVICE arrays: per row the k
 *     best of log_softmax(logits) [- lambda * log_softmax(lm_logits)] (lm_logits NULL =
 *     none), logits (rows,V); cand_v / cand_i (rows,k) sorted by (value descending, index
 *     ascending).  A row with last_tok[row] == stop (last_tok NULL = no such row) gets the
 *     forced candidates of a finished beam.  1 <= k <= min(V, 1024).  path: 0 = the kernel
 *     milan_decode picks in mode 0, 1 = the wide kernels (k >= 2, V <= 36864), 2 = the
 *     threshold path and 3 = the first rank-count path of the register kernel (both
 *     2 <= k <= 256, V <= 6144); a shape the path does not take is MILAN_ERR_ARG.  Every
 *     path gives the same bits.
 * Not part of every build of ABI 11: probe with dlsym / hasattr. */
int milan_row_select(const float* logits, const float* lm_logits, float lambda, int rows,
                     int V, int k, const int64_t* last_tok, int stop, float* cand_v,
                     int* cand_i, int path, milan_stream stream);
int milan_beam_merge(const float* cand_v, const int* cand_i, const float* last_lp,
                     int n, int beam_prev, int beam, int wide, float* new_lp,
                     int* new_tok, int* new_bp, void* workspace,
                     size_t workspace_bytes, milan_stream stream);
int milan_set_beam_path(milan_ctx* ctx, int mode);   /* default 0 */
int milan_get_beam_path(const milan_ctx* ctx);

/* LanguageModel.forward(inputs, reduce=True) (src/milan/lms.py:58-101),
 * including its stop-mask off-by-one.  seqs (rows,L) int64, first column is
 * the start token; out (rows).  seq_len: optional DEVICE int32 per row giving
 * the number of valid columns (<= L) or NULL (= L). */
int milan_lm_score(milan_ctx* ctx, const int64_t* seqs, int rows, int L,
                   const int32_t* seq_len, float* out, void* workspace,
                   size_t workspace_bytes, milan_stream stream);

/* LanguageModel.forward(inputs, reduce=False) (src/milan/lms.py:58-88): the
 * log-probabilities of every next token at every position.  seqs (rows,L)
 * int64; out (rows,L,V).  Used for custom `masks=` reductions and analysis;
 * the rerank path uses milan_lm_score, which never materialises this. */
int milan_lm_logprobs(milan_ctx* ctx, const int64_t* seqs, int rows, int L,
                      float* out, void* workspace, size_t workspace_bytes,
                      milan_stream stream);

/* The whole hot path for one batch = Decoder.forward(images, masks, ...)
 * (what Decoder.predict calls per batch, src/milan/decoders.py:857-865):
 * encode then decode.  images (n,k,3,H,W), masks (n,k,1,H,W); other
 * arguments as milan_decode.  features_out (n,k,F) optional. */
int milan_describe(milan_ctx* ctx, const void* images, int image_dtype,
                   const void* masks, int mask_dtype, int n, int k, int height,
                   int width, int strategy, int length, int beam_size, int mi,
                   float temperature, int group_size, float* features_out,
                   int64_t* tokens, float* scores, float* predictions,
                   float* attentions, int64_t* beam_tokens, float* beam_scores,
                   int32_t* out_len, void* workspace, size_t workspace_bytes,
                   milan_stream stream);

/* hipGraph capture of the decode stage.  When enabled, milan_decode (and the
 * decode half of milan_describe) records its launches -- the whole
 * Decoder.forward search of src/milan/decoders.py:418-512 for one batch -- into
 * a hipGraph the second time an identical call (same sizes AND same buffer
 * pointers, same stream) is seen, and replays it with one hipGraphLaunch from
 * then on.  Requires a non-default stream and caller-side buffer reuse;
 * otherwise (or while milan_profile_enable is on) calls run as plain launches.
 * milan_graph_stats reports how many graphs were captured / replayed. */
int milan_set_graph_capture(milan_ctx* ctx, int enable);
int milan_graph_stats(const milan_ctx* ctx, long long* captures,
                      long long* replays);

/* Arithmetic mode of every dense contraction (convs, Linear, LSTM gates).
 *   MILAN_PRECISION_F32       fp32-in / fp32-accumulate MFMA: bitwise an fmaf
 *                             chain, the reference's precision (default).
 *   MILAN_PRECISION_SPLIT_F16 operands carried as (hi,lo) f16 pairs (22
 *                             significant bits), A.B = Ah.Bh + Ah.Bl + Al.Bh on
 *                             the f16 matrix cores with fp32 accumulation:
 *                             fp32-GEMM-class error at 1/3 of the f16 MFMA rate.
 * Switchable at any time between calls (both weight packings are kept).
 *
 * In split mode the ResNet trunks keep their activations multiplied by a power of two
 * (2^5; environment MILAN_ACT_SCALE_LOG2=<0..10>, read by milan_create): the `lo` half of
 * an operand then stays in the f16 normal range down to activations of ~0.004 (1e-3-scale
 * networks stay in the fp32 error class), while `hi` saturates at 65504 / 2^k (2047).  The
 * scale is invisible at this interface: features, spatial features and descriptions are
 * returned unscaled, and 2^0 reproduces the unscaled storage bit for bit. */
enum { MILAN_PRECISION_F32 = 0, MILAN_PRECISION_SPLIT_F16 = 1,
       /* "Fast mode" (SURVEY 7 hard part 1): NARROWER than the reference's fp32
        * -- a reported extra, never the default and never the headline.  layer3 / layer4 of a
        * bottleneck ResNet trunk run on plain f16 operands (11 significant bits), one f16 MFMA
        * per product with fp32 accumulation, activations stored as 2 bytes per element;
        * everything else (stem, layer1 / layer2, decoder, LM) stays MILAN_PRECISION_SPLIT_F16.
        * Error class 2^-11 of the operand scale; bench.py reports its caption-flip rate against
        * MILAN_PRECISION_F32 next to its throughput. */
       MILAN_PRECISION_F16 = 2 };

/* Cross-layer fusions of the trunk (split-f16 mode; results are bitwise those of
 * the unfused schedule, so this is a scheduling knob for A/B timing and tests):
 *   MILAN_FUSE_CHAIN  a bottleneck's 1x1 expand conv (+ residual + ReLU) and the next
 *                     bottleneck's 1x1 reduce conv run as one launch
 *                     (csrc/chain.hip; torchvision Bottleneck.forward as called from
 *                     src/milan/encoders.py:298).
 *   MILAN_FUSE_STEM   conv1 7x7/2 + bn1 + ReLU + maxpool 3x3/2 as one persistent
 *                     launch over LDS-resident input tiles (csrc/stem.hip; the raw
 *                     conv1 tensor, pyramid level 0 of encoders.py:303-320, is only
 *                     materialised where the mask-weighted pooling reads it).
 *   MILAN_FUSE_CONV3  the 64 -> 64 channel 3x3 convolutions of layer1 as a persistent
 *                     kernel with register-resident weights and an LDS-resident input
 *                     tile (csrc/conv3.hip) instead of the implicit GEMM.
 *   MILAN_FUSE_SKIP_EMPTY  exemplars whose mask is all zero pool exact zeros at every
 *                     pyramid level whatever the trunk computes (src/milan/encoders.py:
 *                     310-317): they are left out of the trunk pass (uint8 images).  The
 *                     number of images with work stays ON THE DEVICE (round 6): every
 *                     trunk launch is sized for the whole batch and reads the count
 *                     itself, workgroups beyond it exit -- nothing is read back and
 *                     the stream is never synchronised (rounds 5's form did both).
 *   MILAN_FUSE_BNECK  (round 6; needs MILAN_FUSE_CHAIN) layer1's 3x3 convolution -- and for the
 *                     stage's first block its own 1x1 reduce conv -- run inside the block's
 *                     chain launch, from an LDS copy of the input region (csrc/chain.hip,
 *                     chain_kernel<.., CONV[, C1]>): the bottleneck's intermediate tensors
 *                     (torchvision Bottleneck.forward: out of conv1 / conv2) never exist in
 *                     memory.
 *   MILAN_FUSE_SPARSE_TAIL  (round 6) the last stage's output is read by nothing but the
 *                     level-4 pooling of src/milan/encoders.py:303-320, at the pixels under
 *                     the shrunk mask: the last two bottlenecks run only at those pixels and
 *                     the 3x3 neighbourhoods they depend on (row sets built on the device
 *                     from the pooling's own pixel lists; dense when no masks are given).
 *   MILAN_FUSE_TAIL_LISTS  (needs MILAN_FUSE_SPARSE_TAIL: the flag without it is rejected) those
 *                     row sets are handed to the GEMM tile itself as device-side row lists: a tile is 256 listed pixels, reads
 *                     its operand rows and writes its output rows in place in the dense tensors
 *                     -- no gather / scatter / im2col copies -- and the same treatment reaches
 *                     down to the first block of the last stage (its c1 at the pixels its
 *                     strided 3x3 reads) and to c2 / c3 of the last block of the stage before
 *                     (at those pixels, the downsample's and the level-3 pooling's).  Same bits.
 * Default: all eight (environment MILAN_CHAIN=<flags> overrides at context creation).
 * Not a flag but the same idea in the decoder: the rerank pass (decoders.py:495-512) scores
 * one LM row per distinct beam PREFIX instead of one per beam (csrc/decoder.hip,
 * lm_score_dedup; MILAN_LM_DEDUP=0 restores every row; same bits). */
enum { MILAN_FUSE_CHAIN = 1,       /* planes <= 128 (layer1, layer2): HBM-bound, wins */
       MILAN_FUSE_CHAIN_WIDE = 2,  /* planes 256 (layer3): the role ping-pong of csrc/chain3.hip
                                      (round 5) */
       MILAN_FUSE_STEM = 4,
       MILAN_FUSE_CONV3 = 8,       /* layer1's 3x3 convs: weights in registers (csrc/conv3.hip) */
       MILAN_FUSE_SKIP_EMPTY = 16,
       MILAN_FUSE_BNECK = 32,      /* layer1: the 3x3 conv in front of the chain launch (round 6) */
       MILAN_FUSE_SPARSE_TAIL = 64,    /* the last two bottlenecks only at the pixels the level-4
                                          pooling (and their 3x3 neighbourhoods) read (round 6) */
       MILAN_FUSE_TAIL_LISTS = 128 };  /* ... on row lists inside the GEMM tile, and extended down
                                          to the last block of the stage before */
int milan_set_fusion(milan_ctx* ctx, int flags);
int milan_set_precision(milan_ctx* ctx, int precision);
int milan_get_precision(const milan_ctx* ctx);

/* Image sharing (opt-in, default off; csrc/share.hip).  The reference runs the
 * trunk on the unmasked image and the masks enter at the pooling only (src/milan/encoders.py:
 * 295-318): the features of an exemplar slot are pool(trunk(image), mask).  With sharing
 * enabled, slots of ONE ENCODER PASS that hold byte-identical uint8 images go through the
 * trunk once and every slot pools its own mask from that result; the features are bit for
 * bit those of the unshared pass.  Identity is decided by comparing bytes (a 64-bit hash only
 * selects the candidates), so two different images are never merged.
 *   Scope: one encoder pass = MILAN_ENC_SUB images (default 9600: one 640-neuron chunk of 15
 *     exemplars).  Duplicates in different passes, chunks or calls are NOT shared.
 *   Applies to: the pooled encode (milan_encode, the encode half of milan_describe) of a
 *     ResNet trunk over uint8 images, outside calibration; `masks` may be NULL.
 *   Accepted and ignored for: float images (they may carry NaN pixels and take the full
 *     pass), milan_encode_spatial and the AlexNet pyramid: such a pass runs exactly as
 *     without the flag and counts slots == trunk_images.
 *   milan_image_sharing_stats: cumulative over the encoder passes run WHILE SHARING WAS
 *     ENABLED since creation / the last clear: exemplar slots seen, and images that actually
 *     went through the trunk.  The counters live on the device and are added to by a kernel of
 *     the pass: milan_encode / milan_describe read nothing back, stay free of synchronisation
 *     and capturable into a hipGraph.  This call synchronises `stream` (like milan_status).
 *   MILAN_SHARE_HASH_BITS=<0..64> (read at milan_create, default 64) keeps only that many low
 *     bits of the hash: a test knob (0: every pair of slots is compared byte for byte).
 * MILAN_ABI_VERSION did not change with these entry points: probe for them
 * (dlsym / hasattr(lib, "milan_set_image_sharing")). */
int milan_set_image_sharing(milan_ctx* ctx, int enable);   /* default 0 */
int milan_get_image_sharing(const milan_ctx* ctx);
int milan_image_sharing_stats(milan_ctx* ctx, long long* slots,
                              long long* trunk_images, int clear,
                              milan_stream stream);

/* Split-f16 mode fails LOUDLY (round 5).  The reference computes in plain fp32
 * (src/milan/encoders.py:295-320) and never saturates; the (hi, lo) f16 storage clamps
 * |x * 2^act_scale_log2| at 65504.  Every kernel that writes split format keeps the running
 * maximum of what it clamped and ORs MILAN_STATUS_SATURATED into the context's device status
 * word when the clamp was hit; the input conversion ORs MILAN_STATUS_NONFINITE_INPUT when a
 * float pixel was NaN / Inf (the features of such an image are NaN at every pyramid level,
 * exactly as the reference's pooling of NaN x mask yields them).
 *   milan_status            copies the word to *flags (host), optionally clearing it;
 *                           synchronises `stream`.  The Python mirror reads it after every
 *                           encode / describe and raises FloatingPointError on
 *                           MILAN_STATUS_SATURATED (or reruns the call in MILAN_PRECISION_F32
 *                           when Decoder.precision == 'auto').
 *   milan_set_act_scale_log2 activation scale 2^k of the split trunk, k in [0, 10]
 *                           (replaces the MILAN_ACT_SCALE_LOG2 default of 5): `hi` saturates
 *                           at 65504 / 2^k, `lo` leaves the f16 normal range below
 *                           2^-3 / 2^k.  Rewrites the pre-scaled bias vectors in place.
 *   milan_encoder_absmax    calibration: runs the trunk in MILAN_PRECISION_F32 over a sample
 *                           and returns the largest |activation| of every tensor the split
 *                           trunk would store (*absmax, host); Decoder.calibrate picks the
 *                           scale from it.  Synchronises `stream`. */
enum { MILAN_STATUS_SATURATED = 1, MILAN_STATUS_NONFINITE_INPUT = 2 };
int milan_status(milan_ctx* ctx, uint32_t* flags, int clear, milan_stream stream);
int milan_set_act_scale_log2(milan_ctx* ctx, int log2_scale, milan_stream stream);
int milan_get_act_scale_log2(const milan_ctx* ctx);
int milan_encoder_absmax(milan_ctx* ctx, const void* images, int image_dtype,
                         int n_images, int height, int width, float* absmax,
                         void* workspace, size_t workspace_bytes,
                         milan_stream stream);

/* The split-f16 decoder's feature scale.  The decoder's feature-carrying operands (the pooled
 * features of init_h / init_c, the features of the hoisted key_to_hidden, the gated context of
 * the cell's [emb | ctx * gate | h]) are converted to split format as x * 2^k and the factor is
 * undone exactly (accumulator scale; feature columns of the cell's split weight copy), so
 * features far below 1 keep the fp32 class (`lo` leaves the f16 normal range below
 * 2^-3 / 2^k) and features above 65504 / 2^k are reported (MILAN_STATUS_SATURATED).  A
 * property of the context, never of a call's data; default 2^0, at which every bit is what
 * it was before this entry point existed.  The exact-fp32 mode does not know about it.
 *   milan_set_feature_scale_log2  k in [-MAX, MAX]; rewrites the cell's split weight copy,
 *                           drops captured decode graphs, synchronises `stream`.
 *   milan_get_feature_absmax     what bounds |feature| for the last milan_encoder_absmax
 *                           sample under ANY mask: the largest |value| of the five pyramid
 *                           taps (a pooled feature is a mask-weighted mean of them); 0 before
 *                           the first.
 *   milan_set_embedding_scale_log2  the same for the embedding columns of the two LSTM inputs
 *                           (decoder and LM layer 0): the tables are gathered as e * 2^k, those
 *                           weight columns hold W / 2^k; an embedding beyond 65504 / 2^k is
 *                           reported.  milan_get_embedding_absmax: the largest |entry| of the
 *                           tables (computed on first use, on the legacy stream).
 * A NaN feature is not a saturation: it crosses the conversion as an f16 NaN and poisons what
 * fp32 arithmetic would poison.
 * MILAN_ABI_VERSION did not change with these entry points: probe for them. */
#define MILAN_FEATURE_SCALE_LOG2_MAX 30
int milan_set_feature_scale_log2(milan_ctx* ctx, int log2_scale, milan_stream stream);
int milan_get_feature_scale_log2(const milan_ctx* ctx);
float milan_get_feature_absmax(const milan_ctx* ctx);
int milan_set_embedding_scale_log2(milan_ctx* ctx, int log2_scale, milan_stream stream);
int milan_get_embedding_scale_log2(const milan_ctx* ctx);
float milan_get_embedding_absmax(milan_ctx* ctx);

/* Measurement hook (bench.py's roofline leg): while enabled, every launch of
 * the implicit-GEMM MFMA kernel is bracketed by HIP events on its launch
 * stream.  milan_profile_read synchronises the device and returns the summed
 * kernel time (ms), the algorithmic FLOPs (2*M*N*K, un-padded K) and the launch
 * count since milan_profile_enable(1).  Process-wide; not for production. */
int milan_profile_enable(int enable);
int milan_profile_read(double* gemm_ms, double* gemm_flops,
                       long long* gemm_launches);

/* Per-stage breakdown of the same measurement (north_star: "fraction of
 * HBM/MFMA roofline reported per stage").  While profiling is enabled every
 * stage region of the hot path is also bracketed by two HIP events and every
 * GEMM record carries the stage it ran in.  `table` receives
 * MILAN_STAGE_COUNT rows of 6 doubles: region ms (sum over calls), region
 * count, GEMM ms inside the stage, GEMM algorithmic FLOPs, GEMM launches, GEMM
 * algorithmic HBM bytes (every operand of a launch crossing HBM once: visited
 * input pixels, weights, residual, output -- what bounds the small-K layers). */
enum milan_stage {
  MILAN_STAGE_OTHER = 0,
  MILAN_STAGE_ENC_INPUT = 1,     /* mask pyramid lists + u8 -> normalised input
                                    (datasets.py:191-197, encoders.py:295)   */
  MILAN_STAGE_ENC_STEM = 2,      /* conv1 7x7/2                               */
  MILAN_STAGE_ENC_STEM_TAIL = 3, /* bn1 + relu + maxpool 3x3/2                */
  MILAN_STAGE_ENC_LAYER1 = 4,    /* torchvision layer1..layer4 (convs only)   */
  MILAN_STAGE_ENC_LAYER2 = 5,
  MILAN_STAGE_ENC_LAYER3 = 6,
  MILAN_STAGE_ENC_LAYER4 = 7,
  MILAN_STAGE_ENC_POOL = 8,      /* mask-weighted pooling of the five taps
                                    (encoders.py:303-320)                    */
  MILAN_STAGE_DEC_INIT = 9,      /* hoisted key projection + init_state       */
  MILAN_STAGE_DEC_SEARCH = 10,   /* the T-step greedy / beam loop             */
  MILAN_STAGE_DEC_LM = 11,       /* LM scoring of the beams + rerank select   */
  MILAN_STAGE_COUNT = 12
};
int milan_profile_read_stages(double* table /* [MILAN_STAGE_COUNT][6] */);

/* The same records by kernel family: `table` receives MILAN_KERNEL_COUNT rows of 4
 * doubles -- summed launch time (ms), algorithmic FLOPs, launches, algorithmic HBM bytes --
 * so that bench.py's `roofline` can price the DOMINANT kernel on its own launches. */
enum milan_kernel_family {
  MILAN_KERNEL_OTHER = 0,
  MILAN_KERNEL_PP32_256 = 1,    /* igemm_split16_pp32_kernel (256 x 256 ping-pong tile)  */
  MILAN_KERNEL_PP32_128 = 2,    /* igemm_split16_pp32n_kernel<128>                       */
  MILAN_KERNEL_SPLIT_OTHER = 3, /* the other split-f16 implicit-GEMM tiles               */
  MILAN_KERNEL_F32 = 4,         /* igemm_kernel, v_mfma_f32_32x32x2_f32                  */
  MILAN_KERNEL_CHAIN = 5,       /* chain_kernel (layer1 / layer2 expand -> reduce)       */
  MILAN_KERNEL_CHAIN_WIDE = 6,  /* layer3 expand -> reduce chain                         */
  MILAN_KERNEL_STEM = 7,        /* stem_fused_kernel                                     */
  MILAN_KERNEL_CONV3 = 8,       /* conv3_p64_kernel                                      */
  MILAN_KERNEL_F16 = 9,         /* igemm_f16_pp32_kernel (fast mode)                     */
  MILAN_KERNEL_PP32T_256 = 10,  /* igemm_split16_pp32t_kernel<256>: the same tile function as
                                   PP32_256 on k x k convs in (slice, tap, channel) order  */
  MILAN_KERNEL_BNECK = 11,      /* chain_kernel<.., CONV>: layer1's 3x3 + expand + reduce  */
  MILAN_KERNEL_COUNT = 12
};
int milan_profile_read_kernels(double* table /* [MILAN_KERNEL_COUNT][4] */);

/* ---- exemplar computation ---------------------------
 * The stage that WRITES the images.npy / masks.npy this path reads
 * (src/exemplars/compute.py:27-246).  The dissected model stays the caller's
 * (the reference takes it as two black-box functions, compute.py:27-29);
 * these entry points are the tensor operations of its netdissect
 * dependencies on the activation tensor `hiddens` (batch, channels, h, w)
 * fp32 NCHW, hw = h * w.  `units` (device int32 [n_units], or NULL = all
 * channels) is the `units=` subset of compute.py:186-199.  The control flow of
 * the quantile sketch (which level is compacted when, with which random bit)
 * is host logic, as it is Python in the reference (milan_amd/exemplars.py). */

/* RunningTopK.add + result (src/deps/netdissect/runningstats.py:58-116) on the
 * spatial max of compute.py:331: merges this batch into top_values/top_index
 * [n_units][k], of which `filled` columns are valid; afterwards
 * min(k, filled + batch) are, sorted by value descending (equal values: lower
 * dataset index first).  Image b of the batch has dataset index
 * first_index + b.  pooled_scratch: n_units * batch floats.
 * filled + batch <= 2048. */
int milan_exemplar_topk_update(const float* hiddens, int batch, int channels,
                               int hw, const int32_t* units, int n_units,
                               int64_t first_index, int k, int filled,
                               float* pooled_scratch, float* top_values,
                               int64_t* top_index, milan_stream stream);

/* RunningQuantile._add_every's copy (runningstats.py:363-385): activation rows
 * [first, first + count) of hiddens.permute(0,2,3,1).reshape(-1, C) go,
 * transposed, into level0[n_units][capacity] at columns column.. */
int milan_exemplar_sketch_append(const float* hiddens, int batch, int channels,
                                 int hw, const int32_t* units, int n_units,
                                 int64_t first, int64_t count, float* level0,
                                 int64_t capacity, int64_t column,
                                 milan_stream stream);

/* One compaction of RunningQuantile._shift / _expand (runningstats.py:387-407,
 * 485-521): every row's first n columns of src are sorted ascending, every
 * second element starting at `offset` (the random bit) is written to dst at
 * columns position.., and -- when `extremes` [n_units][2] is given -- the
 * row's minimum / maximum are folded into it (:415-419).  dst may equal src
 * (the in-place "scrunch") with position 0.  Workspace:
 * milan_exemplar_sort_workspace(n_units, n, 0). */
size_t milan_exemplar_sort_workspace(int n_units, int64_t n, int pairs);
int milan_exemplar_sketch_compact(const float* src, int64_t src_capacity,
                                  int64_t n, int n_units, int offset, float* dst,
                                  int64_t dst_capacity, int64_t position,
                                  float* extremes, void* workspace,
                                  size_t workspace_bytes, milan_stream stream);

/* RunningQuantile._add_every for a whole batch (runningstats.py:363-407): the
 * sketch's control flow depends on buffer sizes only, so it is played forward on
 * the host and executed level by level -- one launch per level, every compaction
 * of a level in parallel -- instead of one append + one compaction launch per
 * 128..8192 samples.  Consumes activation rows [first, batch*hw) of `hiddens`
 * (row order as milan_exemplar_sketch_append).  levels / firstfree / capacities:
 * HOST arrays of n_levels entries (device row pointers; fill counts, updated on
 * return; row capacities, each in [2, 8192]).  randbits: HOST array of the
 * caller's random bits (torch's, so that seeded runs match the reference),
 * *currentbit the index of the last one used, updated on return.  Stops early --
 * *consumed < batch*hw - first, level 0 full -- before a _shift() that needs
 * _expand() or more random bits than remain: the caller performs that one
 * _shift() (milan_exemplar_sketch_compact) and calls again.  Same results as
 * the per-operation path, bit for bit. */
size_t milan_exemplar_sketch_add_workspace(int n_units, int64_t supplied,
                                           const int64_t* capacities,
                                           int n_levels);
int milan_exemplar_sketch_add(const float* hiddens, int batch, int channels, int hw,
                              const int32_t* units, int n_units, int64_t first,
                              int64_t* consumed, float* const* levels,
                              int64_t* firstfree, const int64_t* capacities,
                              int n_levels, const uint8_t* randbits,
                              int64_t n_randbits, int64_t* currentbit,
                              float* extremes, void* workspace,
                              size_t workspace_bytes, milan_stream stream);

/* RunningQuantile._scan_extremes (runningstats.py:409-419), used by the sketch's
 * subsampling regime where not every sample enters a buffer: column-wise minimum /
 * maximum of `rows` [n_rows][n_units] (row-major, device) folded into `extremes`
 * [n_units][2] = (min, max). */
int milan_exemplar_rows_extremes(const float* rows, int64_t n_rows, int n_units,
                                 float* extremes, milan_stream stream);

/* What RunningQuantile does when level 0 is full and the bulk call above stopped: one
 * _shift() (runningstats.py:387-407) INCLUDING the _expand() it may end in
 * (:485-529), as a plan -- host arithmetic only, no device work.  The caller executes
 * the operations in order (on its own tensors) and adopts the returned fill counts:
 *   MILAN_SKETCH_COMPACT  sort level `src`'s first n columns, keep every second one
 *                         from `offset`, write them to level `dst` at `position`
 *                         (milan_exemplar_sketch_compact; `extremes` != 0: fold min /
 *                         max into the extremes);
 *   MILAN_SKETCH_INSERT   a new, empty level 0 of `capacity` columns (every later
 *                         level index in the plan counts it);
 *   MILAN_SKETCH_MOVE     level `src`'s first n columns -> level `dst` at `position`;
 *   MILAN_SKETCH_HALVE    the sample rate halves (no room for another level).
 * Level indices are those at the moment the operation runs.  `draw_bit(user)` hands
 * out the caller's random bits in the order upstream consumes them (torch's global
 * generator, so that a seeded run reproduces the reference).  capacities_out /
 * firstfree_out need room for n_levels + 1 entries. */
enum { MILAN_SKETCH_COMPACT = 0, MILAN_SKETCH_INSERT = 1, MILAN_SKETCH_MOVE = 2,
       MILAN_SKETCH_HALVE = 3 };
typedef struct milan_sketch_op {
  int32_t kind, src, dst, offset, extremes, reserved;
  int64_t n, position, capacity;
} milan_sketch_op;
int milan_exemplar_sketch_plan_shift(int64_t resolution, int64_t buffersize,
                                     int full_rate, int n_levels,
                                     const int64_t* capacities,
                                     const int64_t* firstfree,
                                     int (*draw_bit)(void*), void* user,
                                     milan_sketch_op* ops, int max_ops, int* n_ops,
                                     int64_t* capacities_out, int64_t* firstfree_out,
                                     int* n_levels_out);

/* RunningQuantile.quantiles(q) for one q (runningstats.py:531-580): weighted
 * summary of all levels (level l has weight 2^l), stable sort, float32
 * cumulative weights, numpy.interp in float64 -> out [n_units] float32.
 * levels / firstfree / capacities are HOST arrays of n_levels entries (device
 * row pointers, fill counts, row capacities); extremes [n_units][2] is updated
 * with the level-0 remainder like the reference does.  Exact parity needs the
 * total weight (= samples seen) below 2^24 per unit (float32 sums, as in the
 * reference).  Workspace: milan_exemplar_sort_workspace(n_units, sum of
 * firstfree, 1). */
int milan_exemplar_sketch_quantile(const float* const* levels,
                                   const int64_t* firstfree,
                                   const int64_t* capacities, int n_levels,
                                   int n_units, float* extremes, float q,
                                   float* out, void* workspace,
                                   size_t workspace_bytes, milan_stream stream);

/* ImageVisualizer cells (src/deps/ext/netdissect/imgviz.py:56-81): for each of
 * the n_cells rows (batch item, activation channel, unit slot, rank) of `cells`
 * (device int32 [n_cells][4]):
 *   mask   = grid_sample(act, upsample_grid, bilinear, align_corners) > level
 *            (imgviz.py:185-198, upsample.py:6-45,132-156)        -> out_masks
 *   image  = nearest resize of (image * mul + add).clamp(0,255).byte()
 *            (imgviz.py:200-210, renormalize.py:119-136)          -> out_images
 *   masked = image inside the mask, 0.25 * image outside          -> out_masked
 * written at [slot][rank] of the (slots, k, 3|1, out, out) uint8 outputs.
 * images (batch, 3, img_h, img_w) fp32; levels [slots] fp32 (device);
 * mul3 / add3 host float[3]. */
int milan_exemplar_render(const float* hiddens, int batch, int channels, int h,
                          int w, const float* images, int img_h, int img_w,
                          const int32_t* cells, int n_cells, const float* levels,
                          const float* mul3, const float* add3, int out_size,
                          int k, uint8_t* out_images, uint8_t* out_masks,
                          uint8_t* out_masked, milan_stream stream);

/* Building block exposed for kernel-level parity tests: one NHWC fp32
 * convolution through the same implicit-GEMM MFMA kernel the trunk uses
 * (counterpart of torch.nn.functional.conv2d as torchvision's ResNet calls it).
 * x (n,h,w,cin) NHWC with cin % 4 == 0; weight (cout,cin,kh,kw) OIHW as in the
 * reference state dict; bias (cout) or NULL; residual (n,ho,wo,cout) or NULL
 * (residual implies relu(conv + bias + residual)); y (n,ho,wo,cout).
 * precision: MILAN_PRECISION_* (split mode converts x and the weights first).
 * Allocates temporaries and synchronises: not for the hot path. */
int milan_conv2d_nhwc(const float* x, int n, int h, int w, int cin,
                      const float* weight_oihw, const float* bias, int cout,
                      int kh, int kw, int stride, int pad, int relu,
                      const float* residual, float* y, int precision,
                      milan_stream stream);

/* Building block exposed for kernel-level tests: ONE launch of the implicit GEMM with every
 * argument of its launcher in the caller's hand (milan_conv2d_nhwc reaches fp32 output, dense
 * rows and three epilogues only).  The caller owns the device buffers A, A2, aux and C -- in
 * the format the flags announce: split format [hi x8 | lo x8] per 8 channels where a_split /
 * aux_split / out_split say so, fp32 otherwise -- with their strides, so an operand may sit in
 * a channel slice of a wider row; and the int32 word m_live, the int32 row_list and the uint32
 * status word (set as a context's is for the launch; NULL = nobody listens).
 * The entry point owns the weights: `weight` is fp32 [groups][N][K] in the GEMM's k order
 * ((tap, channel) of A, then the channels of A2), from which it makes what a trunk makes with
 * the library's own packers: rows padded to Kp = round_up(K, 32), the groups' rows back to back
 * (that is the weights' group stride), with a_split their split copy at a power-of-two scale
 * undone by the accumulator scale, and for a k x k conv of whole 32-channel slices the
 * (slice, tap, channel) copy unless no_wt is set.  bias: fp32 [groups][N] or NULL.
 * Every other field is the launcher's argument of the same name; K1 = 0 without A2;
 * tap_ncls = -1 keeps a tap-inner launch on the linear tile order; groups <= 1 = none.
 * Nothing is decided here: the plan of the launch (which kernel, which refusal) is the
 * library's.  f16 != 0 and the LSTM / log-sum-exp epilogues (epilogue > 5) are MILAN_ERR_ARG.
 * Allocates temporaries and synchronises: not for the hot path. */
typedef struct milan_gemm_probe_args {
  const void* A;
  const void* A2;
  const void* aux;
  void* C;
  const float* weight;
  const float* bias;
  const int32_t* m_live;
  const int32_t* row_list;
  uint32_t* status;
  int64_t a_pix_stride, a_img_stride, a2_pix_stride, a2_img_stride;
  int64_t a_grp, bias_grp, c_grp, aux_grp;
  int32_t M, N, K, ldc, ldaux;
  int32_t H, Wd, Cin, Ho, Wo, KH, KW, stride, pad;
  int32_t aniso, stride_w, pad_w;
  int32_t epilogue, a_split, out_split, aux_split, f16;
  int32_t K1, H2, W2d, stride2;
  int32_t m_live_mul, groups, tap_ncls, no_wt;
} milan_gemm_probe_args;
int milan_gemm_probe(const milan_gemm_probe_args* args, milan_stream stream);

/* ---- LanguageModel training (src/milan/lms.py:134-265) --------------------
 * Loss, forward and backward of Embedding -> nn.LSTM(dropout) -> Linear ->
 * LogSoftmax -> NLLLoss(ignore_index = pad_index) over a padded batch.
 *   params / grads: HOST arrays of n_params DEVICE fp32 pointers in
 *     LanguageModel.state_dict() order: embedding.weight, then per layer
 *     lstm.weight_ih_l, weight_hh_l, bias_ih_l, bias_hh_l, then output.0.weight,
 *     output.0.bias (n_params = 3 + 4 * lm_layers), raw torch layout.  They are
 *     read on every call: the ctx only supplies the LM dims (vocab_size,
 *     pad_index, lm_*) and need not be finalized; its weight arena is not used.
 *   inputs / targets: (rows, L) int64 (the reference's lossify: inputs with
 *     <start>, targets with <stop>, both padded).  Ids must lie in
 *     [0, vocab_size): the caller validates (out-of-range ids are clamped, not
 *     reported).  Targets equal to pad_index do not count.
 *   loss_sum_and_count: DEVICE float[2] <- sum of -log p(target) over the
 *     valid targets and their number; the mean loss is [0] / [1] (NaN when
 *     [1] == 0, as in torch).
 *   milan_lm_nll        eval mode (no dropout): the loss only.
 *   milan_lm_train_step train mode: dropout p on the output of every layer but
 *     the last, mask a pure function of (seed, layer, row, t, unit):
 *     keep <=> (mix64(seed ^ mix64(layer<<56 | row<<32 | t<<16 | unit)) >> 40)
 *     >= (uint32)(p * 2^24), kept values scaled by 1 / (1 - p), mix64 = the
 *     splitmix64 finaliser.  Then the gradient of the MEAN loss with respect to
 *     every parameter is written to `grads`: OVERWRITTEN, not accumulated.
 *     The embedding row of pad_index gets exactly zero.
 * Precision: exact fp32 MFMA whatever milan_set_precision says (split-f16 is an
 * inference mode).  Deterministic: no float atomics, fixed reduction orders;
 * equal inputs and seed give equal bits.  Neither call synchronises.
 * rows < 2^24, L < 2^16, 1 <= lm_layers <= 8. */
size_t milan_lm_train_workspace_bytes(const milan_ctx* ctx, int rows, int L);
int milan_lm_nll(milan_ctx* ctx, const float* const* params, int n_params,
                 const int64_t* inputs, const int64_t* targets, int rows, int L,
                 float* loss_sum_and_count, void* workspace,
                 size_t workspace_bytes, milan_stream stream);
int milan_lm_train_step(milan_ctx* ctx, const float* const* params,
                        float* const* grads, int n_params,
                        const int64_t* inputs, const int64_t* targets, int rows,
                        int L, float dropout, uint64_t seed,
                        float* loss_sum_and_count, void* workspace,
                        size_t workspace_bytes, milan_stream stream);

/* Forward and backward for autograd (LanguageModel.forward in training mode with
 * trainable parameters): the forward of milan_lm_train_step with its log-probs
 * returned instead of a loss, and a backward driven by arbitrary upstream
 * gradients.  Parameter list, ctx, dims, dropout mask, precision and
 * determinism as above; neither call synchronises.
 *
 * MILAN_ABI_VERSION did not change with these entry points: probe for them
 * (dlsym / hasattr(lib, "milan_lm_forward_train")).
 *   milan_lm_grad_workspace_bytes: the workspace both calls need (the
 *     train-step workspace plus the forward's unused loss terms); 0 on bad dims.
 *   milan_lm_forward_train: logprobs_out (rows, L, vocab) fp32 DEVICE <-
 *     log_softmax of every position (NULL: not written); picked_out (rows, L)
 *     fp32 DEVICE <- logprobs[r, t, targets[r, t]] (NULL: not written).
 *     targets: (rows, L) int64 DEVICE, given if and only if picked_out is; ids
 *     in [0, vocab_size), the caller validates (clamped, not reported).  With
 *     picked_out alone the (rows, L, vocab) log-probs are never written.  Pad
 *     ids are ordinary inputs (their embedding row is whatever the parameter
 *     holds) and ordinary targets.  The workspace keeps the activations for one
 *     milan_lm_backward.
 *   milan_lm_backward: consumes a workspace filled by milan_lm_forward_train
 *     with the same params, inputs, dims, dropout and seed.  dlogprobs (rows, L,
 *     vocab) and dpicked (rows, L) fp32 DEVICE are the upstream gradients (NULL:
 *     zero; both NULL: MILAN_ERR_ARG); targets as in the forward, required with
 *     dpicked.  Per position g_v = dlogprobs[v] + (v == target ? dpicked : 0)
 *     and dlogit_v = g_v - exp(logit_v - lse) * sum_v g_v, the row sum in a
 *     fixed order.  `grads` are OVERWRITTEN with the gradient of
 *     sum(dlogprobs * logprobs) + sum(dpicked * picked) with respect to every
 *     parameter; the embedding row of pad_index gets exactly zero.  The backward
 *     overwrites activations in place: one forward supports exactly one
 *     backward. */
size_t milan_lm_grad_workspace_bytes(const milan_ctx* ctx, int rows, int L);
int milan_lm_forward_train(milan_ctx* ctx, const float* const* params,
                           int n_params, const int64_t* inputs, int rows, int L,
                           float dropout, uint64_t seed, float* logprobs_out,
                           float* picked_out, const int64_t* targets,
                           void* workspace, size_t workspace_bytes,
                           milan_stream stream);
int milan_lm_backward(milan_ctx* ctx, const float* const* params,
                      float* const* grads, int n_params, const int64_t* inputs,
                      int rows, int L, float dropout, uint64_t seed,
                      const float* dlogprobs, const float* dpicked,
                      const int64_t* targets, void* workspace,
                      size_t workspace_bytes, milan_stream stream);

/* ---- Decoder training (src/milan/decoders.py:873-1070) -----------------------
 * Loss, forward and backward of the teacher-forced attention LSTM,
 * Decoder.forward(features, strategy=targets, mi=False) in training mode, with
 * NLLLoss(ignore_index = pad_index) and the double-stochasticity regulariser.
 *   params / grads: HOST arrays of 19 DEVICE fp32 pointers, the decoder's own
 *     state dict in the reference's order: init_h.0.weight, init_h.0.bias,
 *     init_c.0.weight, init_c.0.bias, embedding.weight,
 *     attend.query_to_hidden.weight, .bias, attend.key_to_hidden.weight, .bias,
 *     attend.output.0.weight, .bias, feature_gate.0.weight, .bias,
 *     lstm.weight_ih, lstm.weight_hh, lstm.bias_ih, lstm.bias_hh,
 *     output.1.weight, output.1.bias; raw torch layout.  They are read on every
 *     call: the ctx only supplies the decoder dims (feature, hidden, embedding,
 *     attention and vocab sizes, start_index, pad_index) and need not be
 *     finalized; its weight arena is not used.
 *   features: (rows, k, feature_size) fp32 DEVICE, the frozen encoder's output
 *     (no gradient flows into it here; milan_decoder_backward below computes
 *     one).
 *   targets: (rows, L) int64 DEVICE, the indexed captions without <start>
 *     (with <stop>, padded).  The input of step 0 is <start>, of step t
 *     targets[:, t-1].  Ids must lie in [0, vocab_size): the caller validates
 *     (out-of-range ids are clamped, not reported).  Targets equal to pad_index
 *     do not count in the NLL.
 *   loss_terms: DEVICE float[3] <- the sum of -log p(target) over the valid
 *     targets, their number, and sum over (row, feature) of
 *     (1 - sum_t alpha_t)^2 over all L steps (pad steps included).  The mean
 *     NLL is [0] / [1] (NaN when [1] == 0, as in torch); the training loss is
 *     [0] / [1] + regularization_weight * [2] / (rows * k).
 *   milan_decoder_nll        eval mode (no dropout).  The reference's validation
 *     loss is the NLL alone, [0] / [1].
 *   milan_decoder_train_step train mode: dropout p on h before the output
 *     Linear, mask a pure function of (seed, row, t, unit):
 *     keep <=> (mix64(seed ^ mix64(0xDC<<56 | row<<32 | t<<16 | unit)) >> 40)
 *     >= (uint32)(p * 2^24), kept values scaled by 1 / (1 - p), mix64 = the
 *     splitmix64 finaliser (the LM's hash with its own tag 0xDC in place of the
 *     layer).  Then the gradient of the training loss with respect to every
 *     parameter is written to `grads`: OVERWRITTEN, not accumulated.  The
 *     embedding has no padding row: pad inputs get their gradient too.
 * Precision: exact fp32 MFMA whatever milan_set_precision says.  Deterministic:
 * no float atomics, fixed reduction orders; equal inputs and seed give equal
 * bits.  Neither call synchronises.
 * 0 < rows < 2^24, 0 < L < 2^16, 0 < k <= 64, rows * L * k < 2^30,
 * hidden_size < 2^14. */
size_t milan_decoder_train_workspace_bytes(const milan_ctx* ctx, int rows,
                                           int k, int L);
int milan_decoder_nll(milan_ctx* ctx, const float* const* params, int n_params,
                      const float* features, const int64_t* targets, int rows,
                      int k, int L, float* loss_terms, void* workspace,
                      size_t workspace_bytes, milan_stream stream);
int milan_decoder_train_step(milan_ctx* ctx, const float* const* params,
                             float* const* grads, int n_params,
                             const float* features, const int64_t* targets,
                             int rows, int k, int L, float dropout,
                             uint64_t seed, float regularization_weight,
                             float* loss_terms, void* workspace,
                             size_t workspace_bytes, milan_stream stream);

/* Teacher-forced forward and backward for autograd (Decoder.forward in training
 * mode with a tensor strategy): the forward of milan_decoder_train_step with its
 * outputs returned instead of a loss, and a backward driven by arbitrary
 * upstream gradients.  Parameter list, ctx, dims, dropout mask, precision and
 * determinism as above; neither call synchronises.
 *   milan_decoder_grad_workspace_bytes: the workspace both calls need (the
 *     train-step workspace plus dctx, the pooled-feature gradient and the
 *     feature-gradient GEMM scratch); 0 on bad dims.
 *   milan_decoder_forward_train: logprobs_out (rows, L, vocab) fp32 DEVICE <-
 *     log_softmax of every position; attentions_out (rows, L, k) fp32 DEVICE
 *     <- the attention weights.  Pad targets are ordinary inputs (no loss).
 *     The workspace keeps the activations for one milan_decoder_backward.
 *   milan_decoder_backward: consumes a workspace filled by
 *     milan_decoder_forward_train with the same params, features, targets,
 *     dims, dropout and seed.  dlogprobs (rows, L, vocab) and dattentions
 *     (rows, L, k) fp32 DEVICE are the upstream gradients (NULL: zero).
 *     `grads` are OVERWRITTEN with the gradient of sum(dlogprobs * logprobs)
 *     + sum(dattentions * attentions) with respect to the 19 parameters;
 *     dfeatures (rows, k, feature_size) fp32 DEVICE <- its gradient with
 *     respect to the features (NULL: not computed), summed in the fixed order
 *     (keys + context over increasing t) + mean pool.  The backward overwrites
 *     activations in place: one forward supports exactly one backward. */
size_t milan_decoder_grad_workspace_bytes(const milan_ctx* ctx, int rows, int k,
                                          int L);
int milan_decoder_forward_train(milan_ctx* ctx, const float* const* params,
                                int n_params, const float* features,
                                const int64_t* targets, int rows, int k, int L,
                                float dropout, uint64_t seed,
                                float* logprobs_out, float* attentions_out,
                                void* workspace, size_t workspace_bytes,
                                milan_stream stream);
int milan_decoder_backward(milan_ctx* ctx, const float* const* params,
                           float* const* grads, int n_params,
                           const float* features, const int64_t* targets,
                           int rows, int k, int L, float dropout, uint64_t seed,
                           const float* dlogprobs, const float* dattentions,
                           float* dfeatures, void* workspace,
                           size_t workspace_bytes, milan_stream stream);

/* ---- CLIP reranker (src/milan/rerankers.py, DecoderWithCLIP) ------------------
 * A context of its own: the dims of a ViT CLIP and one arena holding its weights
 * in the state-dict layout of OpenAI's `clip` (visual.conv1.weight, ...,
 * transformer.resblocks.N.*, text_projection), row-major fp32 as torch stores
 * them.  milan_clip_set_weight records caller-owned DEVICE pointers by name;
 * milan_clip_finalize_weights checks that every tensor the dims need is there
 * with the right element count, copies them into the arena and synchronises
 * (the only call here that does).  Unknown names are ignored.
 *
 * Precision: exact fp32 MFMA, whatever any milan_ctx's precision is.
 * Deterministic: fixed reduction orders, no float atomics.
 * Attention runs one workgroup per (sequence, head) with Q, K, V of the head in
 * LDS: 4 * (3 * tokens * (head + 1) + 4 * tokens) bytes must fit 64 KiB, for
 * tokens = (resolution / patch)^2 + 1 and tokens = context_length;
 * milan_clip_create refuses other dims with MILAN_ERR_SHAPE and says so. */
typedef struct milan_clip_ctx milan_clip_ctx;
typedef struct milan_clip_dims {
  int32_t resolution;     /* input pixels per side (224)          */
  int32_t patch;          /* conv1 kernel = stride (32)           */
  int32_t vision_width;   /* 768 */
  int32_t vision_layers;  /* 12; at most 64 can be mask layers    */
  int32_t vision_heads;   /* 12  */
  int32_t embed_dim;      /* 512 */
  int32_t context_length; /* 77  */
  int32_t vocab_size;     /* 49408 */
  int32_t text_width;     /* 512 */
  int32_t text_layers;    /* 12  */
  int32_t text_heads;     /* 8   */
} milan_clip_dims;

int milan_clip_create(milan_clip_ctx** out, int device,
                      const milan_clip_dims* dims);
void milan_clip_destroy(milan_clip_ctx* ctx);
int milan_clip_set_weight(milan_clip_ctx* ctx, const char* name,
                          const float* data, const int64_t* shape, int ndim);
int milan_clip_finalize_weights(milan_clip_ctx* ctx, milan_stream stream);

/* Image embeddings (CLIPWithMasks.forward, image side).
 *   images: (n, 3, resolution, resolution) fp32 DEVICE.  `resolution` must be the
 *     model's (MILAN_ERR_SHAPE otherwise: the reference's default path fails
 *     there too, it never uses its resized tensor).
 *   renorm_mul_add: HOST float[6] = mul[3], add[3]: every pixel of channel c
 *     becomes x * mul[c] + add[c] before the patch embedding (the reference's
 *     Renormalizer); NULL: no renormalisation.
 *   masks: (n, 1, resolution, resolution) fp32 DEVICE or NULL.  They are resized
 *     to the patch grid (bilinear, align_corners = false, no antialiasing); in
 *     every layer l with bit l of mask_layers set, after the softmax, the CLS
 *     query's weights on the patch keys are multiplied by them, the same for
 *     every head; the row is not renormalised.
 *   both = 0: out (n, embed_dim) <- L2-normalised embeddings, masked if masks.
 *   both = 1 (needs masks): out (2, n, embed_dim) <- [0] masked, [1] unmasked;
 *     the 2 n sequences go through every layer as one batch.
 * Does not synchronise. */
size_t milan_clip_image_workspace_bytes(const milan_clip_ctx* ctx, int n,
                                        int both);
int milan_clip_encode_images(milan_clip_ctx* ctx, const float* images, int n,
                             int resolution, const float* masks,
                             uint64_t mask_layers, int both,
                             const float* renorm_mul_add, float* out,
                             void* workspace, size_t workspace_bytes,
                             milan_stream stream);

/* Text embeddings (encode_text + L2 normalisation).
 *   tokens: (rows, context_length) int64 DEVICE.  The embedding of a row is read
 *     at the first position of its largest id (the end-of-text token).
 *   positions: the tower runs over the first `positions` <= context_length
 *     positions only.  It is causal, so any positions > every row's
 *     end-of-text position gives what context_length gives, up to the rounding
 *     of GEMM tiles; the caller passes max(eot) + 1.  (A row whose end-of-text
 *     lies beyond is read at positions - 1.)
 *   out: (rows, embed_dim) fp32 DEVICE.  Does not synchronise. */
size_t milan_clip_text_workspace_bytes(const milan_clip_ctx* ctx, int rows,
                                       int positions);
int milan_clip_encode_texts(milan_clip_ctx* ctx, const int64_t* tokens,
                            int rows, int positions, float* out,
                            void* workspace, size_t workspace_bytes,
                            milan_stream stream);

/* Rerank scores (CLIPWithMasksReranker.forward before the sort):
 *   out[c] = (1 - lam) * sum_i <masked[n][i], texts[c]>
 *            +     lam * sum_i <unmasked[n][i], texts[c]>,   i < k in order,
 * for text row c of neuron n = neuron_of[c] (int32 DEVICE, `rows` entries), or
 * n = c / candidates when neuron_of is NULL.  masked / unmasked: (neurons, k,
 * embed) fp32 DEVICE, texts (rows, embed), out (rows).  Does not synchronise. */
int milan_clip_rerank_scores(const float* masked, const float* unmasked,
                             const float* texts, const int32_t* neuron_of,
                             int neurons, int k, int rows, int candidates,
                             int embed, float lam, float* out,
                             milan_stream stream);

/* ---- BERTScore (src/utils/metrics.py:94-150, Decoder.bert_score) ----------------
 * A context of its own: the dims of a BERT-family (post-LN) encoder and one arena
 * holding its weights under their HuggingFace state-dict names without the
 * model prefix (embeddings.word_embeddings.weight, ...,
 * encoder.layer.N.attention.self.query.weight, ...), row-major fp32 as torch
 * stores them, nothing packed.  set_weight / finalize_weights behave as their
 * milan_clip_* namesakes; only layers 0 .. layers - 1 are asked for.  No pooler.
 *
 * MILAN_ABI_VERSION did not change with these entry points: probe for them
 * (dlsym / hasattr(lib, "milan_bert_create")).
 *
 * Precision: exact fp32 MFMA.  Deterministic: fixed reduction orders, no float
 * atomics, and the GEMMs' split count depends on K alone, so the embeddings of
 * a sentence do not depend on which other sentences share its call.
 * Attention runs one workgroup per (sentence, head) with Q, K, V of the head in
 * LDS: 4 * (3 * tokens * (head + 1) + 4 * tokens) bytes at tokens =
 * MILAN_BERT_MAX_TOKENS must fit 64 KiB (head size <= 83); milan_bert_create
 * refuses other dims with MILAN_ERR_SHAPE and names them. */
#define MILAN_BERT_MAX_TOKENS 64 /* longest supported sentence, specials included */
typedef struct milan_bert_ctx milan_bert_ctx;
typedef struct milan_bert_dims {
  int32_t vocab_size;      /* 50265 (roberta-large)                           */
  int32_t width;           /* 1024 */
  int32_t layers;          /* encoder layers TO RUN (17 of roberta-large's 24) */
  int32_t heads;           /* 16   */
  int32_t intermediate;    /* 4096 */
  int32_t max_positions;   /* rows of the position table (514)                */
  int32_t type_vocab;      /* rows of the token-type table; row 0 is used     */
  int32_t position_offset; /* position id of a sentence's first token:
                              pad_id + 1 for RoBERTa (2), 0 for BERT          */
  float eps;               /* layer_norm_eps (1e-5 RoBERTa, 1e-12 BERT)       */
} milan_bert_dims;

int milan_bert_create(milan_bert_ctx** out, int device,
                      const milan_bert_dims* dims);
void milan_bert_destroy(milan_bert_ctx* ctx);
int milan_bert_set_weight(milan_bert_ctx* ctx, const char* name,
                          const float* data, const int64_t* shape, int ndim);
int milan_bert_finalize_weights(milan_bert_ctx* ctx, milan_stream stream);

/* Token embeddings of n ragged sentences: the last hidden state of the cut model.
 *   ids: (total) int64 DEVICE, the sentences' token ids (specials included)
 *     one after the other; offsets: (n + 1) int32 DEVICE, ascending, offsets[0]
 *     = 0, offsets[n] = total: sentence s owns rows offsets[s] .. offsets[s + 1].
 *   max_len: the longest sentence, computed by the caller on the host.  More
 *     than MILAN_BERT_MAX_TOKENS, or than max_positions - position_offset, is
 *     MILAN_ERR_SHAPE.  (The kernels clamp a length beyond max_len for memory
 *     safety only.)
 *   Position ids are position_offset + index in the sentence; token type 0.
 *   Every GEMM runs over the `total` real rows; there is no padding.
 *   normalize = 1: every row is divided by its L2 norm (what score_pairs takes).
 *   out: (total, width) fp32 DEVICE.  Does not synchronise. */
size_t milan_bert_encode_workspace_bytes(const milan_bert_ctx* ctx, int n,
                                         int total);
int milan_bert_encode(milan_bert_ctx* ctx, const int64_t* ids,
                      const int32_t* offsets, int n, int total, int max_len,
                      int normalize, float* out, void* workspace,
                      size_t workspace_bytes, milan_stream stream);

/* BERTScore's greedy matching for `pairs` (candidate, reference) pairs.
 *   emb: (rows, width) L2-normalised token embeddings of n_sent sentences,
 *     offsets (n_sent + 1) int32 as above (several encode calls may have filled
 *     the table); weights: (rows) idf weight of every token, not normalised;
 *     cand / ref: (pairs) int32 sentence numbers.  All DEVICE.
 *   Per pair: sim = C R^T (float64 accumulation), p_i = max_j sim_ij and r_j =
 *     max_i sim_ij over the other sentence's real tokens, weights normalised to
 *     sum 1 per sentence, P = sum_i w_i p_i, R = sum_j v_j r_j in token order,
 *     F = 2 P R / (P + R), NaN -> 0.  A sentence of at most 2 tokens ([cls, sep])
 *     gives P = R = F = 0.
 *   out: (pairs, 3) fp32 = P, R, F.  Does not synchronise. */
int milan_bert_score_pairs(const float* emb, const int32_t* offsets,
                           const float* weights, const int32_t* cand,
                           const int32_t* ref, int pairs, int n_sent, int width,
                           float* out, milan_stream stream);

/* ---- Streaming attention and the DINO ViT (milan_amd.vits) -------------------------
 * MILAN_ABI_VERSION did not change with these entry points: probe for them
 * (dlsym / hasattr(lib, "milan_vit_create")).
 *
 * milan_attention: softmax(q k^T / sqrt(head)) v per (sequence, head) for sequences
 * of any length.
 *   qkv: (seqs, tokens, 3 * width) fp32 DEVICE, 16-byte aligned: q | k | v, the
 *     heads contiguous inside each (torch's reshape(B, N, 3, heads, head)).
 *   out: (seqs, tokens, width) fp32 DEVICE.
 *   head = width / heads must be a multiple of 16 up to 128; anything else is
 *     MILAN_ERR_SHAPE and the message names it.  tokens >= 1.
 * The scores never reach memory: K and V stream through LDS 32 keys at a time
 * under an online softmax; both products are exact fp32 MFMA.  Needs no
 * workspace.  Deterministic, and the bits of one (sequence, head) do not depend
 * on the other sequences of the call.  Non-finite inputs are not specified.
 * Does not synchronise. */
int milan_attention(const float* qkv, float* out, int seqs, int tokens, int width,
                    int heads, milan_stream stream);

/* A pre-LN vision transformer as facebookresearch/dino builds it (cls token,
 * learned positions, no distillation token, no head), weights under their DINO
 * state-dict names (cls_token, pos_embed, patch_embed.proj.weight/bias,
 * blocks.N.norm1/attn.qkv/attn.proj/norm2/mlp.fc1/mlp.fc2 .weight/.bias,
 * norm.weight/bias), row-major fp32 as torch stores them.  create / set_weight /
 * finalize_weights / destroy behave as their milan_clip_* namesakes.
 * Exact fp32; every GEMM's split count depends on K alone, so the results for
 * an image do not depend on the other images of the call. */
typedef struct milan_vit_ctx milan_vit_ctx;
typedef struct milan_vit_dims {
  int32_t resolution; /* 224: input side, a multiple of patch            */
  int32_t patch;      /* 8                                                */
  int32_t width;      /* 384                                              */
  int32_t layers;     /* 12                                               */
  int32_t heads;      /* 6; width / heads a multiple of 16 up to 128      */
  int32_t hidden;     /* 1536: columns of mlp.fc1                         */
  float eps;          /* LayerNorm eps, 1e-6                              */
} milan_vit_dims;

int milan_vit_create(milan_vit_ctx** out, int device, const milan_vit_dims* dims);
void milan_vit_destroy(milan_vit_ctx* ctx);
int milan_vit_set_weight(milan_vit_ctx* ctx, const char* name, const float* data,
                         const int64_t* shape, int ndim);
int milan_vit_finalize_weights(milan_vit_ctx* ctx, milan_stream stream);

/* One walk over n images (n, 3, resolution, resolution) fp32 DEVICE.
 *   taps: HOST array of `layers` DEVICE pointers, or NULL.  A non-null taps[l]
 *     receives the output of blocks.l.mlp.fc1, (n, tokens, hidden) fp32, bias
 *     included, before the GELU; tokens = (resolution / patch)^2 + 1.
 *   cls_out: NULL, or (n, width) fp32 DEVICE: the CLS row after the final norm.
 *   Without cls_out the walk ends after fc1 of the deepest block asked for: no
 *   GELU or fc2 of that block and no later block runs.  With it every block runs.
 *   At least one output must be asked for.  Does not synchronise. */
size_t milan_vit_workspace_bytes(const milan_vit_ctx* ctx, int n);
int milan_vit_run(milan_vit_ctx* ctx, const float* images, int n, int resolution,
                  float* const* taps, float* cls_out, void* workspace,
                  size_t workspace_bytes, milan_stream stream);

/* ---- The attention block of a BigGAN generator ----------------------------------------
 * MILAN_ABI_VERSION did not change with this entry point: probe for it
 * (dlsym / hasattr(lib, "milan_sagan_attention")).
 *
 * milan_sagan_attention: the non-local block of SAGAN / BigGAN between its 1 x 1
 * convs, for n images of height x width pixels with `channels` channels, dk =
 * channels / 8, dv = channels / 2:
 *     out_i = sum_j softmax_j(theta_i . phi_j) g_j        (no scale factor)
 * over the height * width queries i and the height * width / 4 keys j of one image.
 * Pixel-major (NHWC) throughout, so the 1 x 1 convs around it are plain GEMMs:
 *   theta: fp32 DEVICE, 8-byte aligned; the dk query columns of pixel p of image b
 *     start at theta + (b * height * width + p) * theta_stride.  theta_stride is
 *     in floats, even and >= dk: dk for a dense (n, height * width, dk) tensor,
 *     dk + dk + dv for the first columns of a fused theta | phi | g conv output.
 *   phi_g: (n, height * width / 4, dk + dv) fp32 DEVICE, 16-byte aligned, dense:
 *     per 2 x 2 max-pooled pixel the dk key columns, then the dv value columns.
 *   out: (n, height * width, dv) fp32 DEVICE, 16-byte aligned, dense.
 *   channels must be a multiple of 32 from 32 to 384 (dk = 4 .. 48, dv = 16 ..
 *     192; BigGAN-128 / -256 have 192, BigGAN-512 has 384), height and width even
 *     (the pooling): anything else is MILAN_ERR_SHAPE and the message names the
 *     offending dimension.  n = 0 does nothing.
 * The scores never reach memory: a workgroup owns 128 queries of one image and
 * streams phi | g through LDS 32 keys at a time under an online softmax; both
 * products are exact fp32 MFMA.  Needs no workspace.  Deterministic, and the bits
 * of one image do not depend on the other images of the call.  Non-finite inputs
 * are not specified.  Does not synchronise. */
int milan_sagan_attention(const float* theta, int64_t theta_stride, const float* phi_g,
                          float* out, int n, int height, int width, int channels,
                          milan_stream stream);

/* A BigGAN generator as ajbrock/BigGAN-PyTorch and pretorched build it (shared class
 * embedding, class-conditional batch norm, optional hierarchical z, one SAGAN attention
 * block), eval mode, weights under their pretorched state-dict names (shared.weight,
 * linear.weight/bias, blocks.I.0.{conv1,conv2,conv_sc}.weight/bias,
 * blocks.I.0.{bn1,bn2}.{gain,bias}.weight and .stored_mean/.stored_var,
 * blocks.I.1.{theta,phi,g,o}.weight and .gamma, output_layer.0.gain/bias/stored_mean/
 * stored_var, output_layer.2.weight/bias), row-major fp32 as torch stores them.
 * Spectral norm is the caller's: upload weight / sv, the eval-mode weight (no u0 / sv0).
 * create / set_weight / finalize_weights / destroy behave as their milan_vit_*
 * namesakes; finalize_weights also packs the convolutions (theta | phi | g as one
 * 1 x 1 conv, gamma folded into o, the 3-channel output conv padded to 4 rows).
 * Exact fp32: every convolution runs on the implicit-GEMM MFMA tile chosen from the
 * layer alone, the batch norms are folded at run time to one scale and shift per
 * (sample, channel), the attention is milan_sagan_attention.  Deterministic; the
 * results for a sample do not depend on the other samples of the call.  The shortcut
 * of a block is conv_sc at the input side upsampled afterwards (a 1 x 1 conv commutes
 * with nearest upsampling), so sums are not formed in torch's order. */
typedef struct milan_gan_ctx milan_gan_ctx;
typedef struct milan_gan_dims {
  int32_t ch;              /* 96: channel multiplier, a multiple of 4                   */
  int32_t dim_z;           /* 120: columns of z (hierarchical: a multiple of blocks + 1) */
  int32_t shared_dim;      /* 128: columns of shared.weight                              */
  int32_t n_classes;       /* 1000                                                       */
  int32_t resolution;      /* 32, 64, 128, 256 or 512: selects the block table           */
  int32_t bottom_width;    /* 4: side of the first feature map                           */
  int32_t attn_resolution; /* 64: the block at this table resolution (8 << index) is
                              followed by attention; 0: none.  Its channel count must be
                              one milan_sagan_attention takes                            */
  int32_t hier;            /* 1: z is split into blocks + 1 chunks; chunk 0 feeds linear,
                              chunk i + 1 joins y as block i's condition                 */
  float bn_eps;            /* the conditional batch norms' eps (1e-4 in BigGAN-256)     */
  float out_bn_eps;        /* the output batch norm's eps (1e-5)                         */
} milan_gan_dims;

int milan_gan_create(milan_gan_ctx** out, int device, const milan_gan_dims* dims);
void milan_gan_destroy(milan_gan_ctx* ctx);
int milan_gan_set_weight(milan_gan_ctx* ctx, const char* name, const float* data,
                         const int64_t* shape, int ndim);
int milan_gan_finalize_weights(milan_gan_ctx* ctx, milan_stream stream);
/* number of taps: one per block plus one for the attention block, in walk order
 * (layer0, .., layerK, attnK, layerK+1, ..) */
int milan_gan_taps(const milan_gan_ctx* ctx);

/* One walk over n samples.
 *   z: (n, dim_z) fp32 DEVICE.
 *   classes: (n) int64 DEVICE class indices, or NULL; y: fp32 DEVICE or NULL: with
 *     y_embedded the embedded classes (n, shared_dim), otherwise soft labels (n,
 *     n_classes), which are multiplied by shared.weight.  Exactly one of classes and
 *     y is given.  An index outside 0 .. n_classes - 1 is clamped: check it before.
 *   taps: HOST array of milan_gan_taps() DEVICE pointers, or NULL.  A non-null
 *     taps[j] receives the output h of that block, (n, C, H, W) fp32 NCHW.
 *   images_out: NULL, or (n, 3, R, R) fp32 DEVICE, tanh included, with R =
 *     bottom_width << blocks (every block doubles the side): `resolution` selects the
 *     block table, and is R only at bottom_width 4.
 *   Without images_out the walk ends after the deepest tap asked for: no later block
 *   runs.  At least one output must be asked for.  Does not synchronise.
 *   n above 65535 (the launch grid's z) or n x the largest activation of a sample
 *   >= 2^31 floats is MILAN_ERR_ARG ("split the batch"); milan_gan_workspace_bytes
 *   then returns 0 with that message in milan_last_error, and nothing is launched. */
size_t milan_gan_workspace_bytes(const milan_gan_ctx* ctx, int n);
int milan_gan_run(milan_gan_ctx* ctx, const float* z, const int64_t* classes,
                  const float* y, int y_embedded, int n, float* const* taps,
                  float* images_out, void* workspace, size_t workspace_bytes,
                  milan_stream stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* MILAN_HIP_H */
