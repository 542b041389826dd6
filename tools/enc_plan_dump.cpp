// Prints the schedule of one ResNet encoder pass (csrc/enc_plan.h) -- host only, no GPU, no
// HIP call:
//
//   g++ -std=c++17 -O1 tools/enc_plan_dump.cpp -o enc_plan_dump
//   enc_plan_dump resnet18|34|50|101|152 width n H W f32|split|f16 [name=value ...]
//
// The trunk is torchvision's, with non-null 16-byte aligned sentinels where encoder_finalize
// would have made a weight copy.  Options (name=value, 0 / 1 unless said otherwise):
//   chain= wide= stem= conv3= skip_empty= bneck= sparse_tail= tail_lists=   the fusion bits (1)
//   images=u8|f32 (u8)   masks=none|u8|f32 (u8)   aligned=<images 4-byte aligned> (1)
//   share= calib= spatial= (0)   cus= experiments=
//   MILAN_STEM_U8= MILAN_POOL_VEC= MILAN_TAPS_INNER= and the launch path's MILAN_PP=,
//   MILAN_PP128=, MILAN_PP_PERSIST=, MILAN_TAP_INNER=, MILAN_TAP_SKIP=
// Output: one "pass" line of the pass-wide choices, one "block" line per block -- form, c1, c2,
// flags, sets, buffers, whether a launch of it writes a buffer it reads, and the kernel family
// of each of its launches in launch order -- and one "families" line: launches per family of
// hip.KERNEL_FAMILIES, in that order, with the launch_gemm calls and the row-list ones among
// them.  tests/test_enc_plan_host.py holds the parent driver's answers against it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../neuron-descriptions_amd/csrc/enc_plan.h"

using namespace milan;

static int usage(const char* why) {
  fprintf(stderr, "enc_plan_dump: %s\nusage: enc_plan_dump resnet18|34|50|101|152 width n H W "
                  "f32|split|f16 [name=value ...]\n", why);
  return 2;
}

// made-up, distinct, 16-byte aligned addresses: the plan looks at null-ness and alignment only
static float* sentinel() {
  static uintptr_t next = uintptr_t(1) << 40;
  next += 4096;
  return reinterpret_cast<float*>(next);
}

static void split_copies(ConvW& c, bool experiments) {
  c.ws = sentinel();
  c.bias_s = sentinel();
  if (c.cin % 64 == 0 && c.Kp % 64 == 0 && c.K == c.Kp) c.wf = sentinel();
  if (c.kh * c.kw > 1 && c.kh * c.kw <= 32 && c.Kp == c.K) {
    c.wst = sentinel();
    if (c.wf && c.cin % 64 == 0) c.wft = sentinel();
  }
  if (experiments && c.kh == 3 && c.kw == 3 && c.Kp == c.K && c.cin % 16 == 0) c.ws3 = sentinel();
}

// encoder.hip, pack_conv: a conv with its BatchNorm folded in (the stem's conv1: without)
static ConvW conv(int cout, int cin_real, int k, int stride, int pad, bool bn, bool experiments) {
  ConvW c;
  c.cout = cout; c.cin_real = cin_real; c.cin = (cin_real + 3) / 4 * 4;
  c.kh = c.kw = k; c.stride = stride; c.pad = pad;
  c.K = k * k * c.cin; c.Kp = (c.K + 31) / 32 * 32;
  c.w = sentinel();
  if (bn) c.bias = sentinel();
  if (bn && c.cin % 32 == 0) split_copies(c, experiments);
  return c;
}

// encoder.hip, fuse_c3_down
static void fuse(Bottleneck& b) {
  const ConvW &c3 = b.c3, &dn = b.down;
  if (c3.K != c3.Kp || dn.K != dn.Kp || c3.K % 32 || dn.K % 32 || c3.cout != dn.cout || !c3.ws || !dn.ws)
    return;
  ConvW f;
  f.cout = c3.cout; f.cin = c3.cin; f.cin_real = c3.cin_real;
  f.kh = f.kw = 1; f.stride = 1; f.pad = 0;
  f.K = f.Kp = c3.K + dn.K;
  f.w = sentinel(); f.bias = sentinel(); f.ws = sentinel(); f.bias_s = sentinel();
  if (f.cin % 64 == 0 && f.Kp % 64 == 0) f.wf = sentinel();
  b.c3d = f;
}

static const char* buf_name(const EncBuffers& pl, const float* p) {
  return p == nullptr ? "-" : p == pl.x0 ? "x0" : p == pl.x1 ? "x1" : p == pl.ds ? "ds"
         : p == pl.t1 ? "t1" : p == pl.t2 ? "t2" : p >= pl.raw && p < pl.x0 ? "raw" : "?";
}

int main(int argc, char** argv) {
  if (argc < 7) return usage("too few arguments");
  const std::string net = argv[1], prec = argv[6];
  const int wd = atoi(argv[2]);
  static const struct { const char* name; bool basic; int blocks[4]; } nets[] = {
      {"resnet18", true, {2, 2, 2, 2}},    {"resnet34", true, {3, 4, 6, 3}},
      {"resnet50", false, {3, 4, 6, 3}},   {"resnet101", false, {3, 4, 23, 3}},
      {"resnet152", false, {3, 8, 36, 3}}};
  int which = -1;
  for (int i = 0; i < 5; ++i) if (net == nets[i].name) which = i;
  if (which < 0) return usage("unknown trunk");
  if (prec != "f32" && prec != "split" && prec != "f16") return usage("unknown precision");
  if (wd < 4 || wd % 4) return usage("width must be a positive multiple of 4");

  EncAsk a;
  a.n = atoi(argv[3]); a.H = atoi(argv[4]); a.W = atoi(argv[5]);
  if (a.n < 1 || a.H < 1 || a.W < 1) return usage("n, H, W must be positive");
  a.trunk_kind = nets[which].basic ? MILAN_TRUNK_BASIC : MILAN_TRUNK_BOTTLENECK;
  a.width = wd; a.feature_size = (nets[which].basic ? 16 : 61) * wd;
  a.precision = prec == "f32" ? MILAN_PRECISION_F32 : MILAN_PRECISION_SPLIT_F16;
  a.trunk_f16 = prec == "f16";
  a.fusion = 255;
  a.image_dtype = MILAN_DTYPE_U8; a.masks = true; a.mask_dtype = MILAN_DTYPE_U8;
  a.images_aligned4 = true;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.stdv[c] = stdv[c]; }
  for (int i = 7; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return usage("options are name=value");
    const std::string name(argv[i], eq - argv[i]), val(eq + 1);
    const int n = atoi(val.c_str());
    static const char* const bits[8] = {"chain", "wide", "stem", "conv3", "skip_empty", "bneck",
                                        "sparse_tail", "tail_lists"};
    int bit = -1;
    for (int k = 0; k < 8; ++k) if (name == bits[k]) bit = k;
    if (bit >= 0) a.fusion = n ? a.fusion | (1 << bit) : a.fusion & ~(1 << bit);
    else if (name == "images" && (val == "u8" || val == "f32")) a.image_dtype = val == "u8" ? MILAN_DTYPE_U8 : MILAN_DTYPE_F32;
    else if (name == "masks" && (val == "none" || val == "u8" || val == "f32")) {
      a.masks = val != "none";
      a.mask_dtype = val == "f32" ? MILAN_DTYPE_F32 : MILAN_DTYPE_U8;
    }
    else if (name == "aligned") a.images_aligned4 = n != 0;
    else if (name == "share") a.share = n != 0;
    else if (name == "calib") a.calib = n != 0;
    else if (name == "spatial") a.spatial = n != 0;
    else if (name == "cus") a.genv.cus = n;
    else if (name == "experiments") a.genv.experiments = n != 0;
    else if (name == "MILAN_STEM_U8") a.env.stem_u8 = n != 0;
    else if (name == "MILAN_POOL_VEC") a.env.pool_vec = n != 0;
    else if (name == "MILAN_TAPS_INNER") a.env.taps_inner = n != 0;
    else if (name == "MILAN_PP") a.genv.pp = n;
    else if (name == "MILAN_PP128") a.genv.pp128 = n;
    else if (name == "MILAN_PP_PERSIST") a.genv.pp_persist = n;
    else if (name == "MILAN_TAP_INNER") a.genv.tap_inner = n;
    else if (name == "MILAN_TAP_SKIP") a.genv.tap_skip = n;
    else return usage(("unknown option " + std::string(argv[i])).c_str());
  }
  if (!a.genv.experiments) a.env.taps_inner = 0;   // (the product build never reads the knob)
  // (milan_encoder_absmax runs its pass in MILAN_PRECISION_F32)
  if (a.calib) { a.precision = MILAN_PRECISION_F32; a.trunk_f16 = 0; }

  // encoder.hip, encoder_finalize
  const bool ex = a.genv.experiments;
  ConvW stem = conv(wd, 3, 7, 2, 3, false, ex), stem_pair;
  if (wd <= 64 && wd % 8 == 0) {
    stem_pair.cout = wd; stem_pair.cin = 8; stem_pair.cin_real = 3; stem_pair.kh = 7; stem_pair.kw = 4;
    stem_pair.stride = 2; stem_pair.pad = 3; stem_pair.K = stem_pair.Kp = 224;
    stem_pair.w = sentinel(); stem_pair.ws = sentinel();
  }
  std::vector<Bottleneck> blocks[4];
  const bool basic = nets[which].basic;
  for (int li = 0, inplanes = wd; li < 4; ++li) {
    const int planes = wd << li, out = basic ? planes : 4 * planes;
    for (int bi = 0; bi < nets[which].blocks[li]; ++bi) {
      Bottleneck b;
      b.basic = basic;
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      if (basic) {
        b.c1 = conv(planes, inplanes, 3, stride, 1, true, ex);
        b.c2 = conv(planes, planes, 3, 1, 1, true, ex);
      } else {
        b.c1 = conv(planes, inplanes, 1, 1, 0, true, ex);
        b.c2 = conv(planes, planes, 3, stride, 1, true, ex);
        b.c3 = conv(out, planes, 1, 1, 0, true, ex);
      }
      b.has_down = bi == 0 && (!basic || li > 0);
      if (b.has_down) {
        b.down = conv(out, inplanes, 1, stride, 0, true, ex);
        if (!basic) fuse(b);
      }
      blocks[li].push_back(b);
      inplanes = out;
    }
  }
  a.blocks = blocks; a.stem = &stem; a.stem_pair = &stem_pair;
  a.zero = sentinel();

  // the arena at a made-up aligned address: the ping-pong is deterministic once it is carved
  Arena arena;
  arena.base = reinterpret_cast<char*>(uintptr_t(1) << 44);
  arena.size = size_t(1) << 43;
  EncBuffers pl;
  enc_carve(a.trunk_kind, wd, a.n, a.H, a.W, &arena, &pl);
  if (arena.off > arena.size) return usage("pass too large for the made-up arena");
  const EncSchedule sc = plan_encoder(a, pl);

  static const char* const family[MILAN_KERNEL_COUNT] = {
      "other", "pp32_256", "pp32_128", "split_other", "f32", "chain", "chain_wide", "stem",
      "conv3", "f16", "pp32t_256", "bneck"};
  static const char* const compact[] = {"none", "skip_empty", "classes"};
  static const char* const pool[] = {"f32", "split", "split8", "f16"};
  static const char* const c1n[] = {"ready", "launch", "fused", "list"};
  static const char* const c2n[] = {"none", "conv3", "gemm", "list"};
  int count[MILAN_KERNEL_COUNT] = {}, gemms = 0, lists = 0, per_line = 0;
  printf("pass split=%d fast=%d pair_stem=%d stem_u8=%d fused_stem=%d compact=%s tail=%d lists=%d "
         "k0=%d lists_l3=%d pool=%s,%s,%s,%s,%s levels=", sc.split, sc.fast, sc.pair_stem,
         sc.stem_u8, sc.fused_stem, compact[sc.compact], sc.tail, sc.lists, sc.k0, sc.lists_l3,
         pool[sc.pool[0]], pool[sc.pool[1]], pool[sc.pool[2]], pool[sc.pool[3]], pool[sc.pool[4]]);
  for (int l = 0; l < 5; ++l) printf("%dx%d%s", pl.lv.h[l], pl.lv.w[l], l < 4 ? "," : "");
  const int stem_family = sc.fused_stem ? MILAN_KERNEL_STEM : plan_gemm(sc.stem, a.genv).family;
  printf(" stem=%s\n", family[stem_family]);
  ++count[stem_family];
  if (!sc.fused_stem) ++gemms;
  for (const EncBlock& r : sc.blocks) {
    int fam[5];
    const GemmArgs* g[5];
    const int k = block_launches(r, a.genv, fam, g);
    bool alias = false;
    for (int i = 0; i < k; ++i) {
      if (g[i]) {
        alias = alias || g[i]->C == g[i]->A || g[i]->C == g[i]->aux || g[i]->C == g[i]->A2;
        ++gemms;
        if (g[i]->row_list) ++lists;
      } else if (fam[i] != MILAN_KERNEL_CONV3) {
        const ChainArgs& c = r.chain;
        alias = alias || c.X == c.T2 || c.X == c.R || c.X == c.A2 || c.X == c.C2in ||
                c.T1 == c.T2 || c.T1 == c.C2in || c.T1 == c.X;
      } else {
        alias = alias || r.g2.A == r.g2.C;
      }
    }
    const bool chain = r.form == EF_CHAIN_PLAIN || r.form == EF_CHAIN_DS;
    printf("block l%d.%d form=%s c1=%s c2=%s conv_front=%d c1_front=%d NR=%d kM=%d kO=%d x=%s y=%s "
           "t1=%s t1n=%s alias=%d launches=", r.stage + 1, r.index, enc_form_name(r.form), c1n[r.c1],
           c2n[r.c2], r.conv_front, r.c1_front, chain ? r.chain.NR : 0, r.kM, r.kO,
           buf_name(pl, r.X), buf_name(pl, r.Y), buf_name(pl, r.T1), buf_name(pl, r.T1_next), alias);
    for (int i = 0; i < k; ++i) {
      printf("%s%s%s", i ? "," : "", family[fam[i]], g[i] && g[i]->row_list ? "@list" : "");
      ++count[fam[i]];
      ++per_line;
    }
    printf("\n");
  }
  printf("families");
  int total = 0;
  for (int f = 0; f < MILAN_KERNEL_COUNT; ++f)
    if (count[f]) { printf(" %s:%d", family[f], count[f]); total += count[f]; }
  printf(" total=%d block_launches=%d launch_gemm=%d on_lists=%d\n", total, per_line, gemms, lists);
  return 0;
}
