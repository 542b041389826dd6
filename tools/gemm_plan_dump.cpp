// Prints the plan of one GEMM launch (csrc/gemm_plan.h) -- host only, no GPU, no HIP call:
//
//   g++ -std=c++17 -O1 tools/gemm_plan_dump.cpp -o gemm_plan_dump
//   gemm_plan_dump N Cin KH KW stride pad H W images f32|split|f16 [option ...]
//   gemm_plan_dump kernels     the product build's kernel forms (MILAN_GEMM_KERNELS), one
//                              "id=name" line each (id: the GemmKernel enumerator's value)
//
// N and Cin are per group.  Options (name=value):
//   out_split= Wt= row_list= groups= tile_hint= tap_ncls= M= ldc= ldaux=
//   A2=<channels of the second source>   epilogue=bias|relu|res_relu|tanh|sigmul|add|lstm|lse
//   stride2=   aux_split=   (default: a split launch's residual is split, SIGMUL's fp32)
//   m_live=1 m_live_mul=   a row count on the device   aniso=1 stride_w= pad_w=
//   shift_group=<q>   plan group q of the grouped conv as the per-group baseline launches it
//   cus= experiments=   and every knob of the launch path, MILAN_PP=0 and the like
// One "key=value" line per field of the plan; a refusal prints err= and msg= instead.
// tests/test_gemm_plan_host.py holds the parent dispatch's answers against it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../neuron-descriptions_amd/csrc/gemm_plan.h"

using namespace milan;

static int usage(const char* why) {
  fprintf(stderr, "gemm_plan_dump: %s\nusage: gemm_plan_dump N Cin KH KW stride pad H W images "
                  "f32|split|f16 [name=value ...]\n", why);
  return 2;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "kernels") == 0) {
#define MILAN_GK_PRINT(id, ...) printf("%d=%s\n", (int)id, #__VA_ARGS__);
#define MILAN_GK_SKIP(id, ...)
    MILAN_GEMM_KERNELS(MILAN_GK_PRINT, MILAN_GK_SKIP)
#undef MILAN_GK_PRINT
#undef MILAN_GK_SKIP
    return 0;
  }
  if (argc < 11) return usage("too few arguments");
  int v[9];
  for (int i = 0; i < 9; ++i) v[i] = atoi(argv[1 + i]);
  const std::string prec = argv[10];
  if (prec != "f32" && prec != "split" && prec != "f16") return usage("unknown precision");

  // operands at made-up, 16-byte aligned addresses: the plan looks at alignment only
  float* const base = reinterpret_cast<float*>(uintptr_t(1) << 32);
  GemmArgs g{};
  GemmEnv env;
  g.N = v[0]; g.Cin = v[1]; g.KH = v[2]; g.KW = v[3]; g.stride = v[4]; g.pad = v[5];
  g.H = v[6]; g.Wd = v[7];
  const int images = v[8];
  g.a_split = prec != "f32";
  g.f16 = prec == "f16";
  g.out_split = prec == "split";
  g.epilogue = EPI_BIAS;
  int a2 = 0, shift = -1, M = -1, ldc = -1, ldaux = -1, stride2 = 1, aux_split = -1;
  bool wt = false, list = false, live = false;
  for (int i = 11; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return usage("options are name=value");
    const std::string name(argv[i], eq - argv[i]), val(eq + 1);
    const int n = atoi(val.c_str());
    if (name == "out_split") g.out_split = n;
    else if (name == "Wt") wt = n != 0;
    else if (name == "A2") a2 = n;
    else if (name == "groups") g.groups = n;
    else if (name == "row_list") list = n != 0;
    else if (name == "tile_hint") g.tile_hint = n;
    else if (name == "tap_ncls") g.tap_ncls = n;
    else if (name == "M") M = n;
    else if (name == "ldc") ldc = n;
    else if (name == "ldaux") ldaux = n;
    else if (name == "shift_group") shift = n;
    else if (name == "stride2") stride2 = n;
    else if (name == "aux_split") aux_split = n;
    else if (name == "m_live") live = n != 0;
    else if (name == "m_live_mul") g.m_live_mul = n;
    else if (name == "aniso") g.aniso = n;
    else if (name == "stride_w") g.stride_w = n;
    else if (name == "pad_w") g.pad_w = n;
    else if (name == "cus") env.cus = n;
    else if (name == "experiments") env.experiments = n != 0;
    else if (name == "epilogue") {
      const char* names[] = {"bias", "relu", "res_relu", "tanh", "sigmul", "add", "lstm", "lse"};
      int e = -1;
      for (int k = 0; k < 8; ++k) if (val == names[k]) e = k;
      if (e < 0) return usage("unknown epilogue");
      g.epilogue = e;
    }
    else if (name == "MILAN_PP") env.pp = n;
    else if (name == "MILAN_PP128") env.pp128 = n;
    else if (name == "MILAN_PP_PERSIST") env.pp_persist = n;
    else if (name == "MILAN_TAP_INNER") env.tap_inner = n;
    else if (name == "MILAN_TAP_SKIP") env.tap_skip = n;
    else if (name == "MILAN_GROUP_LAUNCH") env.group_launch = n;
    else if (name == "MILAN_ABLATE") env.ablate = n;
    else if (name == "MILAN_TILE_HINT") env.tile_hint = n;
    else if (name == "MILAN_TILE_OVERRIDE") {
      int a = 0, b = 0, c = 0;
      if (sscanf(val.c_str(), "%d:%d:%d", &a, &b, &c) != 3) return usage("MILAN_TILE_OVERRIDE=N:K:hint");
      env.tile_override = {a, b, c};
    }
    else if (name == "MILAN_SCHED") env.sched = n;
    else if (name == "MILAN_CONV3X3") env.conv3x3 = n != 0;
    else if (name == "MILAN_LINEAR_KERNEL") env.linear_kernel = n;
    else if (name == "MILAN_PERSIST_LIN") env.persist_lin = n;
    else if (name == "MILAN_PERSIST") env.persist = n;
    else if (name == "MILAN_STAGGER") env.stagger = n;
    else if (name == "MILAN_STAGGER_ALL") env.stagger_all = n;
    else return usage(("unknown option " + name).c_str());
  }
  const int groups = g.groups > 1 ? g.groups : 1;
  g.Ho = (g.H + 2 * g.pad - g.KH) / g.stride + 1;
  g.Wo = g.aniso ? (g.Wd + 2 * g.pad_w - g.KW) / g.stride_w + 1
               : (g.Wd + 2 * g.pad - g.KW) / g.stride + 1;
  g.M = M > 0 ? M : images * g.Ho * g.Wo;
  g.K1 = g.KH * g.KW * g.Cin;
  g.K = g.K1 + a2;
  g.Kp = (g.K + 31) / 32 * 32;
  g.a_pix_stride = (long)g.Cin * groups;
  g.a_img_stride = (long)g.H * g.Wd * g.a_pix_stride;
  g.A = base;
  g.W = base + (1 << 20);
  g.bias = base + (2 << 20);
  g.C = base + (3 << 20);
  g.zero = base + (4 << 20);
  g.ldc = g.N * groups;
  if (wt) g.Wt = base + (5 << 20);
  if (a2 > 0) {
    g.A2 = base + (6 << 20);
    g.H2 = (g.Ho - 1) * stride2 + 1; g.W2d = (g.Wo - 1) * stride2 + 1; g.stride2 = stride2;
    g.a2_pix_stride = a2;
    g.a2_img_stride = (long)g.H2 * g.W2d * a2;
  } else {
    g.K1 = 0;
  }
  if (g.epilogue == EPI_BIAS_RES_RELU || g.epilogue == EPI_BIAS_ADD || g.epilogue == EPI_BIAS_SIGMUL) {
    g.aux = base + (7 << 20);
    g.aux_split = g.out_split && g.epilogue != EPI_BIAS_SIGMUL;
    g.ldaux = g.ldc;
    if (aux_split >= 0) g.aux_split = aux_split;
  }
  if (g.epilogue == EPI_LSTM) {
    g.aux = base + (7 << 20);
    g.C2 = base + (8 << 20);
    g.ldc = g.ldaux = g.N / 4;
  }
  if (g.epilogue == EPI_LSE) {
    g.ldc = 2 * ((g.N + 63) / 64);
    g.lse_tgt = reinterpret_cast<const long long*>(base + (9 << 20));
    g.lse_tgt_stride = 1;
    g.lse_x = base + (10 << 20);
  }
  if (ldc >= 0) g.ldc = ldc;
  if (ldaux >= 0) g.ldaux = ldaux;
  if (list) {
    g.row_list = reinterpret_cast<const int*>(base + (11 << 20));
    g.m_live = reinterpret_cast<const int*>(base + (12 << 20));
    g.m_live_mul = 1;
  }
  if (live) {
    g.m_live = reinterpret_cast<const int*>(base + (12 << 20));
    if (g.m_live_mul == 0) g.m_live_mul = 1;
  }
  if (groups > 1) {
    g.a_grp = g.Cin; g.w_grp = (long)g.N * g.Kp; g.bias_grp = g.N; g.c_grp = g.N; g.aux_grp = g.N;
  }
  if (shift >= 0) shift_group(g, shift);

  const GemmPlan p = plan_gemm(g, env);
  printf("row_list_supported=%d\n", p.err == 0 && p.list);
  if (p.err != 0) {
    printf("err=%d\nmsg=%s\n", p.err, p.msg);
    return 0;
  }
  static const char* const family[MILAN_KERNEL_COUNT] = {
      "other", "pp32_256", "pp32_128", "split_other", "f32", "chain", "chain_wide", "stem",
      "conv3", "f16", "pp32t_256", "bneck"};
  static const char* const out_mode[] = {"scalar", "vec4", "split8", "f16"};
  printf("kernel=%s\n", gemm_kernel_name(p.kernel));
  printf("grid=%d,%d\nthreads=%d\nlds=%d\n", p.grid_x, p.grid_y, p.threads, p.lds);
  printf("tile=%dx%d\ntiles=%d,%d\n", p.bm, p.bn, p.tiles_m, p.tiles_n);
  printf("out_mode=%s\ntap_inner=%d\ntap_ncls=%d\n", out_mode[p.out_mode], p.tap_inner, p.tap_ncls);
  printf("weights=%s\n", p.w_from_wt ? "Wt" : "W");
  printf("family=%s\n", family[p.family]);
  printf("launches=%s\n", p.per_group ? "per-group" : "one");
  return 0;
}
