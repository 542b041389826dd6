"""The case table of tests/test_gpu_gemm_forms.py and tests/test_gemm_forms_host.py: plain data.

One case = one launch of the implicit GEMM through hip.gemm_probe, at the smallest shape at which
its kernel form can still go wrong, with the kernel the plan (csrc/gemm_plan.h) is meant to name
for it.  tests/test_gemm_forms_host.py asks tools/gemm_plan_dump.cpp for every case's plan without
a GPU and holds the table to MILAN_GEMM_KERNELS: a product kernel without a case fails there.

Fields of a case (everything but id / kernel / prec / N / Cin has a default):
  id, kernel      the test's name and the kernel name gemm_plan_dump must print
  prec            'f32' (fp32 operands, fp32 MFMA) or 'split' (split-f16 operands)
  N, Cin          per group
  k, kw           kernel height (and width, default k); stride, pad (default k // 2)
  H, W, images    input extent; a Linear is k = 1, H = W = 1, images = rows
  out             'f32' | 'split' (default: the operands' format)
  epi             0..5 (gemmref.EPI_*); the residual / multiplicand is split with split output
                  except SIGMUL's (fp32)
  pad_c           C is a slice of a wider row: ldc = groups * N + 24, starting at column 8;
                  aux then has its own ldaux = groups * N + 40 (from column 16)
  pad_a           A is a slice: a_pix_stride = groups * Cin + 32, starting at channel 16
  A2, stride2     channels and stride of the second source (H2 x W2d is made non-square: one
                  spare column)
  groups
  m_live          (value, multiplier) of the device-side row count.  The full sweep -- 0, 1, one
                  less than a tile, a tile, straddling, M, more than M -- runs with multiplier 1
                  on the 1x1 form of every tile family and in whole images (multiplier Ho * Wo,
                  where "one less than a tile" does not exist) on the k x k forms; a grouped
                  launch with a row count is the launcher's refusal
  rows            row list: 'one' | 255 | 256 | 257 | 'gaps' (every third image missing, the
                  others with holes) | 'all'
  tap_ncls        -1: a tap-inner launch in linear tile order
  no_wt           the (slice, tap, channel) weight copy is not made
  aniso           (stride_w, pad_w)
  env             the knob setting the case needs (one fresh process per setting)
  refused         the text of the refusal instead of a kernel
"""

IG = 'igemm_kernel<%s>'
S16 = 'igemm_split16_kernel<%s>'
TM2 = 'igemm_split16_tm2_kernel<256, 64, 3>'
TM2G = 'igemm_split16_tm2_kernel<256, 64, 3, true>'
PP = 'igemm_split16_pp_kernel'
PP32 = 'igemm_split16_pp32_kernel'
PP32N = 'igemm_split16_pp32n_kernel<%d>'
PP32T = 'igemm_split16_pp32t_kernel<%d>'
PP32L = 'igemm_split16_pp32l_kernel<%s>'
GPP32N = 'igemm_grouped_pp32n_kernel'
GPP32T = 'igemm_grouped_pp32t_kernel'
LINP = 'igemm_split16_linp_kernel<5>'
F_64_C4, F_64_C32 = IG % '256, 64, 2, false, false', IG % '256, 64, 2, true, false'
F_128_C4, F_128_C32 = IG % '128, 128, 2, false, false', IG % '128, 128, 2, true, false'
S_64_C8, S_64_C32 = IG % '256, 64, 2, false, true', IG % '256, 64, 2, true, true'

EPI = ('bias', 'relu', 'res_relu', 'tanh', 'sigmul', 'add')
CASES = []


def case(id, kernel, prec, N, Cin, **kw):
    assert all(c['id'] != id for c in CASES), id
    CASES.append(dict(id=id, kernel=kernel, prec=prec, N=N, Cin=Cin, **kw))


def lin(id, kernel, prec, N, K, rows, **kw):
    case(id, kernel, prec, N, K, images=rows, **kw)


# ---- the fp32 general kernel ---------------------------------------------------------------------
# 256 x 64 tile (N <= 64), per-lane taps (Cin % 32 != 0): K != Kp (36 -> 64, 108 -> 128)
case('f32-64c4-n8-cin4', F_64_C4, 'f32', 8, 4, k=3, H=5, W=5, images=3)
case('f32-64c4-n20-cin12', F_64_C4, 'f32', 20, 12, k=3, H=9, W=7, images=5, epi=1)
case('f32-64c4-n20-scalar', F_64_C4, 'f32', 20, 12, k=3, H=9, W=7, images=5, ldc=23, ldaux=21,
     epi=2)
for m in (1, 255, 256, 257, 600):
    lin('f32-64c32-m%d' % m, F_64_C32, 'f32', 64, 32, m)
lin('f32-64c32-k96-slices', F_64_C32, 'f32', 64, 96, 257, pad_c=True, pad_a=True, epi=5)
# 128 x 128 tile
for m in (1, 127, 128, 129, 300):
    lin('f32-128c32-m%d' % m, F_128_C32, 'f32', 128, 64, m)
lin('f32-128c32-n136', F_128_C32, 'f32', 136, 32, 257, pad_c=True, pad_a=True)
lin('f32-128c32-n384-k96', F_128_C32, 'f32', 384, 96, 130)
lin('f32-128c32-n256-k288', F_128_C32, 'f32', 256, 288, 129)
case('f32-128c4-n136-cin12', F_128_C4, 'f32', 136, 12, k=3, H=6, W=5, images=9, pad_c=True)
case('f32-128c32-3x3-borders', F_128_C32, 'f32', 128, 32, k=3, H=5, W=5, images=11, stride=2)
for e in range(6):
    lin('f32-vec4-epi-%s' % EPI[e], F_128_C32, 'f32', 136, 32, 257, epi=e, pad_c=True)
    lin('f32-scalar-epi-%s' % EPI[e], F_64_C4, 'f32', 20, 12, 257, epi=e, ldc=23, ldaux=21)
# anisotropic stride / pad: the pixel-pair stem's class (7 x 4 taps of 8-channel pixel pairs,
# stride 2 down, 1 across)
case('f32-aniso-stem', F_64_C4, 'f32', 64, 8, k=7, kw=4, stride=2, pad=3, aniso=(1, 1), H=13, W=6,
     images=3, epi=1)
case('split-aniso-stem', S_64_C8, 'split', 64, 8, k=7, kw=4, stride=2, pad=3, aniso=(1, 1), H=13,
     W=6, images=3, out='f32')
# the device-side row count: none, one, around a tile, all, more than all
for v in (0, 1, 255, 256, 300, 600, 700):
    lin('f32-64c32-live%d' % v, F_64_C32, 'f32', 64, 32, 600, m_live=(v, 1))
for v in (0, 1, 127, 128, 200, 300, 400):
    lin('f32-128c32-live%d' % v, F_128_C32, 'f32', 128, 32, 300, m_live=(v, 1), epi=2)
case('f32-128c32-live-images', F_128_C32, 'f32', 128, 32, k=3, H=5, W=5, images=11,
     m_live=(6, 25), epi=1)
# grouped
case('f32-64c4-groups2', IG % '256, 64, 2, false, false, true', 'f32', 32, 12, k=5, H=7, W=8,
     images=5, groups=2, epi=1)
case('f32-64c32-groups3', IG % '256, 64, 2, true, false, true', 'f32', 64, 32, k=3, H=5, W=5,
     images=11, groups=3, pad_c=True, pad_a=True)
case('f32-128c4-groups2-n136', IG % '128, 128, 2, false, false, true', 'f32', 136, 12, k=3, H=6,
     W=5, images=9, groups=2, epi=2)
case('f32-128c32-groups2', IG % '128, 128, 2, true, false, true', 'f32', 128, 32, k=1, H=5, W=5,
     images=11, groups=2, pad_c=True)

# ---- split operands, N <= 64 ---------------------------------------------------------------------
case('s64c8-cin8', S_64_C8, 'split', 64, 8, k=3, H=5, W=5, images=11)           # K 72 -> Kp 96
case('s64c8-n8-epi', S_64_C8, 'split', 8, 8, k=3, H=5, W=5, images=11, epi=2, pad_c=True)
for m in (1, 255, 256, 257, 600):
    lin('s64c32-m%d' % m, S_64_C32, 'split', 64, 32, m)
lin('s64c32-n8-k64', S_64_C32, 'split', 8, 64, 257, epi=1)
lin('s64c32-k96-slices', S_64_C32, 'split', 64, 96, 257, pad_c=True, pad_a=True, epi=5)
lin('s64c32-k288-f32out', S_64_C32, 'split', 64, 288, 257, out='f32', epi=3)
lin('s64c32-sigmul', S_64_C32, 'split', 64, 64, 257, epi=4, pad_c=True)
case('tm2-borders', TM2, 'split', 64, 32, k=3, H=5, W=5, images=11)             # 275 rows
case('tm2-n8-stride2', TM2, 'split', 8, 32, k=3, H=9, W=7, images=21, stride=2, epi=2, pad_c=True,
     pad_a=True)
case('tm2-live-images', TM2, 'split', 64, 32, k=3, H=5, W=5, images=24, m_live=(11, 25), epi=1)
for v in (0, 1, 10, 11, 24, 30):     # (250 rows: under a tile; 275: straddling)
    case('tm2-live-%dimg' % v, TM2, 'split', 64, 32, k=3, H=5, W=5, images=24, m_live=(v, 25))
for v in (255, 256, 257):
    case('tm2-live-%drows' % v, TM2, 'split', 64, 32, k=3, H=5, W=5, images=24, m_live=(v, 1),
         epi=2)
for v in (0, 1, 255, 256, 300, 600, 700):
    lin('s64c32-live%d' % v, S_64_C32, 'split', 64, 32, 600, m_live=(v, 1), epi=1)
for v, mul in ((0, 25), (30, 25), (255, 1), (257, 1)):
    case('s64c8-live-%dx%d' % (v, mul), S_64_C8, 'split', 64, 8, k=3, H=5, W=5, images=24,
         m_live=(v, mul))
case('tm2-groups2', TM2G, 'split', 64, 32, k=3, H=5, W=5, images=11, groups=2, epi=1)
case('tm2-groups3-slices', TM2G, 'split', 64, 32, k=3, H=5, W=5, images=11, groups=3, epi=2,
     pad_c=True, pad_a=True)

# ---- the pair-staged tile: 128 columns ----------------------------------------------------------
for m in (1, 255, 256, 257, 600):
    lin('pp32n128-m%d' % m, PP32N % 128, 'split', 128, 32, m)
lin('pp32n128-k64', PP32N % 128, 'split', 128, 64, 257, epi=1)
lin('pp32n128-k96', PP32N % 128, 'split', 128, 96, 257)     # three pairs: an odd count
lin('pp32n128-k288', PP32N % 128, 'split', 128, 288, 257)
lin('pp32n128-n136', PP32N % 128, 'split', 136, 96, 300, pad_c=True, pad_a=True, epi=2)
lin('pp32n128-n384', PP32N % 128, 'split', 384, 64, 257, epi=5, pad_c=True)
for e in (0, 1, 2, 4, 5):
    lin('pp32n128-split-epi-%s' % EPI[e], PP32N % 128, 'split', 136, 32, 257, epi=e, pad_c=True)
for e in range(6):
    lin('pp32n128-f32out-epi-%s' % EPI[e], PP32N % 128, 'split', 136, 32, 257, epi=e, pad_c=True,
        out='f32')
case('pp32n128-3x3-no-wt', PP32N % 128, 'split', 128, 32, k=3, H=5, W=5, images=11, no_wt=True)
# ---- ... 256 columns -----------------------------------------------------------------------------
for m in (1, 255, 256, 257, 600):
    lin('pp32-m%d' % m, PP32, 'split', 256, 32, m)
lin('pp32-k96-slices', PP32, 'split', 256, 96, 257, pad_c=True, pad_a=True, epi=2)
lin('pp32-n512-k64', PP32, 'split', 512, 64, 257, epi=1)
lin('pp32-n2296', PP32, 'split', 2296, 32, 257, out='f32')   # N > 2048, pad256 <= pad128
lin('pp32-n2296-split', PP32, 'split', 2296, 96, 130, epi=5, pad_c=True)
lin('pp32-k288', PP32, 'split', 256, 288, 257, epi=4)
for e in (3, 4):
    lin('pp32-f32out-epi-%s' % EPI[e], PP32, 'split', 256, 64, 257, epi=e, out='f32', pad_c=True)
case('pp32-3x3-no-wt', PP32, 'split', 256, 32, k=3, H=5, W=5, images=11, no_wt=True, epi=2)
for v in (0, 1, 255, 256, 300, 600, 700):
    lin('pp32-live%d' % v, PP32, 'split', 256, 32, 600, m_live=(v, 1))
for v in (0, 1, 255, 256, 300, 600, 700):
    lin('pp32n128-live%d' % v, PP32N % 128, 'split', 128, 32, 600, m_live=(v, 1), epi=2)
case('pp32n128-live-images', PP32N % 128, 'split', 128, 32, k=1, H=5, W=5, images=24,
     m_live=(11, 25), epi=2)

# ---- tap-inner k order, border-class tiles -------------------------------------------------------
# (the geometries of test_gpu_tap_skip.py's first three cases within this file's row budget)
TAP_GEOMETRIES = ((3, 14, 14, 256), (2, 17, 17, 128), (3, 7, 7, 256))
for i, (n, h, w, cout) in enumerate(TAP_GEOMETRIES):
    for e in (1, 2):
        case('tap%d-%s' % (i, EPI[e]), PP32T % cout, 'split', cout, 32, k=3, H=h, W=w, images=n,
             epi=e, pad_c=True)
case('tap-linear-order', PP32T % 256, 'split', 256, 32, k=3, H=14, W=14, images=3, epi=2,
     pad_c=True, tap_ncls=-1)
case('tap-stride2-f32out', PP32T % 128, 'split', 136, 32, k=3, H=15, W=14, images=3, stride=2,
     out='f32', epi=1)
case('tap-live-images', PP32T % 256, 'split', 256, 32, k=3, H=7, W=7, images=12, m_live=(5, 49),
     epi=2)

# The first geometry of test_gpu_tap_skip.py was chosen for its two 32-channel slices: Cin = 64,
# K = 576 -- the one case above this file's K <= 288 budget.
case('tap-two-slices', PP32T % 256, 'split', 256, 64, k=3, H=14, W=14, images=3, epi=2, pad_c=True)
# the device-side row count under class tiles: whole images (tap_tile counts live images per
# class: none, one, a tile's worth, straddling, all, more than all), and a count that is no
# multiple of an image (the plan then keeps the linear tile order)
for v in (0, 1, 4, 5, 10, 12):
    case('tap-live-%dimg' % v, PP32T % 256, 'split', 256, 32, k=3, H=8, W=8, images=10,
         m_live=(v, 64), epi=2)
for v in (255, 256, 257):
    case('tap-live-%drows' % v, PP32T % 256, 'split', 256, 32, k=3, H=8, W=8, images=10,
         m_live=(v, 1), epi=1)
for v in (0, 5, 12):
    case('tap128-live-%dimg' % v, PP32T % 128, 'split', 128, 32, k=3, H=8, W=8, images=10,
         m_live=(v, 64), epi=1, pad_c=True)

# ---- M = 1, 255, 256, 257 on the k x k forms: 1 x 1, five 3 x 17, one 16 x 16, one 1 x 257 image --
KXK_EDGES = ((1, 1, 1, 1), (255, 5, 3, 17), (256, 1, 16, 16), (257, 1, 1, 257))
for m, n, h, w in KXK_EDGES:
    case('tm2-m%d' % m, TM2, 'split', 64, 32, k=3, H=h, W=w, images=n, epi=1)
    case('tap256-m%d' % m, PP32T % 256, 'split', 256, 32, k=3, H=h, W=w, images=n, epi=2)
    case('tap128-m%d' % m, PP32T % 128, 'split', 128, 32, k=3, H=h, W=w, images=n)
    case('s64c8-m%d' % m, S_64_C8, 'split', 64, 8, k=3, H=h, W=w, images=n, epi=1)
    case('f32-64c4-m%d' % m, F_64_C4, 'f32', 64, 12, k=3, H=h, W=w, images=n)
    case('f32-128c32-3x3-m%d' % m, F_128_C32, 'f32', 128, 32, k=3, H=h, W=w, images=n, epi=1)

# ---- the second operand source -------------------------------------------------------------------
for n, kern in ((128, PP32N % 128), (256, PP32)):
    for s2 in (1, 2):
        case('two-src-n%d-stride%d' % (n, s2), kern, 'split', n, 32, k=1, H=9, W=7, images=5, A2=32,
             stride2=s2, epi=2, pad_c=True, pad_a=True)
case('two-src-k2-96', PP32, 'split', 256, 32, k=1, H=9, W=7, images=5, A2=96, stride2=2)
case('two-src-k1-48', None, 'split', 256, 48, k=1, H=9, W=7, images=5, A2=32,
     refused='gemm: split-f16 operands with Cin % 32 != 0 need Cin % 8 == 0 and N <= 64 '
             '(Cin=48 N=256)')
case('two-src-f32', None, 'f32', 256, 32, k=1, H=9, W=7, images=5, A2=32,
     refused='gemm: two-source A needs the split16 kernels')

# ---- row lists -----------------------------------------------------------------------------------
for rows in ('one', 255, 256, 257, 'gaps', 'all'):
    case('list-1x1-%s' % rows, PP32L % 'false', 'split', 256, 32, k=1, H=5, W=5, images=24,
         rows=rows, epi=2)
    case('list-3x3-%s' % rows, PP32L % 'true', 'split', 256, 32, k=3, H=5, W=5, images=24,
         rows=rows, epi=1, pad_c=True)
case('list-two-src', PP32L % 'false', 'split', 256, 32, k=1, H=5, W=5, images=24, rows='gaps',
     A2=32, stride2=2, epi=2, pad_c=True, pad_a=True)
case('list-n128', None, 'split', 128, 32, k=1, H=5, W=5, images=24, rows='gaps',
     refused='gemm: no row-list form of this launch (N=128 Cin=32 1x1)')

# ---- grouped launches on the pair-staged tile ----------------------------------------------------
case('gpp32n-groups2', GPP32N, 'split', 128, 32, k=1, H=5, W=5, images=11, groups=2, epi=1)
case('gpp32n-groups3-n136', GPP32N, 'split', 136, 32, k=3, H=5, W=5, images=11, groups=3,
     no_wt=True, epi=2, pad_c=True, pad_a=True)
case('gpp32t-groups2', GPP32T, 'split', 128, 32, k=3, H=7, W=7, images=6, groups=2, epi=2)
case('gpp32t-groups3-n136', GPP32T, 'split', 136, 32, k=3, H=5, W=5, images=11, groups=3, epi=1,
     pad_c=True, pad_a=True)
case('gpp32n-live', None, 'split', 128, 32, k=1, H=5, W=5, images=11, groups=2, m_live=(6, 25),
     refused='gemm: a grouped launch is a plain conv (groups=2)', refused_by='launcher')

# ---- refusals of the epilogue form ---------------------------------------------------------------
lin('refuse-tanh-split', None, 'split', 128, 32, 64, epi=3,
    refused='gemm: unsupported split-format epilogue (N=128 ldc=128 epi=3)')
lin('refuse-sigmul-split-aux', None, 'split', 128, 32, 64, epi=4, aux='split',
    refused='gemm: unsupported split-format epilogue (N=128 ldc=128 epi=4)')

# ---- forms behind a knob -------------------------------------------------------------------------
# (rows of the persistent forms: 257 tiles of 256 rows, more than the device's 256 CUs, the last
# one ragged)
PERSIST_ROWS = 256 * 256 + 37
PP0, PP2, PP128_0, PERSIST = ({'MILAN_PP': 0}, {'MILAN_PP': 2}, {'MILAN_PP128': 0},
                              {'MILAN_PP_PERSIST': 1})
lin('s16-256-s3', S16 % '256, 256, 5, 3', 'split', 256, 96, 257, env=PP0, epi=2, pad_c=True)
lin('s16-256-s3-k32', S16 % '256, 256, 5, 3', 'split', 256, 32, 300, env=PP0)
case('s16-256-s0', S16 % '256, 256, 5, 0', 'split', 256, 32, k=3, H=5, W=5, images=11, env=PP0,
     epi=1)
lin('linp', LINP, 'split', 256, 64, PERSIST_ROWS, env=PP0, epi=1)
lin('s16-128-s3', S16 % '256, 128, 3, 3', 'split', 136, 96, 257, env=PP128_0, epi=2, pad_c=True)
lin('s16-128-s3-k32', S16 % '256, 128, 3, 3', 'split', 128, 32, 300, env=PP128_0)
case('s16-128-s0', S16 % '256, 128, 3, 0', 'split', 128, 32, k=3, H=5, W=5, images=11, env=PP128_0,
     epi=1)
lin('pp16', PP, 'split', 256, 96, 257, env=PP2, epi=2, pad_c=True)
lin('pp16-k32', PP, 'split', 256, 32, 300, env=PP2)
lin('pp32n256-persistent', PP32N % 256, 'split', 256, 32, PERSIST_ROWS, env=PERSIST, epi=1)

# The default-environment twin of a knob case whose bits gemm_plan.h promises to be the same
# ("same bits; A/B timing", "the same tile function in the same k order"): knob id -> twin id.
SAME_BITS = {
    's16-256-s3': 'pp32-twin-k96', 's16-256-s3-k32': 'pp32-twin-k32', 's16-256-s0': 'pp32-twin-3x3',
    's16-128-s3': 'pp32n128-twin-k96', 's16-128-s3-k32': 'pp32n128-twin-k32',
    's16-128-s0': 'pp32n128-twin-3x3', 'pp32n256-persistent': 'pp32-twin-persistent',
    'linp': 'pp32-twin-linp',
}
lin('pp32-twin-k96', PP32, 'split', 256, 96, 257, epi=2, pad_c=True)
lin('pp32-twin-k32', PP32, 'split', 256, 32, 300)
case('pp32-twin-3x3', PP32, 'split', 256, 32, k=3, H=5, W=5, images=11, epi=1, no_wt=True)
lin('pp32n128-twin-k96', PP32N % 128, 'split', 136, 96, 257, epi=2, pad_c=True)
lin('pp32n128-twin-k32', PP32N % 128, 'split', 128, 32, 300)
case('pp32n128-twin-3x3', PP32N % 128, 'split', 128, 32, k=3, H=5, W=5, images=11, epi=1,
     no_wt=True)
lin('pp32-twin-persistent', PP32, 'split', 256, 32, PERSIST_ROWS, epi=1)
lin('pp32-twin-linp', PP32, 'split', 256, 64, PERSIST_ROWS, epi=1)

# Product kernels without a case, each with its reason (tests/test_gemm_forms_host.py).
EXEMPT = {
    'igemm_f16_pp32_kernel<128, false>': 'fast mode: K-side units and operand packing of its own',
    'igemm_f16_pp32_kernel<128, true>': 'fast mode: K-side units and operand packing of its own',
    'igemm_f16_pp32_kernel<256, false>': 'fast mode: K-side units and operand packing of its own',
    'igemm_f16_pp32_kernel<256, true>': 'fast mode: K-side units and operand packing of its own',
}
# Epilogues the probe refuses (extra buffers; float64 tests at model level)
EXEMPT_EPILOGUES = {
    'lstm': 'tests/test_gpu_full_decoder.py',
    'lse': 'tests/test_gpu_lm_lse.py',
}


def by_id(id):
    return next(c for c in CASES if c['id'] == id)


# ---- what the fields mean: the launch's geometry and the question for gemm_plan_dump ------------
def geometry(c):
    """every derived number of a case, as the probe's fields of the same names"""
    kh = c.get('k', 1)
    kw = c.get('kw', kh)
    stride, pad = c.get('stride', 1), c.get('pad', kh // 2)
    stride_w, pad_w = c.get('aniso', (stride, pad))
    h, w, images = c.get('H', 1), c.get('W', 1), c.get('images', 1)
    groups = c.get('groups', 1)
    n, cin = c['N'], c['Cin']
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad_w - kw) // stride_w + 1
    split = c['prec'] == 'split'
    out_split = c.get('out', c['prec']) == 'split'
    epi = c.get('epi', 0)
    uses_aux = epi in (2, 4, 5)
    aux_fmt = c.get('aux', 'split' if out_split and epi != 4 else 'f32') if uses_aux else None
    a2 = c.get('A2', 0)
    stride2 = c.get('stride2', 1)
    k1 = kh * kw * cin
    g = dict(KH=kh, KW=kw, stride=stride, pad=pad, aniso=int('aniso' in c), stride_w=stride_w,
             pad_w=pad_w, H=h, Wd=w, images=images, groups=groups, N=n, Cin=cin, Ho=ho, Wo=wo,
             M=images * ho * wo, K=k1 + a2, K1=k1 if a2 else 0, C2=a2, stride2=stride2,
             H2=(ho - 1) * stride2 + 1, W2d=(wo - 1) * stride2 + 2,
             a_split=int(split), out_split=int(out_split), epilogue=epi, aux_fmt=aux_fmt,
             aux_split=int(aux_fmt == 'split'))
    g['Kp'] = (g['K'] + 31) // 32 * 32
    gn = groups * n
    g['c_col'], g['ldc'] = (8, gn + 24) if c.get('pad_c') else (0, c.get('ldc', gn))
    g['aux_col'], g['ldaux'] = (16, gn + 40) if c.get('pad_c') else (0, c.get('ldaux', gn))
    g['a_col'], g['a_pix_stride'] = (16, groups * cin + 32) if c.get('pad_a') else (0, groups * cin)
    g['a2_col'], g['a2_pix_stride'] = (16, a2 + 32) if c.get('pad_a') else (0, a2)
    # the weight copy in (slice, tap, channel) order exists when the trunk would have made it
    g['Wt'] = int(split and not c.get('no_wt') and 1 < kh * kw <= 32 and g['K'] == g['Kp'] and
                  cin % 32 == 0)
    return g


def dump_args(c):
    """the arguments of tools/gemm_plan_dump.cpp that ask for this case's plan"""
    g = geometry(c)
    args = [g['N'], g['Cin'], g['KH'], g['KW'], g['stride'], g['pad'], g['H'], g['Wd'],
            g['images'], c['prec'], 'out_split=%d' % g['out_split'], 'Wt=%d' % g['Wt'],
            'epilogue=%s' % EPI[g['epilogue']], 'ldc=%d' % g['ldc']]
    if g['aux_fmt']:
        args += ['ldaux=%d' % g['ldaux'], 'aux_split=%d' % g['aux_split']]
    if g['aniso']:
        args += ['aniso=1', 'stride_w=%d' % g['stride_w'], 'pad_w=%d' % g['pad_w']]
    if g['C2']:
        args += ['A2=%d' % g['C2'], 'stride2=%d' % g['stride2']]
    if g['groups'] > 1:
        args.append('groups=%d' % g['groups'])
    if 'rows' in c:
        args.append('row_list=1')
    elif 'm_live' in c:
        args += ['m_live=1', 'm_live_mul=%d' % c['m_live'][1]]
    if 'tap_ncls' in c:
        args.append('tap_ncls=%d' % c['tap_ncls'])
    args += ['%s=%d' % kv for kv in sorted(c.get('env', {}).items())]
    return [str(a) for a in args]
