"""The GEMM plan (csrc/gemm_plan.h) against the dispatch it replaced.

tools/gemm_plan_dump.cpp is compiled for the host (no GPU, no HIP) and asked for the plan of
each case; the expected values were written by hand from the decision tree of the launchers
that plan_gemm() replaced (launch_gemm_impl / launch_split16 / launch_split16_pp32 / ... and the
two predicates row_list_supported / groups_supported), not printed by the new code.

Default knobs, 256 CUs, product build, split operands with split output unless a case says
otherwise.  Convs run on 4 images of 14 x 14.
"""
import pathlib
import shutil
import subprocess

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
SRC = REPO / 'tools' / 'gemm_plan_dump.cpp'


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    cxx = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_dump'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', str(SRC), '-o', str(exe)],
                   check=True)
    cache = {}

    def run(*args):
        key = tuple(str(a) for a in args)
        if key not in cache:
            out = subprocess.run([str(exe), *key], check=True, capture_output=True, text=True)
            cache[key] = dict(line.split('=', 1) for line in out.stdout.splitlines())
        return cache[key]
    return run


def conv(n, cin, k, prec='split', *opts, size=14, images=4, stride=1):
    return (n, cin, k, k, stride, k // 2, size, size, images, prec) + opts


def linear(n, k, prec='split', *opts, rows=64):
    return (n, k, 1, 1, 1, 0, 1, 1, rows, prec) + opts


IG = 'igemm_kernel<%s>'
S16 = 'igemm_split16_kernel<%s>'
PP32 = 'igemm_split16_pp32_kernel'
PP32N = 'igemm_split16_pp32n_kernel<%d>'
PP32T = 'igemm_split16_pp32t_kernel<%d>'
PP32L = 'igemm_split16_pp32l_kernel<%s>'
F16 = 'igemm_f16_pp32_kernel<%s>'
LINP = 'igemm_split16_linp_kernel<5>'
NO_LIST = 'gemm: no row-list form of this launch (N=%d Cin=%d %dx%d)'

# 4 images of 14 x 14 = 784 rows = 4 row tiles of 256.  A 3 x 3 / pad 1 conv has 9 border
# classes: the 12 x 12 middle (4 * 144 = 576 pixels, 3 tiles), four edges (48 pixels) and four
# corners (4 pixels), each rounded up to 8 workgroups per column tile: 9 * 8 = 72.
CASES = [
    # ---- plain kernels and tiles ----
    ('f32 N64 Cin64', conv(64, 64, 1, 'f32'),
     dict(kernel=IG % '256, 64, 2, true, false', family='f32', out_mode='vec4', grid='4,1',
          threads='256', launches='one')),
    ('f32 N64 Cin12', conv(64, 12, 1, 'f32'), dict(kernel=IG % '256, 64, 2, false, false')),
    ('f32 N128', conv(128, 64, 1, 'f32'),
     dict(kernel=IG % '128, 128, 2, true, false', grid='7,1', tile='128x128', lds='65536')),
    ('f32 groups=2', conv(128, 64, 3, 'f32', 'groups=2'),
     dict(kernel=IG % '128, 128, 2, true, false, true', grid='7,2', launches='one', family='f32')),
    ('split N64 3x3', conv(64, 64, 3),
     dict(kernel='igemm_split16_tm2_kernel<256, 64, 3>', threads='256', lds='61440', grid='4,1',
          family='split_other', out_mode='split8')),
    ('split N64 1x1', conv(64, 64, 1), dict(kernel=IG % '256, 64, 2, true, true', lds='81920')),
    ('split N64 Cin8', conv(64, 8, 3), dict(kernel=IG % '256, 64, 2, false, true')),
    ('split N128 Cin8', conv(128, 8, 3),
     dict(err='-2', msg='gemm: split-f16 operands with Cin % 32 != 0 need Cin % 8 == 0 and '
                        'N <= 64 (Cin=8 N=128)')),
    # ---- pair-staged tile, k order and width ----
    ('N256 1x1', conv(256, 64, 1),
     dict(kernel=PP32, lds='163840', grid='4,1', threads='512', family='pp32_256', tap_inner='0')),
    ('N256 3x3 Wt', conv(256, 64, 3, 'split', 'Wt=1'),
     dict(kernel=PP32T % 256, tap_ncls='9', grid='72,1', tap_inner='1', weights='Wt',
          family='pp32t_256')),
    ('N256 3x3 Wt TAP_SKIP=0', conv(256, 64, 3, 'split', 'Wt=1', 'MILAN_TAP_SKIP=0'),
     dict(kernel=PP32T % 256, tap_ncls='0', grid='4,1', tap_inner='1')),
    ('N256 3x3 Wt tap_ncls=-1', conv(256, 64, 3, 'split', 'Wt=1', 'tap_ncls=-1'),
     dict(kernel=PP32T % 256, tap_ncls='0', grid='4,1', tap_inner='1')),
    ('N256 3x3 no Wt', conv(256, 64, 3), dict(kernel=PP32, tap_inner='0', weights='W', grid='4,1')),
    ('N256 3x3 TAP_INNER=0', conv(256, 64, 3, 'split', 'Wt=1', 'MILAN_TAP_INNER=0'),
     dict(kernel=PP32, tap_inner='0', weights='W', family='pp32_256')),
    ('N128 1x1', conv(128, 64, 1), dict(kernel=PP32N % 128, grid='4,1', family='pp32_128',
                                        lds='163840')),
    ('N128 3x3 Wt', conv(128, 64, 3, 'split', 'Wt=1'),
     dict(kernel=PP32T % 128, tap_ncls='9', grid='72,1', family='pp32_128')),
    ('N5004 K512', linear(5004, 512, 'split', 'out_split=0'),
     dict(kernel=PP32, tile='256x256', out_mode='vec4', grid='20,1')),
    ('N3904 K512', linear(3904, 512, 'split', 'out_split=0'),
     dict(kernel=PP32N % 128, tile='256x128', grid='31,1')),
    # ---- knobs ----
    ('PP=0 tiles > cus', linear(256, 512, 'split', 'MILAN_PP=0', rows=100000),
     dict(kernel=LINP, grid='256,1', threads='512', lds='163840', family='split_other')),
    ('PP=0 tiles <= cus', linear(256, 512, 'split', 'MILAN_PP=0', rows=256 * 256),
     dict(kernel=S16 % '256, 256, 5, 3', grid='256,1', threads='512', lds='163840')),
    ('PP=0 3x3', conv(256, 64, 3, 'split', 'Wt=1', 'MILAN_PP=0'),
     dict(kernel=S16 % '256, 256, 5, 0', tap_inner='0', weights='W')),
    ('PP=2', conv(256, 64, 1, 'split', 'MILAN_PP=2'),
     dict(kernel='igemm_split16_pp_kernel', lds='131072', threads='512', family='split_other')),
    ('PP128=0 N128 1x1', conv(128, 64, 1, 'split', 'MILAN_PP128=0'),
     dict(kernel=S16 % '256, 128, 3, 3', threads='256', lds='73728')),
    ('PP128=0 N128 3x3', conv(128, 64, 3, 'split', 'Wt=1', 'MILAN_PP128=0'),
     dict(kernel=S16 % '256, 128, 3, 0', tap_inner='0')),
    ('PP_PERSIST=1 tiles > cus', linear(256, 512, 'split', 'MILAN_PP_PERSIST=1', rows=100000),
     dict(kernel=PP32N % 256, grid='256,1', family='pp32_256')),
    # ---- fast mode ----
    ('f16 N256 Wt', conv(256, 64, 3, 'f16', 'Wt=1'),
     dict(kernel=F16 % '256, true', out_mode='f16', family='f16', tap_ncls='9', grid='72,1')),
    ('f16 N256', conv(256, 64, 3, 'f16'), dict(kernel=F16 % '256, false', grid='4,1')),
    ('f16 N128 Wt', conv(128, 64, 3, 'f16', 'Wt=1'), dict(kernel=F16 % '128, true', family='f16')),
    ('f16 N128', conv(128, 64, 3, 'f16'), dict(kernel=F16 % '128, false', lds='163840')),
    ('f16 N64', conv(64, 64, 3, 'f16'),
     dict(err='-2', msg='gemm: unsupported fast-mode (f16) layer N=64 Cin=64 epi=0')),
    # ---- row lists ----
    ('list N256 1x1', conv(256, 64, 1, 'split', 'row_list=1'),
     dict(kernel=PP32L % 'false', family='pp32_256', grid='4,1', tap_ncls='0',
          row_list_supported='1')),
    ('list N256 3x3 Wt', conv(256, 64, 3, 'split', 'Wt=1', 'row_list=1'),
     dict(kernel=PP32L % 'true', family='pp32t_256', tap_inner='1', weights='Wt', tap_ncls='0',
          grid='4,1', row_list_supported='1')),
    ('list N256 3x3 no Wt', conv(256, 64, 3, 'split', 'row_list=1'),
     dict(err='-2', msg=NO_LIST % (256, 64, 3, 3), row_list_supported='0')),
    ('list N128', conv(128, 64, 1, 'split', 'row_list=1'),
     dict(err='-2', msg=NO_LIST % (128, 64, 1, 1), row_list_supported='0')),
    ('list PP=0', conv(256, 64, 1, 'split', 'row_list=1', 'MILAN_PP=0'),
     dict(err='-2', msg=NO_LIST % (256, 64, 1, 1))),
    ('list fp32 out', conv(256, 64, 1, 'split', 'row_list=1', 'out_split=0'),
     dict(err='-2', msg=NO_LIST % (256, 64, 1, 1))),
    # (row_list_supported() refused every tile hint, MILAN_PP != 1 and, in the experiments
    # build, MILAN_SCHED / MILAN_CONV3X3 -- also where the launch would still reach the tile)
    ('list tile_hint', conv(256, 64, 1, 'split', 'row_list=1', 'tile_hint=10'),
     dict(err='-2', msg=NO_LIST % (256, 64, 1, 1))),
    ('list PP=3', conv(256, 64, 1, 'split', 'row_list=1', 'MILAN_PP=3'),
     dict(err='-2', msg=NO_LIST % (256, 64, 1, 1))),
    ('list SCHED', conv(256, 64, 1, 'split', 'row_list=1', 'experiments=1', 'MILAN_SCHED=1'),
     dict(err='-2', msg=NO_LIST % (256, 64, 1, 1))),
    # ---- grouped launches ----
    ('f32 groups N32 Cin12 5x5', (32, 12, 5, 5, 1, 2, 7, 8, 1, 'f32', 'groups=2'),
     dict(kernel=IG % '256, 64, 2, false, false, true', grid='1,2', launches='one')),
    ('f32 groups N64 Cin64', conv(64, 64, 3, 'f32', 'groups=2'),
     dict(kernel=IG % '256, 64, 2, true, false, true', grid='4,2', launches='one')),
    ('f32 groups N128 Cin12', conv(128, 12, 3, 'f32', 'groups=2'),
     dict(kernel=IG % '128, 128, 2, false, false, true', grid='7,2', launches='one')),
    # (groups_supported() answered for fp32 before it looked at the experiments build's knobs)
    ('f32 groups SCHED', conv(128, 64, 3, 'f32', 'groups=2', 'experiments=1', 'MILAN_SCHED=1'),
     dict(kernel=IG % '128, 128, 2, true, false, true', launches='one')),
    ('split groups SCHED', conv(128, 64, 3, 'split', 'groups=2', 'experiments=1', 'MILAN_SCHED=1'),
     dict(kernel=PP32N % 128, launches='per-group')),
    ('grouped 128', conv(128, 64, 3, 'split', 'groups=2'),
     dict(kernel='igemm_grouped_pp32n_kernel', grid='4,2', family='pp32_128', launches='one',
          tile='256x128')),
    ('grouped 128 Wt', conv(128, 64, 3, 'split', 'groups=2', 'Wt=1'),
     dict(kernel='igemm_grouped_pp32t_kernel', grid='72,2', family='pp32_128', launches='one',
          tap_inner='1', weights='Wt')),
    ('grouped 256', conv(256, 64, 3, 'split', 'groups=2'),
     dict(kernel='igemm_grouped_pp32n_kernel', grid='8,2', tile='256x128', launches='one')),
    ('grouped N64 3x3', conv(64, 64, 3, 'split', 'groups=2'),
     dict(kernel='igemm_split16_tm2_kernel<256, 64, 3, true>', grid='4,2', launches='one')),
    ('grouped N64 1x1', conv(64, 64, 1, 'split', 'groups=2'),
     dict(kernel=IG % '256, 64, 2, true, true', grid='4,1', launches='per-group')),
    ('grouped GROUP_LAUNCH=0', conv(128, 64, 3, 'split', 'groups=2', 'MILAN_GROUP_LAUNCH=0'),
     dict(kernel=PP32N % 128, grid='4,1', launches='per-group', family='pp32_128')),
    ('grouped PP128=0', conv(128, 64, 3, 'split', 'groups=2', 'MILAN_PP128=0'),
     dict(kernel=S16 % '256, 128, 3, 0', launches='per-group')),
    ('grouped tile_hint', conv(64, 64, 3, 'split', 'groups=2', 'tile_hint=6'),
     dict(kernel='igemm_split16_tm2_kernel<256, 64, 3>', launches='per-group')),
    # ---- epilogues ----
    ('lse', linear(5004, 512, 'split', 'out_split=0', 'epilogue=lse'),
     dict(kernel=PP32, out_mode='vec4')),
    ('lstm', linear(256, 512, 'split', 'out_split=0', 'epilogue=lstm'),
     dict(kernel=PP32, out_mode='vec4')),
    ('lse geometry', linear(5004, 512, 'split', 'out_split=0', 'epilogue=lse', 'ldc=7'),
     dict(err='-2', msg='gemm: bad log-sum-exp epilogue geometry (N=5004 ldc=7)')),
    ('lstm geometry', linear(256, 512, 'split', 'out_split=0', 'epilogue=lstm', 'ldc=60'),
     dict(err='-2', msg='gemm: bad LSTM epilogue geometry (N=256 ldc=60)')),
    ('res_relu split', conv(256, 64, 1, 'split', 'epilogue=res_relu'),
     dict(kernel=PP32, out_mode='split8')),
    ('two sources', conv(256, 64, 1, 'split', 'A2=64'), dict(kernel=PP32, grid='4,1')),
    ('two sources f32', conv(256, 64, 1, 'f32', 'A2=64'),
     dict(err='-2', msg='gemm: two-source A needs the split16 kernels')),
    ('fp32 scalar out', linear(30, 64, 'f32'), dict(kernel=IG % '256, 64, 2, true, false',
                                                    out_mode='scalar')),
]


@pytest.mark.parametrize('name,args,want', CASES, ids=[c[0] for c in CASES])
def test_plan_is_the_parents_dispatch(dump, name, args, want):
    got = dump(*args)
    assert {k: got.get(k) for k in want} == want, got


ROWS = (1, 255, 256, 257, 100000)
# The only kernel ids that may change with the row count, both documented as the same tile
# function in the same k order (the same bits): the persistent walk of the 1x1 loop variant
# once there are more tiles than CUs, and the MILAN_PP_PERSIST walk.
SAME_BITS = [{LINP, S16 % '256, 256, 5, 3'}, {PP32, PP32N % 256}]


def test_kernel_does_not_depend_on_rows(dump):
    for name, args, _ in CASES:
        plans = [dump(*args, 'M=%d' % m) for m in ROWS]
        for key in ('err', 'msg', 'tile', 'tap_inner', 'weights', 'out_mode', 'launches', 'family'):
            assert len({p.get(key) for p in plans}) == 1, (name, key, plans)
        kernels = {p.get('kernel') for p in plans}
        if len(kernels) > 1:
            assert kernels in SAME_BITS, (name, kernels)
            if kernels == SAME_BITS[1]:
                assert 'MILAN_PP_PERSIST=1' in args, name
            else:
                assert 'MILAN_PP=0' in args, name


def test_row_list_supported_is_the_list_form(dump):
    for name, args, _ in CASES:
        for m in ROWS:
            p = dump(*args, 'M=%d' % m)
            is_list = p.get('kernel', '').startswith('igemm_split16_pp32l_kernel')
            assert (p['row_list_supported'] == '1') == is_list, (name, p)
            if 'row_list=1' in args:
                assert is_list or p.get('msg', '').startswith('gemm: no row-list form'), (name, p)


def test_grouped_plan_and_its_groups_agree(dump):
    """the grouped launch and each group after shift_group run the same tile in the
    same k order (what makes the per-group baseline a bitwise reference)."""
    grouped = [(n, a) for n, a, _ in CASES if 'groups=2' in a]
    assert len(grouped) >= 8
    for name, args in grouped:
        for m in ROWS:
            whole = dump(*args, 'M=%d' % m)
            for q in (0, 1):
                part = dump(*args, 'M=%d' % m, 'shift_group=%d' % q)
                assert part['launches'] == 'one' and part['grid'].endswith(',1'), (name, part)
                for key in ('tile', 'tap_inner', 'weights', 'out_mode', 'family', 'threads', 'lds'):
                    assert whole[key] == part[key], (name, key, whole, part)
                if whole['launches'] == 'per-group':
                    assert whole['kernel'] == part['kernel'], (name, whole, part)
