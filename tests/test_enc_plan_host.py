"""The encoder schedule (csrc/enc_plan.h) against the driver it replaced.

tools/enc_plan_dump.cpp is compiled for the host (no GPU, no HIP) and asked for the schedule of
each case; the expected values were written by hand from the block loop of the
encoder_run_batch() that plan_encoder() replaced -- which `if` fires first for each block of
torchvision's trunks -- not printed by the new code.

Unless a case says otherwise: resnet50 at width 64, five 96 x 96 uint8 images with uint8 masks,
split_f16, every fusion bit on, default knobs, 256 CUs, product build.  Such a pass has levels
48, 24, 12, 6, 3; its mask-aware tail needs 9 * (2 * 2048 + 2048 + 11 * 512) = 105984 floats of
the raw conv1 tensor's 48 * 48 * 64 = 147456.
"""
import pathlib
import shutil
import subprocess

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
SRC = REPO / 'tools' / 'enc_plan_dump.cpp'


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    cxx = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path_factory.mktemp('enc_plan') / 'enc_plan_dump'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', str(SRC), '-o', str(exe)],
                   check=True)
    cache = {}

    def run(*args):
        key = tuple(str(a) for a in args)
        if key not in cache:
            out = subprocess.run([str(exe), *key], check=True, capture_output=True, text=True)
            cache[key] = parse(out.stdout)
        return cache[key]
    return run


def parse(text):
    """{'pass': {...}, 'blocks': [{...}], 'families': {...}, 'totals': {...}}"""
    sched = {'blocks': []}
    for line in text.splitlines():
        kind, *fields = line.split()
        if kind == 'families':
            sched['families'] = {f.split(':')[0]: int(f.split(':')[1]) for f in fields if ':' in f}
            sched['totals'] = {f.split('=')[0]: int(f.split('=')[1]) for f in fields if '=' in f}
            continue
        rec = dict(f.split('=', 1) for f in fields if '=' in f)
        if kind == 'block':
            rec['name'] = fields[0]
            sched['blocks'].append(rec)
        else:
            sched[kind] = rec
    return sched


def case(net='resnet50', width=64, n=5, h=96, w=96, prec='split', *opts):
    return (net, width, n, h, w, prec) + opts


def blocks(*stages):
    """'F' forms per stage, e.g. ('CHAIN_DS CHAIN_PLAIN*2', ...), '*k' repeats."""
    out = []
    for stage in stages:
        forms = []
        for word in stage.split():
            form, _, rep = word.partition('*')
            forms += [form] * int(rep or 1)
        out.append(forms)
    return out


# ---- what the parent's loop does with the width-64 bottleneck trunks, in split mode ----------
# layer1 (planes 64, 24 x 24 <= 56 wide): every block chains into the next one's c1 with its 3x3
# in front (MILAN_FUSE_BNECK); l1.0 has the stride-1 downsample (CHAIN_DS) and no t1 yet, so its
# c1 runs in the launch too; l1.2 chains across the stage boundary (NR = 128).
L1 = 'CHAIN_DS CHAIN_PLAIN*2'
# layer2 (planes 128): l2.0 has a stride-2 downsample -> no chain, [t2 | x] GEMM; l2.1, l2.2
# chain; l2.3 -> l3.0 would need NR = 256 = 2 P with P = 128: chain_supported says no -> PLAIN.
L2 = 'TWO_SOURCE CHAIN_PLAIN*2 PLAIN'
# layer3 (planes 256, MILAN_FUSE_CHAIN_WIDE): l3.0 as l2.0, l3.1 .. l3.(k-2) chain, the last
# block -> l4.0 would need P = 256 with NR = 512: no.
L3 = 'TWO_SOURCE CHAIN_PLAIN*4 %s'
# layer4 (planes 512: nothing chains)
L4_DENSE = 'TWO_SOURCE PLAIN*2'
L4_LISTS = 'LIST_FIRST TAIL_LISTS*2'
L4_COPY = 'TWO_SOURCE TAIL_COPY*2'
BASE = blocks(L1, L2, L3 % 'LIST_LAST3', L4_LISTS)
NO_TAIL = blocks(L1, L2, L3 % 'PLAIN', L4_DENSE)
COPIES = blocks(L1, L2, L3 % 'PLAIN', L4_COPY)
# dense or on lists a launch is of the same family (pp32l: tap-inner ? pp32t_256 : pp32_256):
# 1x1 convs with N % 256 == 0 -> pp32_256, 3x3 ones -> pp32t_256, N = 128 -> pp32_128
BASE_FAMILIES = dict(pp32_256=12, pp32_128=5, chain=2, chain_wide=4, stem=1, pp32t_256=9, bneck=3)
# (TAIL_COPY: the 3x3 is a Linear product over the im2col rows, K = 9 * 512 -> pp32_256)
COPY_FAMILIES = dict(BASE_FAMILIES, pp32_256=14, pp32t_256=7)
BASE_PASS = dict(split='1', fast='0', pair_stem='1', stem_u8='1', fused_stem='1',
                 compact='skip_empty', tail='1', lists='1', k0='2', lists_l3='1',
                 pool='f32,split8,split8,split8,split8', levels='48x48,24x24,12x12,6x6,3x3',
                 stem='stem')
NO_TAIL_PASS = dict(BASE_PASS, tail='0', lists='0', k0='-1', lists_l3='0')
# an fp32 pass (f32, calibration, or a trunk without split weight copies: width 8 / 16 has convs
# with Cin % 32 != 0): no fused launch, every bottleneck PLAIN with a downsample GEMM of its own
F32_PASS = dict(split='0', fast='0', pair_stem='0', stem_u8='0', fused_stem='0', tail='0',
                lists='0', k0='-1', lists_l3='0', pool='f32,f32,f32,f32,f32', stem='f32')
R50_PLAIN = blocks('PLAIN*3', 'PLAIN*4', 'PLAIN*6', 'PLAIN*3')
R18_BASIC = blocks('BASIC*2', 'BASIC*2', 'BASIC*2', 'BASIC*2')

# (name, arguments, pass fields, forms per stage, families or None, per-block fields)
CASES = [
    ('base', case(), BASE_PASS, BASE, BASE_FAMILIES,
     {'l1.0': dict(c1='fused', c2='none', conv_front='1', c1_front='1', NR='64'),
      'l1.1': dict(c1='ready', c2='none', conv_front='1', c1_front='0', NR='64'),
      'l1.2': dict(c1='ready', conv_front='1', NR='128'),
      'l2.0': dict(c1='ready', c2='gemm'), 'l2.1': dict(c1='launch', conv_front='0'),
      'l2.2': dict(c1='ready'), 'l2.3': dict(c1='ready'),
      'l3.0': dict(c1='launch'), 'l3.1': dict(c1='launch'), 'l3.2': dict(c1='ready'),
      'l3.5': dict(c1='ready', c2='list'),
      'l4.0': dict(c1='list', c2='list', kO='2'), 'l4.1': dict(kM='2', kO='1'),
      'l4.2': dict(kM='1', kO='0')}),
    ('tail_lists off', case('resnet50', 64, 5, 96, 96, 'split', 'tail_lists=0'),
     dict(BASE_PASS, lists='0', k0='-1', lists_l3='0'), COPIES, COPY_FAMILIES,
     {'l3.5': dict(c1='ready', c2='gemm'), 'l4.0': dict(c1='launch'),
      'l4.1': dict(kM='2', kO='1'), 'l4.2': dict(kM='1', kO='0')}),
    ('sparse_tail off', case('resnet50', 64, 5, 96, 96, 'split', 'sparse_tail=0'),
     NO_TAIL_PASS, NO_TAIL, BASE_FAMILIES, {}),
    # MILAN_FUSE_CHAIN off: layer1 / layer2 unchained -- l1.0 is TWO_SOURCE (c3d has 256 > 64
    # columns), layer1's 3x3 on conv3_p64; layer3 still chains
    ('chain off', case('resnet50', 64, 5, 96, 96, 'split', 'chain=0'), BASE_PASS,
     blocks('TWO_SOURCE PLAIN*2', 'TWO_SOURCE PLAIN*3', L3 % 'LIST_LAST3', L4_LISTS), None,
     {'l1.0': dict(c1='launch', c2='conv3'), 'l1.2': dict(c1='launch', c2='conv3'),
      'l2.0': dict(c1='launch', c2='gemm'), 'l3.1': dict(c1='launch'), 'l3.2': dict(c1='ready')}),
    # MILAN_FUSE_CHAIN_WIDE off: layer3 unchained, its last block's c1 is a launch of its own
    ('wide off', case('resnet50', 64, 5, 96, 96, 'split', 'wide=0'), BASE_PASS,
     blocks(L1, L2, 'TWO_SOURCE PLAIN*4 LIST_LAST3', L4_LISTS), None,
     {'l3.1': dict(c1='launch'), 'l3.5': dict(c1='launch', c2='list')}),
    # the pair stem's conv1 as a GEMM: Cin = 8, N = 64 -> the general split kernel
    ('stem off', case('resnet50', 64, 5, 96, 96, 'split', 'stem=0'),
     dict(BASE_PASS, stem_u8='0', fused_stem='0', stem='split_other'), BASE,
     dict({k: v for k, v in BASE_FAMILIES.items() if k != 'stem'}, split_other=1), {}),
    # conv3_p64 is used only where the 3x3 is not in front of a chain: nothing changes
    ('conv3 off', case('resnet50', 64, 5, 96, 96, 'split', 'conv3=0'), BASE_PASS, BASE,
     BASE_FAMILIES, {}),
    ('bneck off', case('resnet50', 64, 5, 96, 96, 'split', 'bneck=0'), BASE_PASS, BASE,
     dict({k: v for k, v in BASE_FAMILIES.items() if k != 'bneck'}, chain=5, conv3=3,
          split_other=1),   # (l1.0's c1: N = 64, 1x1 -> the general split kernel)
     {'l1.0': dict(c1='launch', c2='conv3', conv_front='0', c1_front='0'),
      'l1.1': dict(c1='ready', c2='conv3'), 'l1.2': dict(c2='conv3', NR='128')}),
    ('bneck and conv3 off', case('resnet50', 64, 5, 96, 96, 'split', 'bneck=0', 'conv3=0'),
     BASE_PASS, BASE, None, {'l1.0': dict(c2='gemm'), 'l1.1': dict(c2='gemm')}),
    ('skip_empty off', case('resnet50', 64, 5, 96, 96, 'split', 'skip_empty=0'),
     dict(BASE_PASS, compact='none'), BASE, BASE_FAMILIES, {}),
    # no masks: nothing to compact and no pixel lists to build the tail's sets from
    ('no masks', case('resnet50', 64, 5, 96, 96, 'split', 'masks=none'),
     dict(NO_TAIL_PASS, compact='none'), NO_TAIL, BASE_FAMILIES, {}),
    ('float masks', case('resnet50', 64, 5, 96, 96, 'split', 'masks=f32'), BASE_PASS, BASE,
     BASE_FAMILIES, {}),
    # float images: may hold NaN pixels -> no compaction; the stem reads the pixel-pair tensor
    ('float images', case('resnet50', 64, 5, 96, 96, 'split', 'images=f32'),
     dict(BASE_PASS, stem_u8='0', compact='none'), BASE, BASE_FAMILIES, {}),
    ('unaligned images', case('resnet50', 64, 5, 96, 96, 'split', 'aligned=0'),
     dict(BASE_PASS, stem_u8='0'), BASE, BASE_FAMILIES, {}),
    ('sharing', case('resnet50', 64, 5, 96, 96, 'split', 'share=1'),
     dict(BASE_PASS, compact='classes'), BASE, BASE_FAMILIES, {}),
    # milan_encoder_absmax: an fp32 pass over every image; 16 blocks x 3 convs + 4 downsamples
    # + conv1
    ('calibration', case('resnet50', 64, 5, 96, 96, 'split', 'calib=1'),
     dict(F32_PASS, compact='none'), R50_PLAIN, dict(f32=53), {'l1.0': dict(c1='launch', c2='gemm')}),
    ('f32', case('resnet50', 64, 5, 96, 96, 'f32'), dict(F32_PASS, compact='skip_empty'),
     R50_PLAIN, dict(f32=53), {}),
    # spatial: no pooling, so no lists, no compaction; the mask multiplies the pixels, which the
    # uint8 stem does not do
    ('spatial', case('resnet50', 64, 5, 96, 96, 'split', 'spatial=1'),
     dict(NO_TAIL_PASS, compact='none', stem_u8='0'), NO_TAIL, BASE_FAMILIES, {}),
    # fast mode: stages 3-4 on plain f16, no tail; l2.3 may not chain across into an f16 stage
    ('f16', case('resnet50', 64, 5, 96, 96, 'f16'),
     dict(NO_TAIL_PASS, fast='1', pool='f32,split8,split8,f16,f16'),
     blocks(L1, L2, 'F16*6', 'F16*3'), None, {'l2.3': dict(c1='ready'), 'l3.0': dict(c1='launch')}),
    ('resnet101', case('resnet101', 64, 5, 96, 96), BASE_PASS,
     blocks(L1, L2, 'TWO_SOURCE CHAIN_PLAIN*21 LIST_LAST3', L4_LISTS), None,
     {'l3.22': dict(c1='ready', c2='list')}),
    ('resnet101 copies', case('resnet101', 64, 5, 96, 96, 'split', 'tail_lists=0'),
     dict(BASE_PASS, lists='0', k0='-1', lists_l3='0'),
     blocks(L1, L2, 'TWO_SOURCE CHAIN_PLAIN*21 PLAIN', L4_COPY), None, {}),
    # 224 x 224: layer1 is 56 wide, the widest the 3x3 front takes; the tail needs 49 * 11776 =
    # 577024 floats of 112 * 112 * 64
    ('224', case('resnet50', 64, 2, 224, 224),
     dict(BASE_PASS, levels='112x112,56x56,28x28,14x14,7x7'), BASE, BASE_FAMILIES,
     {'l1.0': dict(conv_front='1', c1_front='1')}),
    ('resnet101 224', case('resnet101', 64, 2, 224, 224),
     dict(BASE_PASS, levels='112x112,56x56,28x28,14x14,7x7'),
     blocks(L1, L2, 'TWO_SOURCE CHAIN_PLAIN*21 LIST_LAST3', L4_LISTS), None, {}),
    # 232 wide: layer1 is 58 > 56 wide -- the chain runs without the 3x3 in front
    ('232 wide', case('resnet50', 64, 2, 64, 232),
     dict(BASE_PASS, levels='32x116,16x58,8x29,4x15,2x8'), BASE, None,
     {'l1.0': dict(c1='launch', c2='conv3', conv_front='0'), 'l1.1': dict(c1='ready', c2='conv3')}),
    # 32 x 32: levels 16, 8, 4, 2, 1 -- the tail still fits (11776 of 16 * 16 * 64 = 16384)
    ('32', case('resnet50', 64, 5, 32, 32), dict(BASE_PASS, levels='16x16,8x8,4x4,2x2,1x1'),
     BASE, BASE_FAMILIES, {}),
    # 8 x 8: levels 4, 2, 1, 1, 1 -- it does not (11776 > 4 * 4 * 64)
    ('8', case('resnet50', 64, 5, 8, 8), dict(NO_TAIL_PASS, levels='4x4,2x2,1x1,1x1,1x1'),
     NO_TAIL, BASE_FAMILIES, {}),
    # W % 4 != 0: the uint8 stem reads whole words of a row
    ('W 94', case('resnet50', 64, 5, 96, 94),
     dict(BASE_PASS, stem_u8='0', levels='48x47,24x24,12x12,6x6,3x3'), BASE, BASE_FAMILIES, {}),
    ('MILAN_STEM_U8=0', case('resnet50', 64, 5, 96, 96, 'split', 'MILAN_STEM_U8=0'),
     dict(BASE_PASS, stem_u8='0'), BASE, BASE_FAMILIES, {}),
    ('MILAN_POOL_VEC=0', case('resnet50', 64, 5, 96, 96, 'split', 'MILAN_POOL_VEC=0'),
     dict(BASE_PASS, pool='f32,split,split,split,split'), BASE, BASE_FAMILIES, {}),
    # MILAN_PP=0: no pair-staged 256-column tile, so no list form: copies, and k0 stays -1
    ('MILAN_PP=0', case('resnet50', 64, 5, 96, 96, 'split', 'MILAN_PP=0'),
     dict(BASE_PASS, k0='-1', lists_l3='0'), COPIES, None, {}),
    # width 8 / 16: convs with Cin % 32 != 0 have no split copy -> the whole pass is fp32
    ('resnet50 w16', case('resnet50', 16, 5, 96, 96), dict(F32_PASS, compact='skip_empty'),
     R50_PLAIN, dict(f32=53), {'l2.0': dict(c1='launch', c2='gemm')}),
    ('resnet50 w16 f32', case('resnet50', 16, 5, 96, 96, 'f32'),
     dict(F32_PASS, compact='skip_empty'), R50_PLAIN, dict(f32=53), {}),
    ('resnet50 w8', case('resnet50', 8, 5, 96, 96), dict(F32_PASS, compact='skip_empty'),
     R50_PLAIN, dict(f32=53), {}),
    # 8 BasicBlocks x 2 convs + 3 downsamples + conv1
    ('resnet18 w16', case('resnet18', 16, 5, 96, 96), dict(F32_PASS, compact='skip_empty'),
     R18_BASIC, dict(f32=20), {}),
    ('resnet18 w16 f32', case('resnet18', 16, 5, 96, 96, 'f32'),
     dict(F32_PASS, compact='skip_empty'), R18_BASIC, dict(f32=20), {}),
    ('resnet18 w8 no masks', case('resnet18', 8, 5, 96, 96, 'split', 'masks=none'),
     dict(F32_PASS, compact='none'), R18_BASIC, dict(f32=20), {}),
    # resnet18 at width 64 has split copies everywhere: BasicBlocks on the split kernels, the
    # fused stem, no chain, no tail (bottleneck trunks only)
    ('resnet18 w64', case('resnet18', 64, 5, 96, 96),
     dict(NO_TAIL_PASS, pool='f32,split8,split8,split8,split8'), R18_BASIC, None, {}),
]
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize('name,args,pass_,forms,families,fields', CASES, ids=IDS)
def test_schedule(dump, name, args, pass_, forms, families, fields):
    sched = dump(*args)
    got = {k: sched['pass'].get(k) for k in pass_}
    assert got == pass_
    by_stage = [[b['form'] for b in sched['blocks'] if b['name'].startswith('l%d.' % (li + 1))]
                for li in range(4)]
    assert by_stage == forms
    if families is not None:
        assert sched['families'] == families
    by_name = {b['name']: b for b in sched['blocks']}
    for block, want in fields.items():
        assert {k: by_name[block][k] for k in want} == want, block


def test_known_line_counts(dump):
    """26 launch_gemm calls, 11 of them on row lists (profiles/gemm_plan.txt)."""
    totals = dump(*case())['totals']
    assert totals['launch_gemm'] == 26 and totals['on_lists'] == 11
    assert dump(*case('resnet50', 64, 5, 96, 96, 'split', 'tail_lists=0'))['totals']['on_lists'] == 0


FORMS = {'F16', 'TAIL_LISTS', 'TAIL_COPY', 'BASIC', 'LIST_FIRST', 'LIST_LAST3', 'CHAIN_PLAIN',
         'CHAIN_DS', 'TWO_SOURCE', 'PLAIN'}


@pytest.mark.parametrize('args', [c[1] for c in CASES], ids=IDS)
def test_properties(dump, args):
    sched = dump(*args)
    depth = {'resnet18': 8, 'resnet50': 16, 'resnet101': 33}[args[0]]
    assert len(sched['blocks']) == depth
    lines = 1   # the stem
    for b in sched['blocks']:
        assert b['form'] in FORMS              # exactly one form, and a named one
        assert b['alias'] == '0', b['name']    # no launch writes a buffer it reads
        assert b['x'] != b['y']
        lines += len(b['launches'].split(','))
        # a list launch only in a list form, and every launch of a tail-list block is one
        on_list = [l.endswith('@list') for l in b['launches'].split(',')]
        assert any(on_list) == (b['form'] in ('TAIL_LISTS', 'LIST_FIRST', 'LIST_LAST3')), b['name']
        if b['form'] == 'TAIL_LISTS':
            assert all(on_list)
    assert sum(sched['families'].values()) == lines == sched['totals']['total']
    assert sched['totals']['block_launches'] == lines - 1
