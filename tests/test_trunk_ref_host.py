"""The float64 yardstick of tests/test_gpu_full_width.py, checked on the host (tests/trunkref.py).

Three things make a comparison with `encode64` at FEATURE_CLASS mean something:

* the restated trunk IS the oracle's trunk (`torch.equal` on float64 inputs);
* conditioning: on every case the GPU file runs, the fp32 CPU oracle -- a correct fp32
  implementation -- stays within FEATURE_CLASS / 4 of it, so a failure at FEATURE_CLASS is not the
  case's own ill-conditioning;
* sensitivity: each bug of the kind the GPU file is for, applied to the reference through its
  hook on a case of the GPU matrix, moves the features by more than FEATURE_CLASS.

The scale is the per-level maximum over the whole batch (`featclass.feature_error`).  A per-row
scale does not hold up: the fp32 oracle alone reaches 1.2e-5 of a row's own maximum (corner masks
at 97 x 131).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunkref as R
from featclass import FEATURE_CLASS, feature_error
from milan_amd import synthetic
from oracle import milan_oracle as O

BLOCKS = synthetic.RESNET_BLOCKS['resnet50']


@pytest.fixture(scope='module')
def sd():
    return synthetic.resnet_state_dict('resnet50', seed=3, width=R.WIDTH, prefix=R.PREFIX)


@pytest.fixture(scope='module')
def sd64(sd):
    return R.double_state(sd)


def test_the_case_table_is_what_it_says():
    """Every row count the table claims belongs to a geometry where the host's condition lets the
    tail run (`trunkref.tail_runs` restates csrc/encoder.hip) -- elsewhere no list is built."""
    assert len(R.GEOMETRIES) == 10 and set(R.BATCHES) == set(R.GEOMETRIES)
    for (h, w), n in R.BATCHES.items():
        assert n * h * w <= 9 * 240 * 240 and max(h, w) <= 300
    # the extra cases keep the pixel budget; the two single images whose level 3 has 255 / 256
    # pixels are the only ones above 240 pixels on a side (272 and 256)
    for (h, w), n, _ in R.EXTRA_CASES:
        assert n * h * w <= 9 * 240 * 240 and (max(h, w) <= 240 or n == 1 and max(h, w) <= 272)
    assert [g for g in R.GEOMETRIES if R.tail_runs(*g)] == [(224, 224), (200, 150), (150, 200), (64, 232)]
    # 11776 floats per level-4 pixel against 64 h1 w1: the reviewer's arithmetic, as a check of the restatement
    assert not R.tail_runs(20, 20) and not R.tail_runs(97, 131) and R.tail_runs(32, 32)
    lengths3, lengths4 = set(), set()
    for (h, w), n, kind, rows3, rows4 in R.LIST_CASES:
        assert R.tail_runs(h, w) and kind == 'full'
        sizes = R.level_sizes(h, w)
        assert (rows3, rows4) == (n * sizes[3][0] * sizes[3][1], n * sizes[4][0] * sizes[4][1])
        assert (h, w, n, kind) in R.matrix_cases()
        lengths3.add(rows3)
        lengths4.add(rows4)
    assert {1, 255, 256, 257} <= lengths4 and {255, 256, 1020, 1024, 1028} <= lengths3
    for h, w, _ in R.DUPLICATE_CASES:
        assert R.tail_runs(h, w) and h != w
    assert R.tail_runs(*R.DESCRIBE_CASE[:2])
    assert R.level_sizes(64, 232)[1] == (16, 58) and R.level_sizes(20, 52)[4] == (1, 2)
    assert R.level_sizes(4, 300)[4] == (1, 10) and R.level_sizes(7, 9)[2:] == [(1, 2), (1, 1), (1, 1)]
    assert len(R.matrix_cases()) == len(R.GEOMETRIES) * len(R.KINDS) + len(R.EXTRA_CASES)


def _resize_weights(size_in, size_out, fused):
    """(size_in, size_out) float32: column o = the weights of the source pixels in target pixel o
    of a bilinear resize (align_corners=False), the source coordinate rounded once (`fused`: a
    fused multiply-add, exact in float64 and rounded) or after the product and after the sum."""
    f = np.float32
    scale = f(size_in) / f(size_out)
    out = np.zeros((size_in, size_out), f)
    for o in range(size_out):
        at = f(o) + f(0.5)
        c = f(np.float64(at) * np.float64(scale) - 0.5) if fused else at * scale - f(0.5)
        c = max(c, f(0))
        i0 = int(c)
        i1 = i0 + (1 if i0 < size_in - 1 else 0)
        l1 = f(c - f(i0))
        out[i0, o] += f(1) - l1
        out[i1, o] += l1
    return out


def test_the_mask_resize_rounds_its_source_coordinate_once():
    """`mask_pyramid_kernel` (csrc/encoder.hip) takes the source coordinate with one fmaf.  That
    form reproduces torch's resize bit for bit at every halving of 1..240; rounded twice, as the
    kernel did before, it is one ulp of the coordinate off at 48 of them, by up to 7.6e-6 in a
    weight (131 -> 66), and at none whose scale is a power of two.

    This pins the torch build as well as the kernel's formula: `F.interpolate` on the CPU rounds
    the coordinate once because torch's kernels are compiled with floating-point contraction.  On
    a torch built without it the two-rounding form would be the exact one, and the counts below
    (48 sizes, worst at 131, 2^-17) would fail here before any GPU test does -- that is the
    signal to revisit the kernel's `fmaf`, not a defect of this test."""
    off = {}
    for size in list(range(1, 241)) + [272, 300]:
        eye = torch.eye(size).view(1, size, size, 1)   # channel r: only source row r is set
        for level, (out, _) in enumerate(R.level_sizes(size, size)):   # the pyramid resizes size -> out
            ref = F.interpolate(eye, size=(out, 1), mode='bilinear', align_corners=False)[0, :, :, 0].numpy()
            assert np.array_equal(_resize_weights(size, out, True), ref), (size, out)
            d = float(np.abs(_resize_weights(size, out, False) - ref).max())
            if level == 0 and d and size <= 240:
                off[size] = d
            if size in (224, 96, 64):   # power-of-two scales: both forms are exact
                assert d == 0
    assert len(off) == 48 and max(off, key=off.get) == 131 and off[131] == 2.0**-17
    assert not any(size & (size - 1) == 0 for size in off) and 224 not in off and 96 not in off


def test_mask_kinds():
    g = torch.Generator().manual_seed(1)
    h, w = 11, 14
    assert R.masks_of('none', 3, h, w, g) is None
    assert bool((R.masks_of('full', 3, h, w, g) == 1).all())
    pixel = R.masks_of('pixel', 8, h, w, g)
    assert pixel.flatten(1).sum(1).tolist() == [1] * 8
    assert pixel[0, 0, 0, 0] == 1 and pixel[2, 0, -1, -1] == 1 and pixel[4, 0, 0, 0] == 1
    assert int(R.masks_of('corners', 2, h, w, g).sum()) == 8
    ring = R.masks_of('ring', 1, h, w, g)[0, 0]
    assert int(ring.sum()) == 2 * (h + w) - 4 and int(ring[1:-1, 1:-1].sum()) == 0
    assert R.masks_of('rowcol', 5, h, w, g).flatten(1).sum(1).tolist() == [h + w - 1] * 5
    soft = R.masks_of('soft', 4, 64, 64, g)
    assert soft.dtype == torch.float32 and 0 < float((soft > 0).float().mean()) < 0.2
    assert 0 < float(soft[soft > 0].min()) and float(soft.max()) < 1
    sparse = R.masks_of('sparse', 4, 100, 100, g)
    assert sparse.dtype == torch.uint8 and 0 < int(sparse.sum()) < 0.01 * sparse.numel()
    mixed = R.masks_of('mixed', 6, h, w, g).flatten(1).sum(1)
    assert mixed[0] == 0 and 0 < mixed[1] < h * w and mixed[2] == h * w and mixed[3] == 0
    # every kind survives the one-pixel image
    for kind in R.KINDS:
        R.masks_of(kind, 3, 1, 1, g)


@pytest.mark.parametrize('hw', [(64, 64), (33, 47), (7, 9), (1, 1)])
def test_the_restated_trunk_is_the_oracles(sd64, hw):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64)
    with torch.no_grad():
        mine = R.resnet_trunk(x, sd64, blocks=BLOCKS)
        theirs = O.resnet_trunk(x, sd64, blocks=BLOCKS)
    assert [tuple(t.shape[-2:]) for t in mine] == R.level_sizes(*hw)
    for a, b in zip(mine, theirs):
        assert a.dtype == torch.float64 and torch.equal(a, b)


def test_encode64_is_the_oracle_in_float64(sd, sd64):
    """At 64 x 64 every level's scale factor is a power of two: the float32 resize of a binary
    mask is exact, so `encode64` and the oracle's own `encode` run entirely in float64 differ by
    the order of float64 sums at most."""
    images, masks = R.make_case(64, 64, 3, 'mixed')
    got = R.encode64(images, masks, sd, BLOCKS)
    assert got.dtype == torch.float64 and got.shape == (3, 61 * R.WIDTH)
    sd_all = dict(sd64)
    with torch.no_grad():
        want = O.encode(O.byte_to_float(images).double()[None], masks.double()[None], sd_all,
                        blocks=BLOCKS)[0]
    # encode() falls back to float32 mean / std tensors: promoted, the same values
    assert feature_error(got, want, family='bottleneck')[0] < 1e-13
    assert bool((got[0] == 0).all()) and float(got[1].abs().max()) > 0


def _condition(case, sd, float_images=False):
    images, masks = R.make_case(*case, float_images=float_images)
    want = R.encode64(images, masks, sd, BLOCKS)
    worst, where = feature_error(R.encode32(images, masks, sd, BLOCKS), want, family='bottleneck')
    return worst, where, want


@pytest.mark.parametrize('case', R.matrix_cases(), ids=R.case_id)
def test_conditioning_of_the_matrix(sd, case):
    worst, where, _ = _condition(case, sd)
    print(R.case_id(case), f'fp32 oracle against float64: {worst:.2e}')
    assert worst <= FEATURE_CLASS / 4, (worst, where)


def test_conditioning_of_the_float_image_case(sd):
    worst, where, _ = _condition(R.FLOAT_CASE, sd, float_images=True)
    assert worst <= FEATURE_CLASS / 4, (worst, where)


@pytest.mark.parametrize('case', R.CASES_101, ids=R.case_id)
def test_conditioning_of_the_resnet101_cases(case):
    sd101 = synthetic.resnet_state_dict('resnet101', seed=3, width=R.WIDTH, prefix=R.PREFIX)
    images, masks = R.make_case(*case)
    blocks = synthetic.RESNET_BLOCKS['resnet101']
    want = R.encode64(images, masks, sd101, blocks)
    worst, where = feature_error(R.encode32(images, masks, sd101, blocks), want, family='bottleneck')
    print(R.case_id(case), f'resnet101 fp32 oracle against float64: {worst:.2e}')
    assert worst <= FEATURE_CLASS / 4, (worst, where)


def test_conditioning_of_the_describe_case():
    sd = R.describe_state_dict()
    worst, where, _ = _condition(R.DESCRIBE_CASE, sd)
    assert worst <= FEATURE_CLASS / 4, (worst, where)


@pytest.mark.parametrize('case', R.DUPLICATE_CASES, ids=lambda c: f'{c[0]}x{c[1]}')
def test_conditioning_of_the_duplicate_cases(sd, case):
    images, masks = R.duplicate_case(*case)
    want = R.encode64(images, masks, sd, BLOCKS)
    worst, where = feature_error(R.encode32(images, masks, sd, BLOCKS), want, family='bottleneck')
    assert worst <= FEATURE_CLASS / 4, (worst, where)
    assert bool((want[0] == 0).all()) and bool((want[-1] == 0).all())
    # slots of one image under different masks do differ
    which = case[2]
    twin = [i for i in range(1, len(which) - 1) if which[i] == which[0]][0]
    assert float(want[twin].abs().max()) > 0


# mutant, the matrix case it is shown on, hook
MUTANTS = [
    ('a3: level-3 pooling drops its lightest pixel', (200, 150, 2, 'soft'), R.drop_lightest_pixel(3)),
    ('a4: level-4 pooling drops its lightest pixel', (200, 150, 2, 'soft'), R.drop_lightest_pixel(4)),
    ('a4: the same with two-valued weights', (97, 131, 4, 'rowcol'), R.drop_lightest_pixel(4)),
    ('b1: layer1.0.conv2 skips an inside tap at a corner', (20, 52, 32, 'rowcol'),
     R.skip_inside_tap('layer1.0.conv2')),
    ('b1: the same under full masks at 224', (224, 224, 2, 'full'), R.skip_inside_tap('layer1.0.conv2')),
    ('b1: layer1.0.conv2 reads an outside tap at a corner', (64, 232, 4, 'full'),
     R.outside_tap_as_inside('layer1.0.conv2')),
    ('b4: layer4.0.conv2 skips an inside tap at a corner', (200, 150, 2, 'full'),
     R.skip_inside_tap('layer4.0.conv2')),
    ('b4: layer4.0.conv2 reads an outside tap at a corner', (150, 200, 3, 'soft'),
     R.outside_tap_as_inside('layer4.0.conv2')),
    ('c: h and w swapped in the level-4 resize', (200, 150, 2, 'rowcol'), R.swapped_resize(4)),
    ('c: the same on the transpose', (150, 200, 3, 'soft'), R.swapped_resize(4)),
    ('e: layer4.0 reads its stride-2 set one column off', (150, 200, 3, 'full'),
     R.shifted_stride2_set('layer4.0')),
    ('e: the same under sparse weights', (97, 131, 4, 'soft'), R.shifted_stride2_set('layer4.0')),
]


@pytest.mark.parametrize('name,case,hook', MUTANTS, ids=[m[0].split(':')[0] + '-' + R.case_id(m[1])
                                                         for m in MUTANTS])
def test_the_yardstick_resolves_the_mutant(sd64, name, case, hook):
    assert case in R.matrix_cases()
    images, masks = R.make_case(*case)
    want = R.encode64(images, masks, sd64, BLOCKS)
    mutant = R.encode64(images, masks, sd64, BLOCKS, hook=hook)
    worst, where = feature_error(mutant, want, family='bottleneck')
    print(f'{name} | {R.case_id(case)} | {worst:.2e}')
    assert worst > FEATURE_CLASS, (name, worst, where)


def test_the_yardstick_resolves_a_siblings_mask(sd64):
    """(d) on a case of test_shared_duplicates_match_float64: slot 2 shows the image of slot 0."""
    case = R.DUPLICATE_CASES[0]
    images, masks = R.duplicate_case(*case)
    assert torch.equal(images[2], images[0]) and not torch.equal(masks[2], masks[0])
    want = R.encode64(images, masks, sd64, BLOCKS)
    for slot, sibling in ((2, 5), (5, 2), (2, 0)):
        mutant = R.encode64(images, masks, sd64, BLOCKS, hook=R.sibling_mask(slot, sibling))
        worst, where = feature_error(mutant, want, family='bottleneck')
        print(f'd: slot {slot} pooled with the mask of slot {sibling} | '
              f'{case[0]}x{case[1]} duplicates | {worst:.2e}')
        assert worst > FEATURE_CLASS, (slot, sibling, worst, where)


def test_fuzz_draws_are_well_conditioned(sd):
    """The share of the default 24 draws that the conditioning rule would skip: none."""
    sizes = set()
    for seed in range(24):
        p, images, masks = R.fuzz_case(seed)
        sizes.add((p['h'] <= 12, p['w'] <= 12))
        want = R.encode64(images, masks, sd, BLOCKS)
        worst, where = feature_error(R.encode32(images, masks, sd, BLOCKS), want, family='bottleneck')
        assert worst <= FEATURE_CLASS / 4, (seed, p, worst, where)
    assert len(sizes) == 4, sizes
