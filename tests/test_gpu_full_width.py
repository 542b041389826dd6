"""The production trunk -- bottleneck, width 64, where the hand-scheduled kernels run -- against
the float64 reference of tests/trunkref.py, off the square path: non-square and odd geometries,
border-concentrated, sparse, soft, empty and missing masks, duplicate images with sharing, and --
at geometries where the host lets the mask-aware tail run (`trunkref.tail_runs`) -- batches that
put its row lists at 1 / 255 / 256 / 257 rows (S0) and 255 / 256 / 1020 / 1024 / 1028 rows (V, W).

The bound is the suite's FEATURE_CLASS (tests/featclass.py: per pyramid level, against the level's
maximum over the batch; rows that are exactly zero in float64 must be exactly zero).
tests/test_trunk_ref_host.py shows on the host that every case here is conditioned for it (the
fp32 CPU oracle stays within a quarter of the bound) and that the bound resolves the bugs this
file is for (a dropped list pixel, a wrong border tap, swapped h / w, a sibling's mask, a shifted
stride-2 set).  Every other schedule must then give the bits of the default one.
"""
import os

import pytest
import torch

import trunkref as R
from featclass import FEATURE_CLASS, feature_error
from milan_amd import hip, synthetic

pytestmark = pytest.mark.gpu
PRECISIONS = ['split_f16', 'f32']

# (arch, (h, w, n, kind), float images)
MATRIX = ([('resnet50', case, False) for case in R.matrix_cases()] +
          [('resnet50', R.FLOAT_CASE, True)] +
          [('resnet101', case, False) for case in R.CASES_101])


def _id(entry):
    arch, case, as_float = entry
    return ('' if arch == 'resnet50' else arch + '-') + R.case_id(case) + ('-float' if as_float else '')


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


@pytest.fixture(scope='module')
def trunks(dev):
    """One full-width context (and its state dict) per architecture; closed at teardown."""
    made = {}

    def get(arch):
        if arch not in made:
            sd = synthetic.resnet_state_dict(arch, seed=3, width=R.WIDTH, prefix=R.PREFIX)
            ctx = hip.Context(hip.make_dims(sd, 10, blocks=synthetic.RESNET_BLOCKS[arch]), sd, dev)
            made[arch] = (ctx, sd, R.double_state(sd))
        return made[arch]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


_REFERENCE = {}


def reference(trunks, entry):
    """inputs and float64 features of a matrix entry: computed once, shared, never modified"""
    if entry not in _REFERENCE:
        arch, case, as_float = entry
        images, masks = R.make_case(*case, float_images=as_float)
        want = R.encode64(images, masks, trunks(arch)[2], synthetic.RESNET_BLOCKS[arch])
        _REFERENCE[entry] = (images, masks, want)
    return _REFERENCE[entry]


def check(ctx, got, want, what):
    assert ctx.status() == 0, what
    worst, where = feature_error(got, want, family='bottleneck')
    print(f'FW {what} {worst:.3e} = {worst / FEATURE_CLASS:.3f} x bound')
    assert worst <= FEATURE_CLASS, (what, worst, where)
    return worst


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('entry', MATRIX, ids=_id)
def test_matrix_matches_float64(trunks, entry, precision):
    ctx = trunks(entry[0])[0]
    images, masks, want = reference(trunks, entry)
    ctx.set_precision(precision)
    ctx.set_fusion()
    got = ctx.encode(images, masks)
    check(ctx, got, want, f'{_id(entry)} {precision}')


SCHEDULES = [
    dict(chain=False), dict(bneck=False), dict(conv3=False), dict(stem=False),
    dict(sparse_tail=False), dict(sparse_tail=True, tail_lists=False), dict(skip_empty=False),
]


def live_classes(images, masks):
    """classes of byte-identical images with work: a class is live if a member's mask is not
    empty (every class without masks)"""
    live = {}
    for i, image in enumerate(images):
        key = image.numpy().tobytes()
        live[key] = live.get(key, False) or masks is None or bool(masks[i].any())
    return sum(live.values())


# the matrix, and the duplicate cases: there sharing has something to share
SCHEDULE_ENTRIES = MATRIX + [('resnet50', case, 'duplicates') for case in R.DUPLICATE_CASES]


def _schedule_id(entry):
    return f'duplicates-{entry[1][0]}x{entry[1][1]}' if entry[2] == 'duplicates' else _id(entry)


@pytest.mark.parametrize('entry', SCHEDULE_ENTRIES, ids=_schedule_id)
def test_every_schedule_has_the_bits_of_the_default(trunks, entry):
    """... and with image sharing on, the counters say that the trunk ran once per live class
    (float images take the full pass: one trunk image per slot)."""
    ctx = trunks(entry[0])[0]
    if entry[2] == 'duplicates':
        host_images, host_masks = R.duplicate_case(*entry[1])
    else:
        host_images, host_masks = R.make_case(*entry[1], float_images=entry[2])
    expect = (len(host_images) if host_images.dtype != torch.uint8
              else live_classes(host_images, host_masks))
    if entry[2] == 'duplicates':
        assert expect < len(host_images)
    images = host_images.cuda()
    masks = None if host_masks is None else host_masks.cuda()
    ctx.set_precision('split_f16')
    ctx.set_fusion()
    ctx.set_image_sharing(False)
    want = ctx.encode(images, masks).clone()
    assert ctx.status() == 0
    try:
        for schedule in SCHEDULES:
            ctx.set_fusion(**schedule)
            got = ctx.encode(images, masks)
            assert ctx.status() == 0, schedule
            assert torch.equal(got, want), schedule
        ctx.set_fusion()
        ctx.set_image_sharing(True)
        ctx.image_sharing_stats(clear=True)
        got = ctx.encode(images, masks)
        stats = ctx.image_sharing_stats(clear=True)
        assert ctx.status() == 0, 'sharing'
        assert torch.equal(got, want), 'sharing'
        assert stats == (len(images), expect), stats
    finally:
        ctx.set_fusion()
        ctx.set_image_sharing(False)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', R.DUPLICATE_CASES, ids=lambda c: f'{c[0]}x{c[1]}')
def test_shared_duplicates_match_float64(trunks, case, precision):
    """Slots that show one image under different masks, the class root and one more slot with an
    empty mask, sharing and the row lists on, at geometries where the tail runs (the unioned
    level-3 / level-4 lists; `trunkref.tail_runs`, asserted on the host): against the float64
    features of the batch as it stands, every slot on its own."""
    ctx, _, sd64 = trunks('resnet50')
    images, masks = R.duplicate_case(*case)
    want = R.encode64(images, masks, sd64, synthetic.RESNET_BLOCKS['resnet50'])
    ctx.set_precision(precision)
    ctx.set_fusion(sparse_tail=True, tail_lists=True)
    ctx.set_image_sharing(True)
    try:
        ctx.image_sharing_stats(clear=True)
        got = ctx.encode(images, masks)
        stats = ctx.image_sharing_stats(clear=True)
        check(ctx, got, want, f'duplicates {case[0]}x{case[1]} {precision}')
        assert stats == (len(images), live_classes(images, masks)), stats
    finally:
        ctx.set_fusion()
        ctx.set_image_sharing(False)
    assert bool((got[0] == 0).all()) and bool((got[-1] == 0).all())


# MILAN_FUZZ_SEEDS=<n> widens the campaign
N_SEEDS = int(os.environ.get('MILAN_FUZZ_SEEDS', '24'))
_FUZZ = {}


def run_fuzz(trunks, seed):
    """-> True when the draw was compared, False when the fp32 CPU oracle itself is not within
    FEATURE_CLASS / 4 of float64 on it (the draw is then no evidence either way)."""
    if seed not in _FUZZ:
        ctx, sd, sd64 = trunks('resnet50')
        blocks = synthetic.RESNET_BLOCKS['resnet50']
        p, images, masks = R.fuzz_case(seed)
        want = R.encode64(images, masks, sd64, blocks)
        alone32 = R.encode32(images, masks, sd, blocks)
        if bool(((want == 0) & (alone32 != 0)).any()):  # fp32 is not zero where float64 is
            alone = float('inf')
        else:
            alone = feature_error(alone32, want, family='bottleneck')[0]
        if alone > FEATURE_CLASS / 4:
            print('FW fuzz', seed, p, 'skipped: fp32 oracle at', alone)
            _FUZZ[seed] = False
            return False
        _FUZZ[seed] = True  # (compared; a failure below is the test's)
        ctx.set_precision(p['precision'])
        ctx.set_fusion()
        ctx.set_image_sharing(p['duplicates'] != 'none')
        try:
            got = ctx.encode(images, masks)
            check(ctx, got, want, f'fuzz {seed} {p}')
        finally:
            ctx.set_image_sharing(False)
    return _FUZZ[seed]


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_fuzz_full_width(trunks, seed):
    run_fuzz(trunks, seed)


def test_fuzz_covers_both_size_ranges_and_skips_at_most_a_tenth(trunks):
    draws = [R.draw_fuzz(seed) for seed in range(N_SEEDS)]
    assert {(p['h'] <= 12, p['w'] <= 12) for p in draws} == {(a, b) for a in (False, True)
                                                             for b in (False, True)}
    assert {p['precision'] for p in draws} == set(PRECISIONS)
    assert len({p['kind'] for p in draws}) >= 6 and len({p['duplicates'] for p in draws}) >= 3
    compared = [run_fuzz(trunks, seed) for seed in range(N_SEEDS)]
    print('fuzz cases', len(compared), 'skipped', compared.count(False))
    assert compared.count(False) <= .1 * len(compared)


def test_describe_features_match_float64(dev):
    """8 neurons x 2 exemplars of 150 x 200 under sparse masks, rerank with beam 4: the features
    the captions are decoded from."""
    h, w, m, kind = R.DESCRIBE_CASE
    nv = R.DESCRIBE_VOCAB
    blocks = synthetic.RESNET_BLOCKS['resnet50']
    sd = R.describe_state_dict()
    images, masks = R.make_case(h, w, m, kind)
    want = R.encode64(images, masks, sd, blocks)
    ctx = hip.Context(hip.make_dims(sd, nv, blocks=blocks), sd, dev)
    try:
        ctx.set_precision('split_f16')
        out = ctx.describe(images.view(8, 2, 3, h, w), masks.view(8, 2, 1, h, w), hip.RERANK, 8, 4,
                           False, 0.2, want_features=True)
        torch.cuda.synchronize()
        check(ctx, out['features'].reshape(m, -1), want, 'describe 150x200')
        tokens = out['tokens'].cpu()
        assert tokens.shape[0] == 8 and bool(((tokens >= 0) & (tokens < nv + 4)).all())
        assert torch.isfinite(out['scores']).all()
    finally:
        ctx.close()
