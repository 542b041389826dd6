"""GPU tests of unit ablation and classification on the HIP trunk (milan_set_ablation,
milan_classify, milan_classify_sweep; milan_amd.ablations on a ResNetClassifier).

Slim trunks (width 8: conv1 is exactly one split group, C4 = 64 / 256), 12 images at 64x64,
33x47 and 7x9 (last stage 2x2, 2x2 and 1x1 pixels), 10 / 37 classes.  The logits are held to
the suite's fp32-GEMM-class bound against a float64 restatement (tests/ablref.py):
max|err| <= FEATURE_CLASS x max|want|.  A masked channel left at its value moves the logits
by orders of magnitude more.
"""
import ctypes
import hashlib
import os
import pathlib
import subprocess
import sys

import pytest
import torch
from torch.utils import data

import ablref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, hip, synthetic

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
PREFIX = 'encoder.encoder.model.'
CONFIGS = ('resnet18', 'resnet50')
PRECISIONS = ('f32', 'split_f16')


@pytest.fixture(scope='module')
def gold():
    return ablref.load_goldens()


@pytest.fixture(scope='module')
def contexts(gold):
    """One context per config (the precision is switched per test)."""
    tensors, meta = gold
    made = {}
    for config in CONFIGS:
        sd = {PREFIX + k: v for k, v in ablref.state_dict(config, tensors, meta).items()}
        dims = hip.make_dims(sd, 1, blocks=synthetic.RESNET_BLOCKS[config])
        made[config] = hip.Context(dims, sd, torch.device('cuda'))
    yield made
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope='module')
def want64(gold):
    """float64 logits of every golden case, computed once."""
    tensors, meta = gold
    cache = {}

    def get(config, geo, name):
        key = (config, geo, name)
        if key not in cache:
            case = [tuple(u) for u in meta['configs'][config]['cases'][name]]
            cache[key] = ablref.forward(tensors[f'images.{geo[0]}x{geo[1]}'].double(),
                                        ablref.state_dict(config, tensors, meta),
                                        synthetic.RESNET_BLOCKS[config], case)
        return cache[key]

    return get


def geometries(meta):
    return [tuple(g) for g in meta['geometries']]


def cases_of(meta, config):
    return {name: [tuple(u) for u in units]
            for name, units in meta['configs'][config]['cases'].items()}


def use(contexts, config, precision):
    ctx = contexts[config]
    ctx.set_precision(precision)
    ctx.set_ablation([])
    return ctx


# ---- 1. logits against float64 --------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config', CONFIGS)
def test_logits_against_float64(gold, contexts, want64, config, precision):
    tensors, meta = gold
    ctx = use(contexts, config, precision)
    worst = 0.0
    for geo in geometries(meta):
        images = tensors[f'images.{geo[0]}x{geo[1]}']
        for name, case in cases_of(meta, config).items():
            ctx.set_ablation(case)
            got = ctx.classify(images).cpu().double()
            want = want64(config, geo, name)
            ratio = float((got - want).abs().max() / want.abs().max())
            worst = max(worst, ratio)
            print(f'ABL {config} {precision} {geo[0]}x{geo[1]} {name}: '
                  f'{ratio / FEATURE_CLASS:.3f} x bound')
            assert ratio <= FEATURE_CLASS, (config, precision, geo, name, ratio)
    ctx.set_ablation([])
    print(f'ABL {config} {precision}: worst {worst / FEATURE_CLASS:.3f} x bound')


# ---- 2. predictions, accuracy, accuracies against the reference's goldens ---------------
@pytest.mark.parametrize('precision', ('f32', 'auto'))
@pytest.mark.parametrize('config', CONFIGS)
def test_image_classifier_against_goldens(gold, want64, config, precision):
    tensors, meta = gold
    model = classifiers.ResNetClassifier(config, num_classes=meta['configs'][config]['classes'],
                                         width=meta['width'], precision=precision)
    model.load_state_dict(ablref.state_dict(config, tensors, meta), strict=True)
    model.eval().to('cuda')
    classifier = ablations.ImageClassifier(model)
    for geo in geometries(meta):
        tag = f'{config}.{geo[0]}x{geo[1]}'
        images = tensors[f'images.{geo[0]}x{geo[1]}']
        targets = tensors[f'{tag}.targets']
        dataset = data.TensorDataset(images, targets)
        for name, case in cases_of(meta, config).items():
            kwargs = dict(batch_size=5, ablate=case, device='cuda', display_progress_as=None)
            predictions = classifier.predict(dataset, **kwargs)
            assert predictions.dtype == torch.int64 and predictions.device.type == 'cuda'
            want = want64(config, geo, name)
            top2 = want.topk(2, dim=-1).values
            excused = (top2[:, 0] - top2[:, 1]) < 2 * FEATURE_CLASS * float(want.abs().max())
            assert int(excused.sum()) <= 0.1 * len(images)
            golden = tensors[f'{tag}.{name}.predictions']
            assert torch.equal(predictions.cpu()[~excused], golden[~excused]), (tag, name)
            result = meta['results'][f'{tag}.{name}']
            accuracy = classifier.accuracy(dataset, **kwargs)
            accuracies = classifier.accuracies(dataset, **kwargs)
            if not bool(excused.any()):
                assert accuracy == result['accuracy']
                assert {str(k): v for k, v in accuracies.items()} == result['accuracies']
            else:
                assert abs(accuracy - result['accuracy']) <= int(excused.sum()) / len(images)
    assert model._ablation == ()


# ---- 3. exact properties (f32) --------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS)
def test_exact_properties_f32(gold, contexts, config):
    tensors, meta = gold
    ctx = use(contexts, config, 'f32')
    channels = ablref.level_channels(config, meta['width'])
    bias = tensors[f'{config}.fc.bias'].cuda()
    for geo in geometries(meta):
        images = tensors[f'images.{geo[0]}x{geo[1]}']
        never = ctx.classify(images)
        # all of layer4: the pooled vector is zero, the logits are the bias
        ctx.set_ablation([('layer4', u) for u in range(channels[4])])
        wiped = ctx.classify(images)
        assert torch.equal(wiped, bias.expand_as(wiped))
        # all of an earlier stage: nothing of the image is left, every image gets the same
        for level in (1, 2, 3):
            ctx.set_ablation([(level, u) for u in range(channels[level])])
            same = ctx.classify(images)
            assert torch.equal(same, same[:1].expand_as(same)), level
            assert not torch.equal(same, wiped)
        # empty, cleared and never set
        ctx.set_ablation([])
        assert torch.equal(ctx.classify(images), never)
        # order and duplicates
        units = [('layer3', 5), ('conv1', 2), ('layer1', 0), ('layer3', 1)]
        ctx.set_ablation(units)
        a = ctx.classify(images)
        ctx.set_ablation(list(reversed(units)) + units[:2])
        assert torch.equal(ctx.classify(images), a)
        assert not torch.equal(a, never)
        # the batch is invariant
        parts = torch.cat([ctx.classify(images[:5]), ctx.classify(images[5:])])
        assert torch.equal(parts, a)
        whole = ctx.classify(images, return_logits=False)
        assert torch.equal(whole, a.argmax(dim=-1))
        assert torch.equal(torch.cat([ctx.classify(images[:5], return_logits=False),
                                      ctx.classify(images[5:], return_logits=False)]), whole)
        ctx.set_ablation([])


def test_argmax_ties_and_nan(gold):
    tensors, meta = gold
    config = 'resnet18'
    sd = ablref.state_dict(config, tensors, meta)
    images = tensors['images.33x47']

    def predictions(weight, bias):
        full = {PREFIX + k: v for k, v in sd.items()}
        full[PREFIX + 'fc.weight'], full[PREFIX + 'fc.bias'] = weight, bias
        ctx = hip.Context(hip.make_dims(full, 1, blocks=synthetic.RESNET_BLOCKS[config]), full,
                          torch.device('cuda'))
        try:
            return (ctx.classify(images), ctx.classify(images, return_logits=False))
        finally:
            ctx.close()

    w, b = sd['fc.weight'].clone(), sd['fc.bias'].clone()
    # every row the same: all logits of an image are equal, the lowest index wins
    logits, preds = predictions(w[:1].repeat(10, 1), b[:1].repeat(10))
    assert torch.equal(logits, logits[:, :1].expand_as(logits))
    assert torch.equal(preds.cpu(), torch.zeros(12, dtype=torch.int64))
    # two equal rows that lead everywhere (zero weights, a large bias): the lower one wins
    w2, b2 = w.clone(), b.clone()
    w2[3], w2[6], b2[3], b2[6] = 0, 0, 100., 100.
    logits, preds = predictions(w2, b2)
    assert torch.equal(logits[:, 3], logits[:, 6])
    assert float(logits[:, 3].min()) == 100. == float(logits.max())
    assert torch.equal(preds.cpu(), torch.full((12,), 3, dtype=torch.int64))
    assert torch.equal(preds.cpu(), logits.cpu().argmax(dim=-1))
    # a NaN counts as the maximum, the first of two wins
    b3 = b.clone()
    b3[4] = float('nan')
    b3[8] = float('nan')
    logits, preds = predictions(w, b3)
    assert bool(torch.isnan(logits[:, 4]).all()) and bool(torch.isnan(logits[:, 8]).all())
    assert torch.equal(preds.cpu(), torch.full((12,), 4, dtype=torch.int64))


@pytest.mark.parametrize('config', CONFIGS)
def test_the_set_does_not_leak_into_encode(gold, contexts, config):
    tensors, meta = gold
    channels = ablref.level_channels(config, meta['width'])
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (6, 3, 33, 47), dtype=torch.uint8, generator=g)
    masks = (torch.rand(6, 1, 33, 47, generator=g) > 0.5).to(torch.uint8)
    for precision in PRECISIONS:
        ctx = use(contexts, config, precision)
        before = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        ctx.set_ablation([('conv1', 0), ('layer2', 3)] +
                         [('layer4', u) for u in range(channels[4])])
        during = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        ctx.set_ablation([])
        after = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        for a, b, c in zip(before, during, after):
            assert torch.equal(a, b) and torch.equal(a, c)
            assert float(a.abs().max()) > 0


# ---- 4. the sweep ----------------------------------------------------------------------------
def sweep_units(config, width):
    channels = ablref.level_channels(config, width)
    if config == 'resnet18':
        return [(level, u) for level in range(5) for u in range(channels[level])]
    return [(level, u) for level in range(5)
            for u in sorted({0, channels[level] - 1, *range(0, channels[level], 7)})]


@pytest.mark.parametrize('base', [(), ((1, 2), (3, 0), (4, 5), (0, 1))], ids=['empty', 'base'])
@pytest.mark.parametrize('geo', [(33, 47), (7, 9)], ids=['33x47', '7x9'])
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config', CONFIGS)
def test_sweep_is_one_classify_per_unit(gold, contexts, config, precision, geo, base):
    tensors, meta = gold
    ctx = use(contexts, config, precision)
    images = tensors[f'images.{geo[0]}x{geo[1]}'].cuda()
    targets = tensors[f'{config}.{geo[0]}x{geo[1]}.targets'].cuda()
    units = sweep_units(config, meta['width'])
    if config == 'resnet18':
        assert len(units) == 128
    # (interleave the levels: the call groups them itself)
    units = units[::2] + units[1::2]
    ctx.set_ablation(base)
    predictions, correct = ctx.classify_sweep(images, units, targets)
    only = ctx.classify_sweep(images, units)
    assert torch.equal(only, predictions)
    assert predictions.shape == (len(units), len(images)) and correct.dtype == torch.int32
    want = []
    for unit in units:
        ctx.set_ablation([*base, unit])
        want.append(ctx.classify(images, return_logits=False, check=False))
    ctx.set_ablation([])
    assert ctx.status() == 0
    want = torch.stack(want)
    assert torch.equal(predictions, want)
    assert torch.equal(correct.long(), (want == targets).sum(dim=1))
    assert len(torch.unique(want, dim=0)) > 1, 'every unit gives the same predictions'


# ---- 4b. the sweep and classify over sub-batches ------------------------------------------------
SUB_BASE = [(0, 1), (2, 5)]


def correct_without_predictions(ctx, images, units, targets):
    """milan_classify_sweep with `predictions` NULL: the prediction rows then live in the
    workspace, carved at the same address in every pass.  `hip.Context.classify_sweep` always
    passes a tensor, so this goes to the library directly."""
    lib = hip.load_library()
    images = images.to(ctx.device, torch.float32).contiguous()
    targets = targets.to(ctx.device, torch.int64).contiguous()
    n, _, h, w = images.shape
    count = len(units)
    levels = (ctypes.c_int32 * count)(*[level for level, _ in units])
    ids = (ctypes.c_int32 * count)(*[unit for _, unit in units])
    need = int(lib.milan_classify_workspace_bytes(ctx._h, n, h, w, count))
    ws = torch.empty(need, dtype=torch.uint8, device=ctx.device)
    correct = torch.full((count,), -1, dtype=torch.int32, device=ctx.device)
    with torch.cuda.device(ctx.device):
        code = lib.milan_classify_sweep(ctx._h, images.data_ptr(), n, h, w, levels, ids, count,
                                        targets.data_ptr(), correct.data_ptr(), None,
                                        ws.data_ptr(), ws.numel(), None)
    assert code == 0, code
    torch.cuda.synchronize()
    return correct


def sweep_that_discriminates(ctx, images, units, targets):
    """`classify_sweep` on inputs that can tell a wrong result from a right one: the prediction
    rows differ between units and between images and `correct` is not one number, so a pass
    that read other images, a held level a suffix overwrote or a row written elsewhere changes
    the result.  The same `correct` comes out with the rows kept in the workspace."""
    predictions, correct = ctx.classify_sweep(images, units, targets)
    assert predictions.shape == (len(units), len(images)) and correct.shape == (len(units),)
    assert len(torch.unique(predictions, dim=0)) > 1, 'every unit gives the same predictions'
    assert len(torch.unique(predictions, dim=1).t()) > 1, 'every image gets the same predictions'
    assert len(torch.unique(correct)) > 1, 'every unit has the same count'
    assert torch.equal(correct_without_predictions(ctx, images, units, targets), correct)
    return predictions, correct


def sub_batch_digest(ctx, tensors, meta, config):
    """sha256 over classify's logits and predictions and the sweep's predictions and `correct`
    for the first 7 images at 33x47, units on all five levels (level 0 is held where it is,
    levels 1..4 in the sweep's copy), on top of a non-empty base set."""
    images = tensors['images.33x47'][:7].cuda()
    targets = tensors[f'{config}.33x47.targets'][:7].cuda()
    channels = ablref.level_channels(config, meta['width'])
    units = [(level, u) for u in (0, -1) for level in range(5)]
    units = [(level, u % channels[level]) for level, u in units]
    ctx.set_precision('f32')
    ctx.set_ablation(SUB_BASE)
    predictions, correct = sweep_that_discriminates(ctx, images, units, targets)
    digest = hashlib.sha256()
    for t in (ctx.classify(images), ctx.classify(images, return_logits=False), predictions,
              correct):
        digest.update(t.cpu().numpy().tobytes())
    ctx.set_ablation([])
    return digest.hexdigest()


SUB_SCRIPT = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import ablref
import test_gpu_ablations as T
from milan_amd import hip, synthetic
tensors, meta = ablref.load_goldens()
sd = {{T.PREFIX + k: v for k, v in ablref.state_dict({config!r}, tensors, meta).items()}}
c = hip.Context(hip.make_dims(sd, 1, blocks=synthetic.RESNET_BLOCKS[{config!r}]), sd,
                hip.require_device('cuda'))
print('SHA', T.sub_batch_digest(c, tensors, meta, {config!r}))
c.close()
"""


@pytest.mark.parametrize('config', CONFIGS)
def test_sweep_and_classify_in_sub_batches(gold, contexts, config, tmp_path):
    """MILAN_ENC_SUB is cached per process: one fresh child classifies and sweeps 7 images in
    passes of 3 + 3 + 1; this process does so in one.  The same bits."""
    tensors, meta = gold
    want = sub_batch_digest(contexts[config], tensors, meta, config)
    script = tmp_path / 'sub.py'
    script.write_text(SUB_SCRIPT.format(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd'),
                                        tests=str(REPO / 'tests'), config=config))
    env = dict(os.environ, MILAN_ENC_SUB='3')
    out = subprocess.run(['timeout', '-k', '10', '120', sys.executable, str(script)], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f'SHA {want}' in out.stdout, out.stdout


@pytest.mark.parametrize('precision', ('f32', 'auto'))
def test_unit_scores_is_the_accuracy_loop(gold, precision):
    tensors, meta = gold
    config = 'resnet18'
    model = classifiers.ResNetClassifier(config, num_classes=10, width=meta['width'],
                                         precision=precision)
    model.load_state_dict(ablref.state_dict(config, tensors, meta), strict=True)
    model.eval().to('cuda')
    classifier = ablations.ImageClassifier(model)
    dataset = data.TensorDataset(tensors['images.7x9'], tensors[f'{config}.7x9.targets'])
    units = [(ablref.LAYERS[level], u) for level, u in sweep_units(config, meta['width'])][::5]
    base = [('layer2', 4), ('layer4', 60)]
    got = classifier.unit_scores(dataset, units, batch_size=5, ablate=base, device='cuda',
                                 display_progress_as=None)
    want = [classifier.accuracy(dataset, batch_size=5, ablate=[*base, u], device='cuda',
                                display_progress_as=None) for u in units]
    assert got == want and len(set(got)) > 1
    assert model._ablation == ()


# ---- 5. errors -------------------------------------------------------------------------------
def test_errors(gold, contexts):
    tensors, meta = gold
    images = tensors['images.7x9']
    ctx = use(contexts, 'resnet18', 'f32')
    channels = ablref.level_channels('resnet18', meta['width'])
    with pytest.raises(IndexError):
        ctx.set_ablation([(2, channels[2])])
    with pytest.raises(ValueError):
        ctx.set_ablation([(5, 0)])
    with pytest.raises(ValueError):
        ctx.set_ablation([('fc', 0)])
    with pytest.raises(IndexError):
        ctx.classify_sweep(images, [(0, channels[0])])
    ctx.set_precision('f16')
    with pytest.raises(ValueError, match='fast f16'):
        ctx.classify(images)
    ctx.set_precision('f32')
    # (a failed setter leaves the set as it was: empty)
    assert torch.equal(ctx.classify(images).cpu().argmax(dim=-1),
                       tensors['resnet18.7x9.none.predictions'])
    # no head
    sd = {PREFIX + k: v for k, v in synthetic.resnet_state_dict(
        'resnet18', seed=1, width=8, with_fc=False).items()}
    bare = hip.Context(hip.make_dims(sd, 1, blocks=(2, 2, 2, 2)), sd, torch.device('cuda'))
    with pytest.raises(RuntimeError, match='fc.weight'):
        bare.classify(images)
    bare.set_ablation([(1, 0)])  # the set itself needs no head
    bare.close()
    # AlexNet
    sd = {PREFIX + k: v for k, v in synthetic.alexnet_state_dict(seed=2, width=8).items()}
    alex = hip.Context(hip.make_dims(sd, 1), sd, torch.device('cuda'))
    with pytest.raises(ValueError, match='ResNet'):
        alex.classify(tensors['images.64x64'])
    with pytest.raises(ValueError, match='ResNet'):
        alex.set_ablation([(0, 0)])
    alex.close()


# ---- 6. the split format itself ----------------------------------------------------------------
# A conv gets split weights only when its input channels are a multiple of 32, so the width-8
# trunks above run the fp32 kernels in both modes (as `encode` does at that width).  Width 32 is
# the smallest trunk on which split_f16 really runs: the pixel-pair stem, the split stem tail,
# the split mask kernel and the average pool that removes the activation scale.
SPLIT_WIDTH = 32


@pytest.mark.parametrize('config', CONFIGS)
def test_split_format_at_width_32(gold, config):
    tensors, meta = gold
    classes = meta['configs'][config]['classes']
    blocks = synthetic.RESNET_BLOCKS[config]
    channels = ablref.level_channels(config, SPLIT_WIDTH)
    g = torch.Generator().manual_seed(77)
    sd = synthetic.resnet_state_dict(config, seed=41, width=SPLIT_WIDTH, with_fc=False)
    sd['fc.weight'] = torch.randn(classes, channels[4], generator=g) * channels[4]**-0.5
    sd['fc.bias'] = 0.05 * torch.randn(classes, generator=g)
    full = {PREFIX + k: v for k, v in sd.items()}
    ctx = hip.Context(hip.make_dims(full, 1, blocks=blocks), full, torch.device('cuda'))
    case = [('conv1', 0), ('conv1', 31), ('layer1', 9), ('layer3', channels[3] - 1),
            ('layer4', 8), ('layer4', 17)]
    try:
        for geo in ((33, 47), (7, 9)):
            images = tensors[f'images.{geo[0]}x{geo[1]}']
            for name, units in (('none', []), ('mixed', case)):
                want = ablref.forward(images.double(), sd, blocks, units)
                got = {}
                for precision in PRECISIONS:
                    ctx.set_precision(precision)
                    ctx.set_ablation(units)
                    got[precision] = ctx.classify(images)
                    ratio = float((got[precision].cpu().double() - want).abs().max() /
                                  want.abs().max())
                    print(f'ABL {config} width 32 {precision} {geo[0]}x{geo[1]} {name}: '
                          f'{ratio / FEATURE_CLASS:.3f} x bound')
                    assert ratio <= FEATURE_CLASS, (config, precision, geo, name, ratio)
                # the split kernels ran: same class of error, other bits
                assert not torch.equal(got['f32'], got['split_f16'])
            ctx.set_precision('split_f16')
            # all of layer4: zeros through the pool, the logits are the bias
            ctx.set_ablation([('layer4', u) for u in range(channels[4])])
            wiped = ctx.classify(images)
            assert torch.equal(wiped, sd['fc.bias'].cuda().expand_as(wiped))
            # batch invariance and the sweep, on the split kernels
            ctx.set_ablation(case[:3])
            whole = ctx.classify(images)
            assert torch.equal(torch.cat([ctx.classify(images[:5]), ctx.classify(images[5:])]),
                               whole)
            units = [(level, u) for level in range(5)
                     for u in sorted({0, channels[level] - 1, *range(3, channels[level], 37)})]
            swept = ctx.classify_sweep(images, units)
            want = []
            for unit in units:
                ctx.set_ablation([*case[:3], unit])
                want.append(ctx.classify(images, return_logits=False, check=False))
            assert ctx.status() == 0
            assert torch.equal(swept, torch.stack(want))
    finally:
        ctx.close()
