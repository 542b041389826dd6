"""GPU tests of AlexNet on the HIP trunk: milan_set_alexnet_head, the Linear kernel
(milan_linear), classify / classify_sweep / activations on an AlexNet context and
classifiers.AlexNetClassifier under milan_amd.ablations and exemplars.discriminative.

The model, images and ablation sets are those of tests/golden/reference_goldens_alexnet.*
(width 8: channels 8 / 24 / 48 / 32 / 32, fc6 reads K = 1152 = 4.5 chunks of the Linear kernel;
hidden 72, 10 classes, 12 images at 63x63, 95x127, 255x287 and 224x224: pool5 leaves 1x1, 2x3,
7x8 and 6x6).  Logits and taps are held to the suite's fp32-GEMM-class bound against
tests/alexref.py in float64: max|got - want| <= FEATURE_CLASS x max|want| per tensor.

The tests print the measured multiple of the bound (`LIN ...` / `ALEX ...` lines); DESIGN 4.23
quotes the worst.
"""
import hashlib
import io
import os
import pathlib
import subprocess
import sys

import numpy
import pytest
import torch
from torch.utils import data

import alexref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, exemplars, hip, synthetic
from oracle import exemplars_oracle as E
from test_gpu_ablations import sweep_that_discriminates

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
PREFIX = 'encoder.encoder.model.'
PRECISIONS = ('f32', 'split_f16')
LAYERS = alexref.LAYERS


def trunk_sd(sd):
    """The convs of an alexref state dict under the encoder's `features.N` names."""
    out = {}
    for layer, index in zip(LAYERS, alexref.FEATURES):
        out[f'{PREFIX}features.{index}.weight'] = sd[f'{layer}.weight']
        out[f'{PREFIX}features.{index}.bias'] = sd[f'{layer}.bias']
    return out


def head_of(sd):
    return [sd[f'{fc}.{part}'] for fc in ('fc6', 'fc7', 'linear8') for part in ('weight', 'bias')]


def make_context(sd, head=True):
    trunk = trunk_sd(sd)
    return hip.Context(hip.make_dims(trunk, 1), trunk, torch.device('cuda'),
                       alexnet_head=head_of(sd) if head else None)


@pytest.fixture(scope='module')
def gold():
    tensors, meta = alexref.load_goldens()
    return tensors, meta, alexref.state_dict(meta)


@pytest.fixture(scope='module')
def ctx(gold):
    made = make_context(gold[2])
    yield made
    made.close()


@pytest.fixture(scope='module')
def pictures(gold):
    meta = gold[1]
    return {tuple(geo): alexref.images(meta, geo) for geo in meta['geometries']}


@pytest.fixture(scope='module')
def want64(gold, pictures):
    """float64 (logits, taps) of every golden case, computed once."""
    _, meta, sd = gold
    cache = {}

    def get(geo, name):
        if (geo, name) not in cache:
            case = [tuple(u) for u in meta['cases'][name]]
            cache[geo, name] = alexref.forward(pictures[geo].double(), sd, case)
        return cache[geo, name]

    return get


def cases_of(meta):
    return {name: [tuple(u) for u in units] for name, units in meta['cases'].items()}


def use(ctx, precision):
    ctx.set_precision(precision)
    ctx.set_ablation([])
    return ctx


def ratio_of(got, want):
    scale = float(want.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    if scale == 0.0:
        assert err == 0.0
        return 0.0
    return err / scale


# ---- 1. the Linear kernel alone -------------------------------------------------------------
LINEAR_SHAPES = ((1, 1, 1), (5, 255, 3), (7, 256, 33), (33, 257, 72), (12, 1152, 72),
                 (3, 9216, 40))


def linear_operands(m, k, n):
    """ReLU-like inputs and N(0, 1/K) weights, the operands of the head's layers."""
    g = torch.Generator().manual_seed(1000 * m + k + n)
    x = torch.randn(m, k, generator=g).clamp_(min=0)
    w = torch.randn(n, k, generator=g) * k**-0.5
    b = 0.05 * torch.randn(n, generator=g)
    return x, w, b


@pytest.mark.parametrize('relu', (False, True))
@pytest.mark.parametrize('shape', LINEAR_SHAPES)
def test_linear_against_float64(shape, relu):
    m, k, n = shape
    x, w, b = linear_operands(m, k, n)
    packed = hip.linear_pack(w.cuda())
    for bias in (b, None):
        want = x.double() @ w.double().t()
        if bias is not None:
            want = want + bias.double()
        if relu:
            want = want.clamp(min=0)
        got = hip.linear(x.cuda(), packed, None if bias is None else bias.cuda(), relu=relu)
        assert got.shape == (m, n) and torch.isfinite(got).all()
        ratio = ratio_of(got, want)
        print(f'LIN M={m} K={k} N={n} relu={int(relu)} bias={int(bias is not None)}: '
              f'{ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS, (shape, relu, ratio)


@pytest.mark.parametrize('shape', ((12, 1152, 72), (12, 257, 33), (12, 9216, 40)))
def test_linear_is_batch_invariant(shape):
    m, k, n = shape
    x, w, b = linear_operands(m, k, n)
    x, b = x.cuda(), b.cuda()
    packed = hip.linear_pack(w.cuda())
    whole = hip.linear(x, packed, b, relu=True)
    assert torch.equal(torch.cat([hip.linear(x[:5], packed, b, relu=True),
                                  hip.linear(x[5:], packed, b, relu=True)]), whole)
    # a row's bits do not depend on its place: alone, last of 33 (a second tile), in the middle
    row = x[3:4]
    alone = hip.linear(row, packed, b, relu=True)
    assert torch.equal(alone, whole[3:4])
    padded = torch.cat([x, x, x[:8], row])
    assert torch.equal(hip.linear(padded, packed, b, relu=True)[32:33], alone)
    # (an unaligned view takes the scalar loads: the same bits)
    shifted = torch.empty(m * k + 1, device='cuda')[1:].view(m, k).copy_(x)
    assert torch.equal(hip.linear(shifted, packed, b, relu=True), whole)


# ---- 2. logits and taps against float64, predictions against the goldens -------------------
@pytest.mark.parametrize('precision', PRECISIONS)
def test_logits_and_taps_against_float64(gold, ctx, pictures, want64, precision):
    tensors, meta, _ = gold
    use(ctx, precision)
    worst = {}
    for geo, images in pictures.items():
        for name, case in cases_of(meta).items():
            ctx.set_ablation(case)
            want_logits, want_taps = want64(geo, name)
            got = {'logits': ctx.classify(images), **ctx.activations(images, LAYERS)}
            for key, want in (('logits', want_logits), *want_taps.items()):
                assert got[key].shape == want.shape, (key, got[key].shape, want.shape)
                ratio = ratio_of(got[key], want)
                worst[key] = max(worst.get(key, 0.0), ratio)
                assert ratio <= FEATURE_CLASS, (precision, geo, name, key, ratio)
                if key != 'logits':
                    # zeros are handed out as +0
                    assert not bool(torch.signbit(got[key]).any()), (geo, name, key)
            # no image excused: the maker checked every margin
            assert torch.equal(got['logits'].argmax(dim=-1).cpu(),
                               tensors[f'{geo[0]}x{geo[1]}.{name}.predictions']), (geo, name)
    ctx.set_ablation([])
    for key, ratio in worst.items():
        print(f'ALEX width 8 {precision} {key}: {ratio / FEATURE_CLASS:.3f} x bound')


@pytest.mark.parametrize('precision', ('f32', 'auto'))
def test_image_classifier_against_goldens(gold, pictures, precision):
    tensors, meta, sd = gold
    model = classifiers.AlexNetClassifier(meta['classes'], meta['width'], meta['hidden'],
                                          precision=precision)
    model.load_state_dict(sd, strict=True)
    model.eval().to('cuda')
    classifier = ablations.ImageClassifier(model)
    for geo, images in pictures.items():
        tag = f'{geo[0]}x{geo[1]}'
        dataset = data.TensorDataset(images, tensors[f'{tag}.targets'])
        for name, case in cases_of(meta).items():
            kwargs = dict(batch_size=5, ablate=case, device='cuda', display_progress_as=None)
            predictions = classifier.predict(dataset, **kwargs)
            assert predictions.dtype == torch.int64 and predictions.device.type == 'cuda'
            assert torch.equal(predictions.cpu(), tensors[f'{tag}.{name}.predictions'])
            result = meta['results'][f'{tag}.{name}']
            assert classifier.accuracy(dataset, **kwargs) == result['accuracy']
            accuracies = classifier.accuracies(dataset, **kwargs)
            assert {str(k): v for k, v in accuracies.items()} == result['accuracies']
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


# ---- 3. the split format itself ---------------------------------------------------------------
# A conv gets split weights only when its input channels are a multiple of 32, so the width-8
# trunk above runs the fp32 kernels in both modes (as `encode` does at that width).  Width 32 is
# the smallest at which conv2 .. conv5 run on the split kernels.
def test_split_format_at_width_32(pictures):
    width, geo = 32, (95, 127)
    sd = alexref.make_state_dict(61, width, 72, 10)
    images = pictures[geo][:5]
    ch = alexref.channels(width)
    case = [('conv1', 0), ('conv1', ch[0] - 1), ('conv2', 9), ('conv4', ch[3] - 1), ('conv5', 8),
            ('conv5', 17)]
    ctx = make_context(sd)
    try:
        for name, units in (('none', []), ('mixed', case)):
            want_logits, want_taps = alexref.forward(images.double(), sd, units)
            got = {}
            for precision in PRECISIONS:
                ctx.set_precision(precision)
                ctx.set_ablation(units)
                got[precision] = {'logits': ctx.classify(images),
                                  **ctx.activations(images, LAYERS)}
                for key, want in (('logits', want_logits), *want_taps.items()):
                    ratio = ratio_of(got[precision][key], want)
                    print(f'ALEX width 32 {precision} {name} {key}: '
                          f'{ratio / FEATURE_CLASS:.3f} x bound')
                    assert ratio <= FEATURE_CLASS, (precision, name, key, ratio)
            # the split kernels ran: same class of error, other bits (conv1 is fp32 in both)
            assert torch.equal(got['f32']['conv1'], got['split_f16']['conv1'])
            assert not torch.equal(got['f32']['logits'], got['split_f16']['logits'])
            assert any(not torch.equal(got['f32'][layer], got['split_f16'][layer])
                       for layer in LAYERS[1:])
        # batch invariance, the wiped conv5 and the sweep on the split kernels
        ctx.set_precision('split_f16')
        ctx.set_ablation([('conv5', u) for u in range(ch[4])])
        wiped = ctx.classify(images)
        assert torch.equal(wiped, wiped[:1].expand_as(wiped))
        ctx.set_ablation(case[:3])
        whole = ctx.classify(images)
        assert torch.equal(torch.cat([ctx.classify(images[:2]), ctx.classify(images[2:])]), whole)
        units = [(level, u) for level in range(5) for u in sorted({0, ch[level] - 1, 21})]
        swept = ctx.classify_sweep(images, units)
        rows = []
        for unit in units:
            ctx.set_ablation([*case[:3], unit])
            rows.append(ctx.classify(images, return_logits=False, check=False))
        assert ctx.status() == 0
        assert torch.equal(swept, torch.stack(rows))
    finally:
        ctx.close()


# ---- 4. exactness in f32 ------------------------------------------------------------------------
def test_batch_invariance_and_wiped_conv5(gold, ctx, pictures):
    _, meta, sd = gold
    use(ctx, 'f32')
    for geo in ((95, 127), (255, 287)):
        images = pictures[geo]
        ctx.set_ablation(cases_of(meta)['mixed'])
        whole = ctx.classify(images)
        assert torch.equal(torch.cat([ctx.classify(images[:5]), ctx.classify(images[5:])]), whole)
        ctx.set_ablation(cases_of(meta)['conv5_all'])
        wiped = ctx.classify(images)
        assert torch.equal(wiped, wiped[:1].expand_as(wiped))
    ctx.set_ablation([])


SUB_SCRIPT = r'''
import hashlib, sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import torch
import alexref
import test_gpu_alexnet as T
tensors, meta = alexref.load_goldens()
c = T.make_context(alexref.state_dict(meta))
c.set_precision('f32')
c.set_ablation([(0, 1), (2, 5)])
images = alexref.images(meta, (95, 127))[:7]
got = c.activations(images, [4, 0, 2])
digest = hashlib.sha256()
for level in (4, 0, 2):
    digest.update(got[level].cpu().numpy().tobytes())
digest.update(c.classify(images).cpu().numpy().tobytes())
print('SHA', digest.hexdigest())
c.close()
'''


def test_sub_batches(ctx, pictures, tmp_path):
    """MILAN_ENC_SUB is cached per process: one fresh child walks 7 images in passes of
    3 + 3 + 1; this process walks them in one.  The same bits."""
    use(ctx, 'f32')
    ctx.set_ablation([(0, 1), (2, 5)])
    images = pictures[95, 127][:7]
    got = ctx.activations(images, [4, 0, 2])
    digest = hashlib.sha256()
    for level in (4, 0, 2):
        digest.update(got[level].cpu().numpy().tobytes())
    digest.update(ctx.classify(images).cpu().numpy().tobytes())
    ctx.set_ablation([])
    script = tmp_path / 'sub.py'
    script.write_text(SUB_SCRIPT.format(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd'),
                                        tests=str(REPO / 'tests')))
    env = dict(os.environ, MILAN_ENC_SUB='3')
    out = subprocess.run(['timeout', '-k', '10', '120', sys.executable, str(script)], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f'SHA {digest.hexdigest()}' in out.stdout, out.stdout


# The golden model at the golden images predicts one class for every image under every unit of
# such a sweep (float64: 70 times class 4), which no wrong pass could change.  This seed, the
# goldens' sizes otherwise (width 8, hidden 72, 10 classes, 63x63), gives in float64 6 distinct
# rows out of 10, 6 distinct columns out of 7, classes 1 / 2 / 4, rows changed by units of all
# five levels, and a top-2 margin of at least 5e-3 x max|logit| (1000 x FEATURE_CLASS).
SWEEP_SEED = 7


def sweep_context():
    return make_context(alexref.make_state_dict(SWEEP_SEED, 8, 72, 10))


def sweep_digest(ctx):
    """sha256 over the sweep's predictions and `correct` for 7 images at 63x63, units on
    conv1..conv5, on top of a non-empty base set; the targets are the base set's predictions,
    so `correct` counts the images a unit leaves alone."""
    images = alexref.make_images(SWEEP_SEED, 7, (63, 63))
    ch = alexref.channels(8)
    units = [(level, u % ch[level]) for u in (0, -1) for level in range(5)]
    ctx.set_precision('f32')
    ctx.set_ablation([(0, 1), (2, 5)])
    targets = ctx.classify(images, return_logits=False)
    predictions, correct = sweep_that_discriminates(ctx, images, units, targets)
    ctx.set_ablation([])
    digest = hashlib.sha256()
    for t in (targets, predictions, correct):
        digest.update(t.cpu().numpy().tobytes())
    return digest.hexdigest()


SWEEP_SUB_SCRIPT = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import test_gpu_alexnet as T
c = T.sweep_context()
print('SHA', T.sweep_digest(c))
c.close()
"""


def test_sweep_in_sub_batches(tmp_path):
    """test_sub_batches for classify_sweep: the child sweeps 7 images in passes of 3 + 3 + 1
    (every pass reads its images, resumes from the levels it holds and writes its columns of
    the prediction rows), this process in one."""
    made = sweep_context()
    try:
        want = sweep_digest(made)
    finally:
        made.close()
    script = tmp_path / 'sub.py'
    script.write_text(SWEEP_SUB_SCRIPT.format(repo=str(REPO),
                                              pkg=str(REPO / 'neuron-descriptions_amd'),
                                              tests=str(REPO / 'tests')))
    env = dict(os.environ, MILAN_ENC_SUB='3')
    out = subprocess.run(['timeout', '-k', '10', '120', sys.executable, str(script)], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f'SHA {want}' in out.stdout, out.stdout


def test_sweep_equals_the_loop(gold, ctx, pictures):
    _, meta, _ = gold
    use(ctx, 'f32')
    ch = alexref.channels(meta['width'])
    base = [('conv2', 3), ('conv4', 30)]
    units = [(level, u) for level in range(5) for u in sorted({0, 5, ch[level] - 1})]
    units.append(('conv4', 30))   # (already in the set)
    for geo in ((63, 63), (255, 287)):
        images = pictures[geo]
        targets = torch.arange(len(images)) % meta['classes']
        ctx.set_ablation(base)
        swept, correct = ctx.classify_sweep(images, units, targets)
        rows = []
        for unit in units:
            ctx.set_ablation([*base, unit])
            rows.append(ctx.classify(images, return_logits=False))
        rows = torch.stack(rows)
        assert torch.equal(swept, rows)
        assert torch.equal(correct.cpu().long(), (rows.cpu() == targets).sum(dim=1))
        # a subset on the highest levels only: the walk starts from the images all the same
        ctx.set_ablation(base)
        assert torch.equal(ctx.classify_sweep(images, units[-7:]), rows[-7:])
    ctx.set_ablation([])


def test_taps_and_classify_do_not_disturb_each_other(gold, ctx, pictures):
    _, meta, _ = gold
    use(ctx, 'f32')
    images = pictures[95, 127]
    ctx.set_ablation(cases_of(meta)['mixed'])
    before = ctx.classify(images)
    together = ctx.activations(images, LAYERS)
    for layer in LAYERS:
        assert torch.equal(ctx.activations(images, [layer])[layer], together[layer])
    by_index = ctx.activations(images, [4, 1])
    assert torch.equal(by_index[4], together['conv5'])
    assert torch.equal(by_index[1], together['conv2'])
    assert torch.equal(ctx.classify(images), before)
    ctx.set_ablation([])


def test_encode_and_the_empty_set(gold, ctx, pictures):
    _, meta, sd = gold
    images = pictures[95, 127][:4]
    g = torch.Generator().manual_seed(9)
    exemplar_images = torch.randint(256, (6, 3, 96, 96), generator=g, dtype=torch.uint8)
    masks = (torch.rand(6, 1, 96, 96, generator=g) > 0.6).to(torch.uint8)
    bare = make_context(sd, head=False)
    try:
        for precision in PRECISIONS:
            use(ctx, precision)
            bare.set_precision(precision)
            want = bare.encode(exemplar_images, masks)
            assert torch.equal(ctx.encode(exemplar_images, masks), want)
            never = ctx.classify(images)
            ctx.set_ablation(cases_of(meta)['mixed'])
            assert torch.equal(ctx.encode(exemplar_images, masks), want)
            assert not torch.equal(ctx.classify(images), never)
            ctx.set_ablation([])
            assert torch.equal(ctx.classify(images), never)
        # a fresh context that never had a set: the same bits
        fresh = make_context(sd)
        fresh.set_precision('split_f16')
        assert torch.equal(fresh.classify(images), never)
        fresh.close()
    finally:
        bare.close()


# ---- 5. surface -----------------------------------------------------------------------------------
def test_errors(gold, ctx, pictures):
    _, meta, sd = gold
    images = pictures[63, 63]
    ch = alexref.channels(meta['width'])
    # a headless context behaves as before the head existed
    bare = make_context(sd, head=False)
    with pytest.raises(ValueError, match='ResNet'):
        bare.classify(images)
    with pytest.raises(ValueError, match='ResNet'):
        bare.set_ablation([(0, 0)])
    with pytest.raises(ValueError, match='ResNet'):
        bare.activations(images, [0])
    # heads that do not chain
    head = head_of(sd)
    with pytest.raises(ValueError, match='chain'):
        bare.set_alexnet_head(head[0][:, :-1], *head[1:])
    with pytest.raises(ValueError, match='chain'):
        bare.set_alexnet_head(head[0], head[1], head[2][:, :-1], *head[3:])
    with pytest.raises(ValueError):
        bare.set_alexnet_head(head[0], head[1][:-1], *head[2:])
    with pytest.raises(ValueError, match='ResNet'):
        bare.classify(images)
    bare.set_alexnet_head(*head)
    use(ctx, 'f32')
    bare.set_precision('f32')
    assert torch.equal(bare.classify(images), ctx.classify(images))
    bare.close()
    # a ResNet context has no such head
    rsd = {PREFIX + k: v for k, v in synthetic.resnet_state_dict('resnet18', seed=1,
                                                                 width=8).items()}
    resnet = hip.Context(hip.make_dims(rsd, 1, blocks=(2, 2, 2, 2)), rsd, torch.device('cuda'))
    with pytest.raises(ValueError, match='AlexNet'):
        resnet.set_alexnet_head(*head)
    resnet.close()
    # levels, units, names
    with pytest.raises(IndexError):
        ctx.set_ablation([(2, ch[2])])
    with pytest.raises(IndexError):
        ctx.set_ablation([('conv1', -1)])
    with pytest.raises(ValueError):
        ctx.set_ablation([(5, 0)])
    with pytest.raises(ValueError, match='conv1'):
        ctx.set_ablation([('layer1', 0)])
    with pytest.raises(ValueError):
        ctx.set_ablation([('fc6', 0)])
    with pytest.raises(IndexError):
        ctx.classify_sweep(images, [(0, ch[0])])
    with pytest.raises(ValueError, match='not one of 0..4'):
        ctx.activations(images, [5])
    with pytest.raises(ValueError, match='twice'):
        ctx.activations(images, ['conv3', 2])
    with pytest.raises(ValueError, match='no native tap'):
        ctx.activations(images, ['layer2'])
    with pytest.raises(ValueError, match='too small'):
        ctx.classify(images[:, :, :62])
    ctx.set_precision('f16')
    with pytest.raises(ValueError, match='fast f16'):
        ctx.classify(images)
    with pytest.raises(ValueError, match='fast f16'):
        ctx.activations(images, [1])
    ctx.set_precision('f32')
    # (a failed setter leaves the set as it was: empty)
    want = alexref.forward(images.double(), sd)[0]
    assert ratio_of(ctx.classify(images), want) <= FEATURE_CLASS


def test_unit_scores_equal_the_loop(gold, pictures):
    tensors, meta, sd = gold
    model = classifiers.AlexNetClassifier(meta['classes'], meta['width'], meta['hidden'],
                                          precision='f32')
    model.load_state_dict(sd, strict=True)
    model.eval().to('cuda')
    classifier = ablations.ImageClassifier(model)
    geo = (95, 127)
    dataset = data.TensorDataset(pictures[geo], tensors[f'{geo[0]}x{geo[1]}.targets'])
    ch = alexref.channels(meta['width'])
    units = [(layer, u) for index, layer in enumerate(LAYERS) for u in (0, ch[index] - 1)]
    kwargs = dict(batch_size=5, ablate=[('conv3', 4)], device='cuda', display_progress_as=None)
    scores = classifier.unit_scores(dataset, units, **kwargs)
    loop = [classifier.accuracy(dataset, **{**kwargs, 'ablate': [('conv3', 4), unit]})
            for unit in units]
    assert scores == loop
    with pytest.raises(ValueError, match='not found in model'):
        classifier.unit_scores(dataset, [('fc6', 0)], **kwargs)
    assert not model.training


def dissect(model, dataset, layer, tmp_path, source):
    """exemplars.discriminative against the oracle's `compute` fed `source(images)` = the
    layer's activations for the same batches (test_gpu_activations.py's check)."""
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    torch.manual_seed(31)
    topk, rq = exemplars.discriminative(model, dataset, layer=layer, image_size=95,
                                        num_workers=0, save_viz=False, results_dir=tmp_path,
                                        **kwargs)

    def hiddens(images):
        return source(images.cuda()).cpu()

    def topk_and_quantile(images):
        h = hiddens(images)
        b, c = h.shape[:2]
        return h.view(b, c, -1).max(dim=2)[0], h.permute(0, 2, 3, 1).reshape(-1, c)

    mul, add = exemplars.byte_renormalization(dataset)
    torch.manual_seed(31)
    want = E.compute(topk_and_quantile, hiddens, dataset, mul=tuple(mul), add=tuple(add),
                     stable_ties=True, **kwargs)
    out = tmp_path / layer
    assert torch.equal(torch.from_numpy(numpy.load(out / 'images.npy')), want['images'])
    assert torch.equal(torch.from_numpy(numpy.load(out / 'masks.npy')), want['masks'])
    assert int(want['masks'].sum()) > 0
    values, ids = topk.result()
    assert torch.equal(ids.cpu(), want['ids'])
    assert torch.equal(values.cpu(), want['activations'])
    text = io.StringIO()
    numpy.savetxt(text, want['activations'].numpy(), delimiter=',', fmt='%.5e')
    assert (out / 'activations.csv').read_text() == text.getvalue()
    assert torch.equal(rq.quantiles(.9).cpu().reshape(-1), want['levels'].reshape(-1))
    return want


@pytest.mark.parametrize('layer', ('conv1', 'conv5'))
def test_dissect_alexnet_classifier(gold, layer, tmp_path):
    _, meta, sd = gold
    model = classifiers.AlexNetClassifier(meta['classes'], meta['width'], meta['hidden'],
                                          precision='f32')
    model.load_state_dict(sd, strict=True)
    model.eval()
    g = torch.Generator().manual_seed(2305)
    dataset = data.TensorDataset(torch.rand(23, 3, 95, 127, generator=g))

    def source(images):
        with torch.no_grad():
            assert model.runs_natively(images)
            return model.activations(images, layer)[layer]

    want = dissect(model, dataset, layer, tmp_path, source)
    channels = alexref.channels(meta['width'])[LAYERS.index(layer)]
    assert want['ids'].shape == (channels, 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
