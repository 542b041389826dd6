"""GPU tests of VGG-11 / 13 / 16 / 19 on the HIP trunk (MILAN_TRUNK_VGG): classify, activations,
unit ablation and the sweep against tests/vggref.py in float64, `classifiers.VGGClassifier` end
to end, and the refusals.

Seeded models (vggref.make_state_dict), hidden 72, 10 classes, 5 images unless said:
  width 8   channels 8 / 16 / 32 / 64 / 64: conv3_2 has 32 input channels but reads conv3_1's
            fp32 output, so blocks 1-3 stay fp32 in the split mode and pool3 converts
  width 16  16 / 32 / 64 / 128 / 128: pool2 converts, block 3 on is split
  width 32  conv1_2 is the first split conv, fed by vgg_first_kernel<true>
  width 64  torchvision's widths once (hidden 128, 2 images of 224 x 224)
Geometries: 32x32 (every pool leaves one pixel, the tail replicates 1x1 to 7x7), 45x38 (odd
extents: pools drop a row or a column), 75x67 (tail 2x2), 299x331 (tail 9x10: uneven,
overlapping bins), 480x544 once (tail 15x17: bins of 3 and 4).
Logits and taps are held to the suite's fp32-GEMM-class bound against float64:
max|got - want| <= FEATURE_CLASS x max|want| per tensor.  The tests print the measured multiple
(`VGG ...` lines); DESIGN 4.30 quotes the worst.
"""
import io

import numpy
import pytest
import torch
from torch.utils import data

import vggref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, exemplars, hip, synthetic
from oracle import exemplars_oracle as E

pytestmark = pytest.mark.gpu

PREFIX = 'encoder.encoder.model.'
PRECISIONS = ('f32', 'split_f16')
SEED, HIDDEN, CLASSES, N_IMAGES = 83, 72, 10, 5
GEOS = ((32, 32), (45, 38), (75, 67), (299, 331))
MODELS = (('vgg11', 8), ('vgg13', 8), ('vgg16', 8), ('vgg19', 8), ('vgg16', 16), ('vgg19', 16),
          ('vgg16', 32))


def trunk_sd(sd, config):
    """torchvision's `features.N` under the library's `vgg.B.J` names."""
    out = {}
    for b, block in enumerate(vggref.conv_indices(config)):
        for j, index in enumerate(block):
            for leaf in ('weight', 'bias'):
                out[f'{PREFIX}vgg.{b + 1}.{j}.{leaf}'] = sd[f'features.{index}.{leaf}']
    return out


def head_of(sd):
    return [sd[f'classifier.{i}.{leaf}'] for i in (0, 3, 6) for leaf in ('weight', 'bias')]


def make_context(sd, config, head=True):
    trunk = trunk_sd(sd, config)
    return hip.Context(hip.make_dims(trunk, 1), trunk, torch.device('cuda'),
                       vgg_head=head_of(sd) if head else None)


def model_sd(config, width, hidden=HIDDEN):
    return vggref.make_state_dict(SEED + width, config, width, hidden, CLASSES)


def pictures(geo, n=N_IMAGES):
    return vggref.make_images(SEED, n, geo)


def ratio_of(got, want):
    scale = float(want.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    if scale == 0.0:
        assert err == 0.0
        return 0.0
    return err / scale


@pytest.fixture(scope='module')
def want64():
    """float64 (logits, taps) per (config, width, geometry, n, units), computed once."""
    cache = {}

    def get(config, width, geo, n=N_IMAGES, units=(), hidden=HIDDEN):
        key = (config, width, geo, n, tuple(units), hidden)
        if key not in cache:
            cache[key] = vggref.forward(pictures(geo, n).double(),
                                        model_sd(config, width, hidden), units)
        return cache[key]

    return get


@pytest.fixture(scope='module')
def contexts():
    made = {}

    def get(config, width):
        if (config, width) not in made:
            made[config, width] = make_context(model_sd(config, width), config)
        ctx = made[config, width]
        ctx.set_ablation([])
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


def check_against(ctx, tag, images, want_logits, want_taps, width):
    """classify + the five taps of `images` against float64; returns {tensor: ratio}."""
    n, _, h, w = images.shape
    got = ctx.activations(images, range(5))
    shapes = hip.level_shapes(hip.TRUNK_VGG, width, h, w)
    ratios = {}
    for level in range(5):
        assert got[level].dtype == torch.float32
        assert tuple(got[level].shape) == (n,) + shapes[level] == tuple(want_taps[level].shape)
        assert not bool(torch.signbit(got[level]).any()), (tag, level)   # zeros are +0
        ratios[f'level{level}'] = ratio_of(got[level], want_taps[level])
    logits = ctx.classify(images)
    assert tuple(logits.shape) == tuple(want_logits.shape)
    ratios['logits'] = ratio_of(logits, want_logits)
    for key, ratio in ratios.items():
        print(f'VGG {tag} {h}x{w} {key}: {ratio / FEATURE_CLASS:.3f} x bound')
    return ratios


# ---- 1. classify and taps against float64 ----------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config,width', MODELS)
def test_logits_and_taps_against_float64(contexts, want64, config, width, precision):
    ctx = contexts(config, width)
    ctx.set_precision(precision)
    worst = {}
    for geo in GEOS:
        ratios = check_against(ctx, f'{config} width {width} {precision}', pictures(geo),
                               *want64(config, width, geo), width)
        for key, ratio in ratios.items():
            worst[key] = max(worst.get(key, 0.0), ratio)
    assert ctx.status() == 0
    for key, ratio in worst.items():
        assert ratio <= FEATURE_CLASS, (config, width, precision, key, ratio)
    # which convs multiplied split operands: from the first one whose input width is a
    # multiple of 32 behind a pool (or behind the first conv's kernel) on
    trace = ctx.vgg_trace()
    split_from = {8: (4, 0), 16: (3, 0), 32: (1, 1)}[width]
    for (block, conv), (launches, split) in trace.items():
        assert launches == 1, (block, conv, launches)
        assert split == int(precision == 'split_f16' and (block, conv) >= split_from), (block, conv)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_large_image_once(contexts, want64, precision):
    """480 x 544: the tail's input is 15 x 17, bins of 3 and 4 pooled pixels."""
    ctx = contexts('vgg11', 8)
    ctx.set_precision(precision)
    geo = (480, 544)
    ratios = check_against(ctx, f'vgg11 width 8 {precision}', pictures(geo, 2),
                           *want64('vgg11', 8, geo, 2), 8)
    assert ctx.status() == 0
    for key, ratio in ratios.items():
        assert ratio <= FEATURE_CLASS, (precision, key, ratio)


# ---- 2. full width once ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def full_width():
    sd = vggref.make_state_dict(SEED, 'vgg16', 64, 128, CLASSES)
    images = pictures((224, 224), 2)
    return sd, images, vggref.forward(images.double(), sd)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_full_width_once(full_width, precision):
    sd, images, (want_logits, want_taps) = full_width
    ctx = make_context(sd, 'vgg16')
    try:
        ctx.set_precision(precision)
        ratios = check_against(ctx, f'vgg16 width 64 {precision}', images, want_logits,
                               want_taps, 64)
        assert ctx.status() == 0
        for key, ratio in ratios.items():
            assert ratio <= FEATURE_CLASS, (precision, key, ratio)
        # conv1_2 (and every conv behind it) ran on split operands in the split mode
        trace = ctx.vgg_trace()
        assert len(trace) == 13 and trace[1, 0] == (1, 0)
        for key, (launches, split) in trace.items():
            if key != (1, 0):
                assert (launches, split) == (1, int(precision == 'split_f16')), key
    finally:
        ctx.close()


# ---- 3. tap subsets ----------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config,width', (('vgg11', 8), ('vgg16', 16), ('vgg16', 32)))
def test_tap_subsets_equal_the_full_walk(contexts, config, width, precision):
    ctx = contexts(config, width)
    ctx.set_precision(precision)
    images = pictures((45, 38))
    full = ctx.activations(images, range(5))
    assert all(launches == 1 for launches, _ in ctx.vgg_trace().values())
    for subset in ([3, 1], [4], [0], [2, 0, 1]):
        got = ctx.activations(images, subset)
        assert list(got) == subset
        for level in subset:
            assert torch.equal(got[level], full[level]), (subset, level)
        # nothing behind the highest level was launched
        for (block, _), (launches, _) in ctx.vgg_trace().items():
            assert launches == int(block <= max(subset) + 1), (subset, block)
    by_name = ctx.activations(images, [ctx.ablation_levels[2]])
    assert torch.equal(by_name[ctx.ablation_levels[2]], full[2])
    assert ctx.ablation_levels == vggref.LAYERS[config]


# ---- 4. batch invariance -----------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config,width', (('vgg13', 8), ('vgg16', 32)))
def test_a_batch_gives_the_bits_of_its_images(contexts, config, width, precision):
    ctx = contexts(config, width)
    ctx.set_precision(precision)
    images = pictures((75, 67))
    together = ctx.classify(images)
    taps = ctx.activations(images, [0, 4])
    for i in range(len(images)):
        assert torch.equal(ctx.classify(images[i:i + 1]), together[i:i + 1]), i
        alone = ctx.activations(images[i:i + 1], [0, 4])
        assert torch.equal(alone[0], taps[0][i:i + 1]) and torch.equal(alone[4], taps[4][i:i + 1])


# ---- 5. ablation and the sweep -----------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config,width', (('vgg11', 8), ('vgg16', 16), ('vgg16', 32)))
def test_ablation_and_sweep(contexts, want64, config, width, precision):
    ctx = contexts(config, width)
    ctx.set_precision(precision)
    geo = (45, 38)
    images = pictures(geo)
    ch = vggref.channels(width)
    base = [(0, 1), (0, ch[0] - 1), (1, 5), (2, ch[2] - 2), (3, 7), (4, 0), (4, ch[4] - 1), (3, 7)]
    want_logits, want_taps = want64(config, width, geo, units=base)
    ctx.set_ablation(base)
    ratios = check_against(ctx, f'{config} width {width} {precision} ablated', images,
                           want_logits, want_taps, width)
    for key, ratio in ratios.items():
        assert ratio <= FEATURE_CLASS, (config, width, precision, key, ratio)
    taps = ctx.activations(images, range(5))
    clean = want64(config, width, geo)[1]
    for level, unit in base:
        gone = taps[level][:, unit]
        assert not bool(gone.any()) and not bool(torch.signbit(gone).any())   # exactly +0
    # (the set is live: some of its units fire on these images without it)
    assert sum(bool(clean[level][:, unit].any()) for level, unit in base) >= 3
    # the sweep's rows are the single calls, bit for bit
    units = [(level, u) for level in range(5) for u in (0, ch[level] - 1)]
    targets = want_logits.argmax(dim=1)
    swept, correct = ctx.classify_sweep(images, units, targets)
    rows = []
    for unit in units:
        ctx.set_ablation([*base, unit])
        rows.append(ctx.classify(images, return_logits=False))
    rows = torch.stack(rows)
    assert torch.equal(swept, rows)
    assert torch.equal(correct.cpu().long(), (rows.cpu() == targets).sum(dim=1))
    # layer names do what level numbers do
    names = ctx.ablation_levels
    ctx.set_ablation(base)
    by_number = ctx.classify(images)
    ctx.set_ablation([(names[level], unit) for level, unit in base])
    assert torch.equal(ctx.classify(images), by_number)
    ctx.set_ablation([])
    assert ctx.status() == 0


# ---- 6. predictions ----------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config,width', MODELS)
def test_predictions_are_the_float64_argmax(contexts, want64, config, width, precision):
    ctx = contexts(config, width)
    ctx.set_precision(precision)
    for geo in GEOS[:3]:
        want_logits = want64(config, width, geo)[0]
        top = want_logits.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
        # (the seed leaves no image out: every top-two gap is clear of the bound)
        assert bool((gap > 2 * FEATURE_CLASS * float(want_logits.abs().max())).all()), (geo, gap)
        got = ctx.classify(pictures(geo), return_logits=False)
        assert got.dtype == torch.int64
        assert torch.equal(got.cpu(), want_logits.argmax(dim=1))


# ---- 7. refusals (argument checks that return before any launch) -------------------------------
def test_refusals(contexts):
    ctx = contexts('vgg16', 8)
    ctx.set_precision('f32')
    images = pictures((32, 32))
    lib = hip.load_library()
    with pytest.raises(ValueError, match='31x32 is too small'):
        ctx.classify(images[:, :, :31])
    with pytest.raises(ValueError, match='too small'):
        ctx.classify_sweep(images[:, :, :, :31], [(0, 0)])
    with pytest.raises(ValueError, match='15x16 is too small for VGG level 4'):
        ctx.activations(images[:, :, :15, :16], [4])
    assert tuple(ctx.activations(images[:, :, :15, :16], [3])[3].shape) == (N_IMAGES, 64, 1, 2)
    assert tuple(ctx.activations(images[:, :, :16, :16], [4])[4].shape) == (N_IMAGES, 64, 1, 1)
    ws = ctx._classify_ws(N_IMAGES, 31, 32, 0)
    logits = torch.empty(N_IMAGES, CLASSES, device='cuda')
    dev = images[:, :, :31].contiguous().cuda()
    assert lib.milan_classify(ctx._h, dev.data_ptr(), N_IMAGES, 31, 32, logits.data_ptr(), None,
                              ws.data_ptr(), ws.numel(), None) == hip.ERR_SHAPE
    ctx.set_precision('f16')
    with pytest.raises(ValueError, match='fast f16'):
        ctx.classify(images)
    with pytest.raises(ValueError, match='fast f16'):
        ctx.activations(images, [0])
    ctx.set_precision('f32')
    g = torch.Generator().manual_seed(9)
    exemplar_images = torch.randint(256, (2, 3, 96, 96), generator=g, dtype=torch.uint8)
    masks = torch.ones(2, 1, 96, 96, dtype=torch.uint8)
    with pytest.raises(ValueError, match='no encoder config'):
        ctx.encode(exemplar_images, masks)
    with pytest.raises(ValueError, match='level 5'):
        ctx.activations(images, [5])
    with pytest.raises(IndexError):
        ctx.set_ablation([(4, 64)])
    # the heads: a wrong width, and each setter on the other kind of context
    sd = model_sd('vgg16', 8)
    head = head_of(sd)
    with pytest.raises(ValueError, match='64 x 49'):
        ctx.set_vgg_head(head[0][:, :-49].contiguous(), *head[1:])
    with pytest.raises(ValueError, match='not AlexNet'):
        ctx.set_alexnet_head(*head)
    assert torch.equal(ctx.classify(images), ctx.classify(images))   # (the head is as it was)
    # a headless context taps and ablates, and says what classify lacks
    bare = make_context(sd, 'vgg16', head=False)
    bare.set_precision('f32')
    bare.set_ablation([(2, 1)])
    ctx.set_ablation([(2, 1)])
    assert torch.equal(bare.activations(images, [4])[4], ctx.activations(images, [4])[4])
    with pytest.raises(RuntimeError, match='milan_set_vgg_head'):
        bare.classify(images)
    ws = bare._classify_ws(N_IMAGES, 32, 32, 0)
    full = images.cuda()
    assert lib.milan_classify(bare._h, full.data_ptr(), N_IMAGES, 32, 32, logits.data_ptr(), None,
                              ws.data_ptr(), ws.numel(), None) == hip.ERR_STATE
    bare.close()
    ctx.set_ablation([])
    # structure from the keys: a gap in J, a block too many, a wrong width
    trunk = trunk_sd(sd, 'vgg16')
    gap = {k.replace('vgg.3.2.', 'vgg.3.3.'): v for k, v in trunk.items()}
    with pytest.raises(ValueError, match='without a gap'):
        hip.Context(hip.make_dims(gap, 1), gap, torch.device('cuda'))
    six = dict(trunk)
    six[PREFIX + 'vgg.6.0.weight'] = trunk[PREFIX + 'vgg.5.0.weight']
    with pytest.raises(ValueError, match='not a VGG key'):
        hip.Context(hip.make_dims(six, 1), six, torch.device('cuda'))
    wide = dict(trunk)
    wide[PREFIX + 'vgg.4.0.weight'] = torch.zeros(32, 32, 3, 3)
    wide[PREFIX + 'vgg.4.0.bias'] = torch.zeros(32)
    with pytest.raises(ValueError, match='vgg.4.0'):
        hip.Context(hip.make_dims(wide, 1), wide, torch.device('cuda'))
    # milan_set_vgg_head on another kind of context
    rsd = {PREFIX + k: v for k, v in synthetic.resnet_state_dict('resnet18', seed=1,
                                                                 width=8).items()}
    resnet = hip.Context(hip.make_dims(rsd, 1, blocks=(2, 2, 2, 2)), rsd, torch.device('cuda'))
    with pytest.raises(ValueError, match='not a VGG'):
        resnet.set_vgg_head(*head)
    resnet.close()


# ---- 8. VGGClassifier end to end ---------------------------------------------------------------
def classifier(config, width, precision):
    model = classifiers.VGGClassifier(config, CLASSES, width, HIDDEN, precision=precision)
    model.load_state_dict(model_sd(config, width), strict=True)
    return model.eval().to('cuda')


@pytest.mark.parametrize('precision', ('auto', 'f32'))
def test_classifier_module_runs_natively(precision):
    model = classifier('vgg16', 16, precision)
    images = pictures((75, 67)).cuda()
    with torch.enable_grad():
        assert not model.runs_natively(images)
    eager = model.forward_eager(images).detach()
    eager_taps = model.activations(images, model.layers)   # (grad is on: the hook path)
    with torch.no_grad():
        assert model.runs_natively(images)
        got = model(images)
        taps = model.activations(images, model.layers)
        ratio = ratio_of(got, eager.cpu().double())
        print(f'VGG classifier {precision} logits vs eager: {ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS
        for layer in model.layers:
            assert ratio_of(taps[layer], eager_taps[layer].cpu().double()) <= FEATURE_CLASS
        # ablations.ablated: the native set against the eager hook path
        with ablations.ablated(model, [('features.7', 3)]):
            native = model(images)
            tap = model.activations(images, 'features.7')['features.7']
        assert not bool(tap[:, 3].any())
    with ablations.ablated(model, [('features.7', 3)]):
        hooked = model(images).detach()   # (grad is on: forward hooks)
    assert ratio_of(native, hooked.cpu().double()) <= FEATURE_CLASS
    assert ratio_of(native, eager.cpu().double()) > FEATURE_CLASS   # the unit matters
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


def test_places_keyed_checkpoint_classifies_natively(want64):
    sd = model_sd('vgg16', 16)
    names = [f'conv{b + 1}_{j + 1}' for b, block in enumerate(vggref.conv_indices('vgg16'))
             for j in range(len(block))]
    indices = [i for block in vggref.conv_indices('vgg16') for i in block]
    places = {}
    for name, index in zip(names, indices):
        for leaf in ('weight', 'bias'):
            places[f'features.{name}.{leaf}'] = sd[f'features.{index}.{leaf}']
    for name, index in (('fc6', 0), ('fc7', 3), ('fc8a', 6)):
        for leaf in ('weight', 'bias'):
            places[f'classifier.{name}.{leaf}'] = sd[f'classifier.{index}.{leaf}']
    model = classifiers.VGGClassifier('vgg16', CLASSES, 16, HIDDEN, precision='auto')
    model.load_state_dict(classifiers.rekey_vgg16_places(places), strict=True)
    model.eval().to('cuda')
    geo = (75, 67)
    with torch.no_grad():
        got = model(pictures(geo).cuda())
    assert ratio_of(got, want64('vgg16', 16, geo)[0]) <= FEATURE_CLASS


def test_dissect_vgg(tmp_path):
    """exemplars.discriminative on features.7 against the oracle's `compute` fed the layer's
    activations for the same batches (test_gpu_places.py's arrangement)."""
    model = classifiers.VGGClassifier('vgg16', CLASSES, 8, HIDDEN, precision='f32')
    model.load_state_dict(model_sd('vgg16', 8), strict=True)
    model.eval()
    g = torch.Generator().manual_seed(2307)
    dataset = data.TensorDataset(torch.rand(23, 3, 48, 64, generator=g))
    layer = 'features.7'
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    torch.manual_seed(31)
    topk, rq = exemplars.discriminative(model, dataset, layer=layer, image_size=48,
                                        num_workers=0, save_viz=False, results_dir=tmp_path,
                                        **kwargs)

    def hiddens(images):
        with torch.no_grad():
            images = images.cuda()
            assert model.runs_natively(images)
            return model.activations(images, layer)[layer].cpu()

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
    assert want['ids'].shape == (16, 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
