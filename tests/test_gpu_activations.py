"""GPU tests of the activation taps on the HIP trunk (milan_activations,
hip.Context.activations, classifiers.ResNetClassifier.activations) and of dissecting a
ResNetClassifier with exemplars.discriminative.

The trunks, images and ablation sets are those of tests/golden/reference_goldens_ablations.*
(width 8, 12 images at 64x64, 33x47 and 7x9: level extents from 32x32 down to 1x1, P = 1, 2,
4, 6, 9, 20, 30, 108, 408 ... against the layout kernel's 64-pixel x 32-channel tile, C = 8 ..
256).  Every tap is held to the suite's fp32-GEMM-class bound against tests/actref.py in
float64: max|got - want| <= FEATURE_CLASS x max|want| per level.

The tests print the measured multiple of the bound per level (`ACT ...` lines); DESIGN 4.22
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

import ablref
import actref
from featclass import FEATURE_CLASS
from milan_amd import classifiers, exemplars, hip, synthetic
from oracle import exemplars_oracle as E

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
PREFIX = 'encoder.encoder.model.'
CONFIGS = ('resnet18', 'resnet50')
PRECISIONS = ('f32', 'split_f16')
LAYERS = actref.LAYERS
SETS = ('none', 'two_stages', 'layer3_thirds')


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
    """float64 taps of every (config, geometry, set), computed once and left alone."""
    tensors, meta = gold
    cache = {}

    def get(config, geo, name):
        key = (config, geo, name)
        if key not in cache:
            case = [tuple(u) for u in meta['configs'][config]['cases'][name]]
            cache[key] = actref.forward(tensors[f'images.{geo[0]}x{geo[1]}'].double(),
                                        ablref.state_dict(config, tensors, meta),
                                        synthetic.RESNET_BLOCKS[config], case)[1]
        return cache[key]

    return get


def geometries(meta):
    return [tuple(g) for g in meta['geometries']]


def use(contexts, config, precision):
    ctx = contexts[config]
    ctx.set_precision(precision)
    ctx.set_ablation([])
    return ctx


def check_taps(got, want, tag):
    """The float64 bound per level; channels that are exactly zero stay exactly zero.
    Returns the worst multiple of the bound."""
    worst = 0.0
    for layer in LAYERS:
        g, w = got[layer].cpu(), want[layer]
        assert g.dtype == torch.float32 and g.shape == w.shape, (tag, layer, g.shape, w.shape)
        ratio = float((g.double() - w).abs().max() / w.abs().max())
        worst = max(worst, ratio)
        print(f'ACT {tag} {layer}: {ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS, (tag, layer, ratio)
        dead = (w == 0).all(dim=3).all(dim=2).all(dim=0)
        assert not g[:, dead].any(), (tag, layer)
    return worst


# ---- 1. against float64 -------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config', CONFIGS)
def test_taps_against_float64(gold, contexts, want64, config, precision):
    tensors, meta = gold
    ctx = use(contexts, config, precision)
    worst = 0.0
    for geo in geometries(meta):
        images = tensors[f'images.{geo[0]}x{geo[1]}']
        for name in SETS:
            case = [tuple(u) for u in meta['configs'][config]['cases'][name]]
            ctx.set_ablation(case)
            got = ctx.activations(images, LAYERS)   # all five levels in ONE call
            assert tuple(got) == LAYERS
            worst = max(worst, check_taps(got, want64(config, geo, name),
                                          f'{config} {precision} {geo[0]}x{geo[1]} {name}'))
            for layer, unit in case:
                assert not got[layer][:, unit].any()
    ctx.set_ablation([])
    print(f'ACT {config} {precision}: worst {worst / FEATURE_CLASS:.3f} x bound')


# ---- 2. exact properties (f32) ------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS)
def test_exact_properties_f32(gold, contexts, config):
    tensors, meta = gold
    ctx = use(contexts, config, 'f32')
    channels = ablref.level_channels(config, meta['width'])
    base = [(1, 2), (3, 0), (0, 1)]
    for geo in geometries(meta):
        images = tensors[f'images.{geo[0]}x{geo[1]}'].cuda()
        ctx.set_ablation(base)
        logits = ctx.classify(images)
        every = ctx.activations(images, [0, 1, 2, 3, 4])
        # one call for all = one call each; names and numbers are the same levels
        for level in range(5):
            one = ctx.activations(images, [level])
            assert tuple(one) == (level,)
            assert torch.equal(one[level], every[level]), (geo, level)
            assert torch.equal(ctx.activations(images, [LAYERS[level]])[LAYERS[level]],
                               every[level])
        # another order, a subset
        other = ctx.activations(images, [3, 0, 4, 2, 1])
        assert tuple(other) == (3, 0, 4, 2, 1)
        for level in range(5):
            assert torch.equal(other[level], every[level]), (geo, level)
        some = ctx.activations(images, [2, 0])
        assert torch.equal(some[2], every[2]) and torch.equal(some[0], every[0])
        # scratch reuse does not leak into classify
        assert torch.equal(ctx.classify(images), logits)
        # one more unit u at level L: its channel is +0, its level's other channels and every
        # level below are bitwise what they were
        for level in range(5):
            unit = channels[level] - 3
            assert (level, unit) not in base
            ctx.set_ablation([*base, (level, unit)])
            got = ctx.activations(images, [0, 1, 2, 3, 4])
            zeros = got[level][:, unit]
            assert not zeros.any() and not torch.signbit(zeros).any(), (geo, level)
            keep = torch.arange(channels[level], device='cuda') != unit
            assert torch.equal(got[level][:, keep], every[level][:, keep]), (geo, level)
            for below in range(level):
                assert torch.equal(got[below], every[below]), (geo, level, below)
        ctx.set_ablation([])


@pytest.mark.parametrize('config', CONFIGS)
def test_activations_do_not_leak_into_encode(gold, contexts, config):
    tensors, meta = gold
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (6, 3, 33, 47), dtype=torch.uint8, generator=g)
    masks = (torch.rand(6, 1, 33, 47, generator=g) > 0.5).to(torch.uint8)
    floats = tensors['images.33x47']
    for precision in PRECISIONS:
        ctx = use(contexts, config, precision)
        before = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        ctx.set_ablation([('conv1', 0), ('layer2', 3)])
        taps = ctx.activations(floats, LAYERS)
        during = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        ctx.set_ablation([])
        after = (ctx.encode(images, masks), ctx.encode_spatial(images, masks))
        for a, b, c in zip(before, during, after):
            assert torch.equal(a, b) and torch.equal(a, c)
            assert float(a.abs().max()) > 0
        assert float(taps['layer4'].abs().max()) > 0


# ---- 3. the split format at width 32 ------------------------------------------------------
# (test_gpu_ablations.py: width 32 is the smallest trunk on which split_f16 really runs -- the
# pixel-pair stem, the split stem tail, split level tensors)
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
                want = actref.forward(images.double(), sd, blocks, units)[1]
                got = {}
                for precision in PRECISIONS:
                    ctx.set_precision(precision)
                    ctx.set_ablation(units)
                    got[precision] = ctx.activations(images, LAYERS)
                    check_taps(got[precision], want,
                               f'{config} width 32 {precision} {geo[0]}x{geo[1]} {name}')
                # level 0 is the raw conv output: both signs, no ReLU, no scale left in it
                raw = got['split_f16']['conv1']
                assert float(raw.min()) < 0 < float(raw.max())
                assert float(want['conv1'].min()) < 0
                # levels 1..4 were decoded from split tensors: same class of error, other bits
                assert any(not torch.equal(got['f32'][layer], got['split_f16'][layer])
                           for layer in LAYERS[1:])
                for layer in LAYERS[1:]:
                    assert float(got['split_f16'][layer].min()) >= 0
    finally:
        ctx.close()


# ---- 4. sub-batches -----------------------------------------------------------------------
SUB_SCRIPT = r'''
import hashlib, sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import torch
import ablref
from milan_amd import hip, synthetic
PREFIX = 'encoder.encoder.model.'
tensors, meta = ablref.load_goldens()
sd = {{PREFIX + k: v for k, v in ablref.state_dict('resnet18', tensors, meta).items()}}
c = hip.Context(hip.make_dims(sd, 1, blocks=synthetic.RESNET_BLOCKS['resnet18']), sd,
                hip.require_device('cuda'))
c.set_precision('f32')
c.set_ablation([(0, 1), (2, 5)])
got = c.activations(tensors['images.33x47'][:7], [4, 0, 2])
digest = hashlib.sha256()
for level in (4, 0, 2):
    digest.update(got[level].cpu().numpy().tobytes())
print('SHA', digest.hexdigest())
c.close()
'''


def test_sub_batches(gold, contexts, tmp_path):
    """MILAN_ENC_SUB is cached per process: one fresh child walks 7 images in passes of
    3 + 3 + 1; this process walks them in one.  The same bits."""
    tensors, meta = gold
    ctx = use(contexts, 'resnet18', 'f32')
    ctx.set_ablation([(0, 1), (2, 5)])
    got = ctx.activations(tensors['images.33x47'][:7], [4, 0, 2])
    ctx.set_ablation([])
    digest = hashlib.sha256()
    for level in (4, 0, 2):
        digest.update(got[level].cpu().numpy().tobytes())
    script = tmp_path / 'sub.py'
    script.write_text(SUB_SCRIPT.format(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd'),
                                        tests=str(REPO / 'tests')))
    env = dict(os.environ, MILAN_ENC_SUB='3')
    out = subprocess.run(['timeout', '-k', '10', '120', sys.executable, str(script)], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert f'SHA {digest.hexdigest()}' in out.stdout, out.stdout


# ---- 5. errors ----------------------------------------------------------------------------
def test_errors(gold, contexts):
    tensors, meta = gold
    images = tensors['images.7x9']
    ctx = use(contexts, 'resnet18', 'f32')
    with pytest.raises(ValueError, match='not one of 0..4'):
        ctx.activations(images, [5])
    with pytest.raises(ValueError, match='not one of 0..4'):
        ctx.activations(images, [1, -1])
    with pytest.raises(ValueError, match='twice'):
        ctx.activations(images, [2, 4, 2])
    with pytest.raises(ValueError, match='twice'):
        ctx.activations(images, ['layer2', 2])
    with pytest.raises(ValueError, match='no native tap'):
        ctx.activations(images, ['fc'])
    with pytest.raises(ValueError):
        ctx.activations(images, [])
    ctx.set_precision('f16')
    with pytest.raises(ValueError, match='fast f16'):
        ctx.activations(images, [1])
    ctx.set_precision('f32')
    # a workspace that is too small
    lib = hip.load_library()
    need = int(lib.milan_activations_workspace_bytes(ctx._h, 12, 7, 9))
    assert need > 256
    import ctypes
    dev = images.cuda()
    out = torch.empty(12, 8, 4, 5, device='cuda')
    small = torch.empty(need // 2, dtype=torch.uint8, device='cuda')
    levels = (ctypes.c_int32 * 1)(0)
    outs = (ctypes.c_void_p * 1)(out.data_ptr())
    with torch.cuda.device(ctx.device):
        code = lib.milan_activations(ctx._h, dev.data_ptr(), 12, 7, 9, levels, 1, outs,
                                     small.data_ptr(), small.numel(), None)
    assert code == hip.ERR_WORKSPACE
    torch.cuda.synchronize()
    # a context without a head: no head runs, the taps come out
    sd = {PREFIX + k: v for k, v in synthetic.resnet_state_dict(
        'resnet18', seed=1, width=8, with_fc=False).items()}
    bare = hip.Context(hip.make_dims(sd, 1, blocks=(2, 2, 2, 2)), sd, torch.device('cuda'))
    plain = {k[len(PREFIX):]: v for k, v in sd.items()}
    plain['fc.weight'], plain['fc.bias'] = torch.zeros(1, 64), torch.zeros(1)
    want = actref.forward(images.double(), plain, (2, 2, 2, 2))[1]
    check_taps(bare.activations(images, LAYERS), want, 'no head 7x9')
    bare.close()
    # AlexNet
    sd = {PREFIX + k: v for k, v in synthetic.alexnet_state_dict(seed=2, width=8).items()}
    alex = hip.Context(hip.make_dims(sd, 1), sd, torch.device('cuda'))
    with pytest.raises(ValueError, match='ResNet'):
        alex.activations(tensors['images.64x64'], [0])
    alex.close()


# ---- 6. dissect end to end ----------------------------------------------------------------
def dissect_model(gold):
    tensors, meta = gold
    config = 'resnet18'
    model = classifiers.ResNetClassifier(config, num_classes=meta['configs'][config]['classes'],
                                         width=meta['width'], precision='f32')
    model.load_state_dict(ablref.state_dict(config, tensors, meta), strict=True)
    return model.eval()


def dissect_dataset():
    g = torch.Generator().manual_seed(2305)
    return data.TensorDataset(torch.rand(23, 3, 33, 47, generator=g))


def dissect(model, dataset, layer, tmp_path, source):
    """exemplars.discriminative against the oracle's `compute` fed `source(images)` =
    the layer's activations for the same batches.  The oracle sorts the quantile summary
    stably, which is the order the HIP sketch defines (test_gpu_exemplars.py)."""
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    torch.manual_seed(31)
    topk, rq = exemplars.discriminative(model, dataset, layer=layer, image_size=33,
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
    ids_csv = numpy.loadtxt(out / 'ids.csv', delimiter=',', dtype=numpy.int64, ndmin=2)
    assert (ids_csv == want['ids'].numpy()).all()
    text = io.StringIO()
    numpy.savetxt(text, want['activations'].numpy(), delimiter=',', fmt='%.5e')
    assert (out / 'activations.csv').read_text() == text.getvalue()
    assert torch.equal(rq.quantiles(.9).cpu().reshape(-1), want['levels'].reshape(-1))
    return want


@pytest.mark.parametrize('layer', LAYERS)
def test_dissect_resnet_classifier(gold, layer, tmp_path):
    model = dissect_model(gold)
    dataset = dissect_dataset()

    def source(images):
        with torch.no_grad():
            assert model.runs_natively(images)
            return model.activations(images, layer)[layer]

    want = dissect(model, dataset, layer, tmp_path, source)
    channels = ablref.level_channels('resnet18', 8)[LAYERS.index(layer)]
    assert want['ids'].shape == (channels, 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


def test_dissect_a_layer_outside_the_taps(gold, tmp_path):
    """'layer2.0.conv1' has no native tap: the eager forward runs and its hook fires."""
    model = dissect_model(gold)
    dataset = dissect_dataset()
    layer = 'layer2.0.conv1'

    def source(images):
        with torch.no_grad():
            x = model.maxpool(model.relu(model.bn1(model.conv1(images))))
            return model.layer2[0].conv1(model.layer1(x))

    want = dissect(model, dataset, layer, tmp_path, source)
    assert want['ids'].shape == (16, 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
