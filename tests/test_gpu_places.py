"""GPU tests of the Places365 AlexNet on the HIP trunk (MILAN_TRUNK_ALEXNET_PLACES): grouped
convs as one launch against the per-group baseline, the LRN kernel, classify / classify_sweep /
activations, `classifiers.PlacesAlexNetClassifier` and `OldResNet152` under
exemplars.discriminative.

Seeded models (tests/placesref.py), hidden 72, 10 classes, 5 images:
  width 8   channels 24 / 64 / 96 / 96 / 64, per-group Cin 12 / 48 / 48: every grouped level on
            the fp32 kernel, K per group no multiple of 32 (the per-group Kp padding is live);
            conv3 reads split operands and writes fp32 in the split mode
  width 16  48 / 128 / 192 / 192 / 128, per-group Cin 24 / 96 / 96: conv4 and conv5 on the split
            kernels (N per group 96: the 128-column tile; 64: the 64-column tile)
  width 32  the reference's widths once (hidden 128, 3 images): N per group 192 / 128, conv2
            with Cin 48 per group in fp32
Logits and taps are held to the suite's fp32-GEMM-class bound against placesref in float64:
max|got - want| <= FEATURE_CLASS x max|want| per tensor.  The tests print the measured multiple
(`PLACES ...` / `LRN ...` lines); DESIGN 4.27 quotes the worst.
"""
import hashlib
import io
import json
import os
import pathlib
import subprocess
import sys

import numpy
import pytest
import torch
from torch.utils import data

import actref
import placesref
from featclass import FEATURE_CLASS
from splitfmt import from_split, to_split
from milan_amd import classifiers, exemplars, hip, synthetic
from oracle import exemplars_oracle as E

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
PREFIX = 'encoder.encoder.model.'
PRECISIONS = ('f32', 'split_f16')
LAYERS = placesref.LAYERS
SEED, HIDDEN, CLASSES, N_IMAGES = 71, 72, 10, 5
CLASSIFY_GEOS = ((227, 227), (229, 228))
TAP_GEOS = ((67, 75), (99, 131))
LRN = placesref.LRN


def make_context(sd, head=True, lrn=False):
    trunk = {PREFIX + k: v for k, v in sd.items() if k.startswith('conv')}
    head = ([sd[f'{fc}.{part}'] for fc in ('fc6', 'fc7', 'fc8') for part in ('weight', 'bias')]
            if head else None)
    ctx = hip.Context(hip.make_dims(trunk, 1), trunk, torch.device('cuda'), alexnet_head=head)
    if lrn:
        ctx.set_alexnet_lrn(*LRN)
    return ctx


def model_sd(width, split_groups=True):
    return placesref.make_state_dict(SEED + width, width, HIDDEN, CLASSES, split_groups)


def pictures(geo, n=N_IMAGES):
    return placesref.make_images(SEED, n, geo)


def ratio_of(got, want):
    scale = float(want.abs().max())
    err = float((got.cpu().double() - want).abs().max())
    if scale == 0.0:
        assert err == 0.0
        return 0.0
    return err / scale


@pytest.fixture(scope='module')
def want64():
    """float64 (logits, taps) per (width, geometry, lrn, case name), computed once."""
    cache = {}

    def get(width, geo, lrn=False, case=()):
        key = (width, geo, lrn, tuple(case))
        if key not in cache:
            cache[key] = placesref.forward(pictures(geo).double(), model_sd(width), case,
                                           include_lrn=lrn)
        return cache[key]

    return get


@pytest.fixture(scope='module')
def contexts():
    made = {}

    def get(width, lrn=False):
        if (width, lrn) not in made:
            made[width, lrn] = make_context(model_sd(width), lrn=lrn)
        ctx = made[width, lrn]
        ctx.set_ablation([])
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


# ---- 1. classify and taps against float64 ----------------------------------------------------
@pytest.mark.parametrize('lrn', (False, True))
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('width', (8, 16))
def test_logits_and_taps_against_float64(contexts, want64, width, precision, lrn):
    ctx = contexts(width, lrn)
    ctx.set_precision(precision)
    worst = {}
    for geo in CLASSIFY_GEOS + TAP_GEOS:
        images = pictures(geo)
        want_logits, want_taps = want64(width, geo, lrn)
        got = dict(ctx.activations(images, LAYERS))
        wants = list(want_taps.items())
        if geo in CLASSIFY_GEOS:
            got['logits'] = ctx.classify(images)
            wants.append(('logits', want_logits))
        else:
            assert want_logits is None
        for key, want in wants:
            assert got[key].shape == want.shape, (key, got[key].shape, want.shape)
            ratio = ratio_of(got[key], want)
            worst[key] = max(worst.get(key, 0.0), ratio)
            print(f'PLACES width {width} {precision} lrn={int(lrn)} {geo[0]}x{geo[1]} {key}: '
                  f'{ratio / FEATURE_CLASS:.3f} x bound')
            if key != 'logits':
                assert not bool(torch.signbit(got[key]).any()), (geo, key)   # zeros are +0
    assert ctx.status() == 0
    for key, ratio in worst.items():
        assert ratio <= FEATURE_CLASS, (width, precision, lrn, key, ratio)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_full_width_once(precision):
    sd = placesref.make_state_dict(SEED, 32, 128, CLASSES)
    images = pictures((227, 227), 3)
    want_logits, want_taps = placesref.forward(images.double(), sd)
    ctx = make_context(sd)
    try:
        ctx.set_precision(precision)
        got = {'logits': ctx.classify(images), **ctx.activations(images, LAYERS)}
        for key, want in (('logits', want_logits), *want_taps.items()):
            ratio = ratio_of(got[key], want)
            print(f'PLACES width 32 {precision} {key}: {ratio / FEATURE_CLASS:.3f} x bound')
            assert ratio <= FEATURE_CLASS, (precision, key, ratio)
        assert ctx.status() == 0
    finally:
        ctx.close()


# ---- 2. the LRN kernel alone --------------------------------------------------------------------
@pytest.mark.parametrize('split', (False, True))
@pytest.mark.parametrize('beta', (0.75, 0.5))
@pytest.mark.parametrize('local_size', (5, 3))
@pytest.mark.parametrize('channels', (8, 24, 48, 96))
def test_lrn_kernel_against_float64(channels, local_size, beta, split):
    alpha = 0.5   # (large, so that the divisor is far from 1 and the window matters)
    for pixels in (1, 9, 169):
        g = torch.Generator().manual_seed(channels * 1000 + pixels)
        x = torch.randn(pixels, channels, generator=g).abs_() * 3
        if split:
            fed, held = to_split(x)
            got = from_split(hip.lrn(fed.cuda(), local_size, alpha, beta, split=True).cpu())
        else:
            held = x.double()
            got = hip.lrn(x.cuda(), local_size, alpha, beta).cpu().double()
        want = placesref.lrn(held.t().reshape(1, channels, pixels), local_size, alpha, beta)
        want = want.reshape(channels, pixels).t()
        ratio = ratio_of(got, want)
        print(f'LRN C={channels} P={pixels} n={local_size} beta={beta} split={int(split)}: '
              f'{ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS, (channels, pixels, local_size, beta, split, ratio)
        # the edge channels see zeros beyond the ends, and the divisor stays local_size
        half = local_size // 2
        for c in (0, channels - 1):
            lo, hi = max(0, c - half), min(channels, c + half + 1)
            total = (held[:, lo:hi]**2).sum(dim=1)
            edge = held[:, c] / (1 + alpha * total / local_size)**beta
            assert float((got[:, c] - edge).abs().max()) <= FEATURE_CLASS * float(want.abs().max())
            wrong = held[:, c] / (1 + alpha * total / (hi - lo))**beta
            assert float((got[:, c] - wrong).abs().max()) > 100 * FEATURE_CLASS * float(
                want.abs().max())


def test_lrn_arguments():
    x = torch.rand(4, 16, device='cuda')
    for bad in (4, 0, -1, 19):
        with pytest.raises(ValueError, match='local_size'):
            hip.lrn(x, bad, 1e-4, 0.75)
    with pytest.raises(ValueError, match='multiple of 8'):
        hip.lrn(x[:, :12].contiguous(), 5, 1e-4, 0.75)
    # a window of one channel, and the widest the kernel takes
    for size in (1, 17):
        got = hip.lrn(x, size, 0.5, 0.75).cpu().double()
        want = placesref.lrn(x.cpu().double().t().reshape(1, 16, 4), size, 0.5, 0.75)
        assert ratio_of(got, want.reshape(16, 4).t()) <= FEATURE_CLASS


# ---- 3. the grouped launch against one launch per group ---------------------------------------
def launch_digest(width, precision, check=False):
    """sha256 over logits and taps of the seeded model, with an ablation set and the LRN on;
    `check`: the logits are also held to the bound against float64."""
    ctx = make_context(model_sd(width), lrn=True)
    try:
        ctx.set_precision(precision)
        ctx.set_ablation([(1, 3), (3, 5)])
        digest = hashlib.sha256()
        images = pictures((227, 227))
        logits = ctx.classify(images)
        if check:
            want = placesref.forward(images.double(), model_sd(width),
                                     [('conv2', 3), ('conv4', 5)], include_lrn=True)[0]
            assert ratio_of(logits, want) <= FEATURE_CLASS, (width, precision)
        digest.update(logits.cpu().numpy().tobytes())
        for geo in ((227, 227), (99, 131)):
            got = ctx.activations(pictures(geo), LAYERS)
            for layer in LAYERS:
                digest.update(got[layer].cpu().numpy().tobytes())
        assert ctx.status() == 0
        return digest.hexdigest()
    finally:
        ctx.close()


CHILD_SCRIPT = r'''
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import test_gpu_places as T
for width in {widths!r}:
    for precision in T.PRECISIONS:
        print('SHA', width, precision, T.{digest}(width, precision))
'''


def checked_digest(width, precision):
    return launch_digest(width, precision, check=True)


def run_child(tmp_path, digest, env, widths=(8, 16)):
    script = tmp_path / 'child.py'
    script.write_text(CHILD_SCRIPT.format(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd'),
                                          tests=str(REPO / 'tests'), digest=digest,
                                          widths=tuple(widths)))
    out = subprocess.run(['timeout', '-k', '10', '240', sys.executable, str(script)],
                         env=dict(os.environ, **env), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_grouped_launch_equals_per_group_launches(tmp_path):
    """MILAN_GROUP_LAUNCH is read once per process: a fresh child runs every grouped conv as
    `groups` plain launches on offset pointers, this process as one launch.  The same bits.
    Width 64 has 256 output channels per group at conv2 and conv5 and a split conv2: both forms
    stay on the 128-column tile there."""
    assert os.environ.get('MILAN_GROUP_LAUNCH', '1') != '0'
    stdout = run_child(tmp_path, 'launch_digest', {'MILAN_GROUP_LAUNCH': '0'}, (8, 16, 64))
    for width in (8, 16, 64):
        for precision in PRECISIONS:
            assert f'SHA {width} {precision} {launch_digest(width, precision)}' in stdout, stdout


def test_a_launch_without_a_grouped_kernel_runs_per_group(tmp_path):
    """MILAN_PP128=0 sends the 128-column split launches to the lockstep kernel, which has no
    grouped form: the launcher decides that before anything runs and launches group by group.
    The child's logits are held to the bound against float64 (the lockstep kernel multiplies a
    k x k conv in another order: other bits than this process has)."""
    stdout = run_child(tmp_path, 'checked_digest', {'MILAN_PP128': '0'}, (16,))
    again = run_child(tmp_path, 'checked_digest',
                      {'MILAN_PP128': '0', 'MILAN_GROUP_LAUNCH': '0'}, (16,))
    lines = [line for line in stdout.splitlines() if line.startswith('SHA')]
    assert len(lines) == 2 and lines == [l for l in again.splitlines() if l.startswith('SHA')]


@pytest.mark.parametrize('precision', PRECISIONS)
def test_width_64(precision):
    """Twice the reference's width: conv2 has 96 input channels per group and runs split, with
    256 output channels per group, as conv5 has."""
    sd = model_sd(64)
    images = pictures((227, 227), 2)
    want_logits, want_taps = placesref.forward(images.double(), sd)
    ctx = make_context(sd)
    try:
        ctx.set_precision(precision)
        got = {'logits': ctx.classify(images), **ctx.activations(images, LAYERS)}
        for key, want in (('logits', want_logits), *want_taps.items()):
            ratio = ratio_of(got[key], want)
            print(f'PLACES width 64 {precision} {key}: {ratio / FEATURE_CLASS:.3f} x bound')
            assert ratio <= FEATURE_CLASS, (precision, key, ratio)
        assert ctx.status() == 0
    finally:
        ctx.close()


def test_sub_batches(tmp_path):
    """5 images in passes of 2 + 2 + 1 (child, MILAN_ENC_SUB=2) equal one pass."""
    stdout = run_child(tmp_path, 'launch_digest', {'MILAN_ENC_SUB': '2'})
    for width in (8, 16):
        for precision in PRECISIONS:
            assert f'SHA {width} {precision} {launch_digest(width, precision)}' in stdout, stdout


# ---- 4. group wiring --------------------------------------------------------------------------
@pytest.mark.parametrize('width', (8, 16))
def test_groups_do_not_mix(width):
    sd = model_sd(width)
    images = pictures((99, 131))
    ch = placesref.channels(width)
    half = ch[1] // 2
    cut = dict(sd)
    cut['conv2.weight'] = sd['conv2.weight'].clone()
    cut['conv2.weight'][half:] = 0
    whole, zeroed = make_context(sd, head=False), make_context(cut, head=False)
    try:
        for precision in PRECISIONS:
            whole.set_precision(precision)
            zeroed.set_precision(precision)
            a = whole.activations(images, ['conv2'])['conv2']
            b = zeroed.activations(images, ['conv2'])['conv2']
            assert torch.equal(a[:, :half], b[:, :half])
            bias = sd['conv2.bias'][half:].clamp(min=0).cuda()
            assert torch.equal(b[:, half:], bias.view(1, -1, 1, 1).expand_as(b[:, half:]))
            assert not torch.equal(a[:, half:], b[:, half:])
    finally:
        whole.close()
        zeroed.close()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_dense_weights_run_as_groups_of_one(precision):
    sd = model_sd(8, split_groups=False)
    assert sd['conv2.weight'].shape[1] == 24
    images = pictures((227, 227))
    want_logits, want_taps = placesref.forward(images.double(), sd)
    ctx = make_context(sd)
    try:
        ctx.set_precision(precision)
        got = {'logits': ctx.classify(images), **ctx.activations(images, LAYERS)}
        for key, want in (('logits', want_logits), *want_taps.items()):
            assert ratio_of(got[key], want) <= FEATURE_CLASS, (precision, key)
    finally:
        ctx.close()


# ---- 5. ablation -------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('width', (8, 16))
def test_ablation_against_float64(contexts, want64, width, precision):
    ctx = contexts(width)
    ctx.set_precision(precision)
    geo = (227, 227)
    images = pictures(geo)
    ch = placesref.channels(width)
    for name, case in placesref.ablation_cases(width).items():
        ctx.set_ablation(case)
        want_logits, want_taps = want64(width, geo, False, case)
        ratio = ratio_of(ctx.classify(images), want_logits)
        print(f'PLACES width {width} {precision} ablate {name}: {ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS, (width, precision, name, ratio)
    wiped = ctx.classify(images)   # (conv5_all is the last case)
    assert torch.equal(wiped, wiped[:1].expand_as(wiped))
    # one more unit zeroes its channel and leaves the others as they were, bit for bit
    base = [('conv2', 3), ('conv4', 7)]
    ctx.set_ablation(base)
    before = ctx.activations(images, LAYERS)
    for index, layer in enumerate(LAYERS):
        unit = ch[index] - 2
        ctx.set_ablation([*base, (layer, unit)])
        after = ctx.activations(images, [layer])[layer]
        keep = [u for u in range(ch[index]) if u != unit]
        assert not bool(after[:, unit].any())
        assert bool(before[layer][:, unit].any())
        assert torch.equal(after[:, keep], before[layer][:, keep])
    # the sweep's rows are the single calls
    units = [(level, u) for level in range(5) for u in sorted({0, 5, ch[level] - 1})]
    targets = torch.arange(len(images)) % CLASSES
    ctx.set_ablation(base)
    swept, correct = ctx.classify_sweep(images, units, targets)
    rows = []
    for unit in units:
        ctx.set_ablation([*base, unit])
        rows.append(ctx.classify(images, return_logits=False))
    rows = torch.stack(rows)
    assert torch.equal(swept, rows)
    assert torch.equal(correct.cpu().long(), (rows.cpu() == targets).sum(dim=1))
    ctx.set_ablation([])


# ---- 6. geometry and surface ------------------------------------------------------------------
def test_geometry_and_errors(contexts):
    ctx = contexts(8)
    ctx.set_precision('f32')
    images = pictures((224, 224))
    with pytest.raises(ValueError, match='224x224'):
        ctx.classify(images)
    with pytest.raises(ValueError, match='224x224'):
        ctx.classify_sweep(images, [(0, 0)])
    taps = ctx.activations(images, LAYERS)
    want = placesref.forward(images.double(), model_sd(8))[1]
    for layer in LAYERS:
        assert ratio_of(taps[layer], want[layer]) <= FEATURE_CLASS
    # a pool the walk has to cross needs 3 x 3 pixels: 35 x 35 reaches every level, 19 x 19 conv2
    with pytest.raises(ValueError, match='too small'):
        ctx.activations(images[:, :, :34, :34], [4])
    with pytest.raises(ValueError, match='too small'):
        ctx.activations(images[:, :, :18, :35], [1])
    small = ctx.activations(images[:, :, :35, :38], LAYERS)
    want = placesref.forward(images[:, :, :35, :38].double(), model_sd(8))[1]
    for layer in LAYERS:
        assert small[layer].shape == want[layer].shape
        assert ratio_of(small[layer], want[layer]) <= FEATURE_CLASS
    assert ctx.activations(images[:, :, :34, :19], [1])[1].shape == (N_IMAGES, 64, 2, 1)
    assert ctx.activations(images[:, :, :11, :14], [0])[0].shape == (N_IMAGES, 24, 1, 1)
    with pytest.raises(ValueError, match='too small'):
        ctx.activations(images[:, :, :10, :14], [0])
    # a headless context taps and ablates, and says what classify lacks
    bare = make_context(model_sd(8), head=False)
    bare.set_precision('f32')
    bare.set_ablation([(2, 1)])
    ctx.set_ablation([(2, 1)])
    good = pictures((227, 227))
    assert torch.equal(bare.activations(good, [4])[4], ctx.activations(good, [4])[4])
    with pytest.raises(RuntimeError, match='milan_set_alexnet_head'):
        bare.classify(good)
    bare.close()
    ctx.set_ablation([])
    # no encoder config, no fast mode
    g = torch.Generator().manual_seed(9)
    exemplar_images = torch.randint(256, (2, 3, 96, 96), generator=g, dtype=torch.uint8)
    masks = torch.ones(2, 1, 96, 96, dtype=torch.uint8)
    with pytest.raises(ValueError, match='no encoder config'):
        ctx.encode(exemplar_images, masks)
    ctx.set_precision('f16')
    with pytest.raises(ValueError, match='fast f16'):
        ctx.classify(good)
    ctx.set_precision('f32')
    with pytest.raises(ValueError, match='local_size'):
        ctx.set_alexnet_lrn(4)
    # the LRN belongs to this trunk alone
    rsd = {PREFIX + k: v for k, v in synthetic.resnet_state_dict('resnet18', seed=1,
                                                                 width=8).items()}
    resnet = hip.Context(hip.make_dims(rsd, 1, blocks=(2, 2, 2, 2)), rsd, torch.device('cuda'))
    with pytest.raises(ValueError, match='Places365'):
        resnet.set_alexnet_lrn(5)
    # the codes themselves (both surface as ValueError): a wrong trunk kind and a bad size are
    # MILAN_ERR_ARG, an image that does not leave 6 x 6 is MILAN_ERR_SHAPE
    lib = hip.load_library()
    assert lib.milan_set_alexnet_lrn(resnet._h, 5, 1e-4, 0.75) == hip.ERR_ARG
    assert lib.milan_set_alexnet_lrn(ctx._h, 4, 1e-4, 0.75) == hip.ERR_ARG
    assert lib.milan_set_alexnet_lrn(ctx._h, 0, 1e-4, 0.75) == 0
    resnet.close()
    ws = ctx._classify_ws(N_IMAGES, 224, 224, 0)
    logits = torch.empty(N_IMAGES, CLASSES, device='cuda')
    dev = images.cuda()
    assert lib.milan_classify(ctx._h, dev.data_ptr(), N_IMAGES, 224, 224, logits.data_ptr(), None,
                              ws.data_ptr(), ws.numel(), None) == hip.ERR_SHAPE


@pytest.mark.parametrize('lrn', (False, True))
def test_classifier_module_runs_natively(lrn, want64):
    width = 16
    model = classifiers.PlacesAlexNetClassifier(CLASSES, width, HIDDEN, include_lrn=lrn,
                                                precision='auto')
    model.load_state_dict(model_sd(width), strict=True)
    model.eval().to('cuda')
    images = pictures((227, 227)).cuda()
    with torch.no_grad():
        assert model.runs_natively(images)
        got = model(images)
        tap = model.activations(images, 'conv4')['conv4']
    want_logits, want_taps = want64(width, (227, 227), lrn)
    assert ratio_of(got, want_logits) <= FEATURE_CLASS
    assert ratio_of(tap, want_taps['conv4']) <= FEATURE_CLASS


# ---- 7. dissection ----------------------------------------------------------------------------
def dissect(model, dataset, layer, tmp_path, source, image_size):
    """exemplars.discriminative against the oracle's `compute` fed `source(images)` = the
    layer's activations for the same batches (test_gpu_alexnet.py's check)."""
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    torch.manual_seed(31)
    topk, rq = exemplars.discriminative(model, dataset, layer=layer, image_size=image_size,
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
    out = tmp_path / str(layer)
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


def test_dissect_places_alexnet(tmp_path):
    model = classifiers.PlacesAlexNetClassifier(CLASSES, 8, HIDDEN, precision='f32')
    model.load_state_dict(model_sd(8), strict=True)
    model.eval()
    g = torch.Generator().manual_seed(2305)
    dataset = data.TensorDataset(torch.rand(23, 3, 99, 131, generator=g))

    def source(images):
        with torch.no_grad():
            assert model.runs_natively(images)
            return model.activations(images, 'conv4')['conv4']

    want = dissect(model, dataset, 'conv4', tmp_path, source, 99)
    assert want['ids'].shape == (placesref.channels(8)[3], 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


def old_resnet152(width, precision):
    """A slim OldResNet152 loaded from a state dict in the OLD key names."""
    meta = json.loads((placesref.GOLDEN / 'reference_goldens_places.json').read_text())
    tv = placesref.make_resnet152_state_dict(SEED, width, CLASSES)
    model = classifiers.OldResNet152(CLASSES, width, precision=precision)
    own = list(model.state_dict().keys())
    old_names = [k for k, _ in meta['resnet152']['state_dict']]
    assert len(own) == len(old_names)
    old_sd = {old: tv[new] for old, new in zip(old_names, own)
              if not new.endswith('num_batches_tracked')}
    model.load_state_dict(old_sd, strict=True)
    return model.eval(), tv


@pytest.mark.parametrize('precision', PRECISIONS)
def test_old_resnet152_native_logits(precision):
    model, tv = old_resnet152(8, precision)
    model.to('cuda')
    images = placesref.make_images(SEED, 3, (224, 224))
    blocks = synthetic.RESNET_BLOCKS['resnet152']
    want_logits, want_taps = actref.forward(images.double(), tv, blocks)
    with torch.no_grad():
        assert model.runs_natively(images.cuda())
        got = model(images.cuda())
        taps = model.activations(images.cuda(), ['0', 5, 'layer4'])
    ratio = ratio_of(got, want_logits)
    print(f'PLACES OldResNet152 width 8 {precision} logits: {ratio / FEATURE_CLASS:.3f} x bound')
    assert ratio <= FEATURE_CLASS
    for key, layer in (('0', 'conv1'), (5, 'layer2'), ('layer4', 'layer4')):
        assert ratio_of(taps[key], want_taps[layer]) <= FEATURE_CLASS, key
    # the fixed AvgPool2d(7) of the reference: the native forward says so
    with pytest.raises(ValueError, match='AvgPool2d'), torch.no_grad():
        model(images.cuda()[:, :, :192, :192])
    with pytest.raises(KeyError), torch.no_grad():
        model.activations(images.cuda(), '3')


def test_dissect_old_resnet152_by_the_reference_layer_name(tmp_path):
    model, _ = old_resnet152(8, 'f32')
    g = torch.Generator().manual_seed(2306)
    dataset = data.TensorDataset(torch.rand(23, 3, 96, 128, generator=g))

    def source(images):
        with torch.no_grad():
            assert model.runs_natively(images)
            return model.activations(images, 'layer2')['layer2']

    want = dissect(model, dataset, 5, tmp_path, source, 96)
    assert want['ids'].shape == (8 * 8, 3)
    assert (tmp_path / '5' / 'images.npy').exists()
