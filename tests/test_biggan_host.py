"""CPU tests of the BigGAN generator: tests/bigganref.py (the float64 restatement) and
milan_amd.generators' eager modules against the golden that the reference's own modules
produced (tests/golden/make_golden_biggan.py), and the plumbing around them.
"""
import collections

import numpy
import pytest
import torch
from torch import nn

import bigganref
from conftest import GOLDEN_DIR
from milan_amd import exemplars, generators, hip

CONFIGS = collections.OrderedDict(
    c32=bigganref.make_dims(32, 8, 16, 32, 16, 10, hier=True, bn_eps=1e-4),
    c64=bigganref.make_dims(64, 2, 32, 20, 12, 7, hier=False, bn_eps=1e-5),
)


@pytest.fixture(scope='module')
def golden():
    return numpy.load(GOLDEN_DIR / 'reference_goldens_biggan.npz')


def state_dict(golden, name, dtype=torch.float32):
    prefix = f'{name}/sd/'
    return collections.OrderedDict(
        (key[len(prefix):], torch.from_numpy(golden[key].astype(numpy.float32)).to(dtype))
        for key in golden.files if key.startswith(prefix))


def latents(golden, name):
    return (torch.from_numpy(golden[f'{name}/z']), torch.from_numpy(golden[f'{name}/y_hard']),
            torch.from_numpy(golden[f'{name}/y_soft']))


def model(golden, name):
    d = CONFIGS[name]
    g = generators.Generator(G_ch=d['ch'], dim_z=d['dim_z'], resolution=d['resolution'],
                             G_attn=str(d['attn']), n_classes=d['n_classes'],
                             shared_dim=d['shared_dim'], hier=d['hier'], BN_eps=d['bn_eps'])
    g.load_state_dict(state_dict(golden, name), strict=True)
    return g.eval()


def close32(what, got, want, ulps=64):
    """float32 rounding: the golden is a float32 run, so two correct float32 (or one float64)
    computations of it differ by accumulated roundings of the tensor's scale."""
    want = torch.as_tensor(want).double()
    got = got.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max())
    limit = ulps * 2.**-24 * float(want.abs().max())
    print(f'BIGGAN host {what}: max|err| {err:.3g}, limit {limit:.3g}')
    assert err <= limit, f'{what}: max|err| {err:g} > {limit:g}'


@pytest.mark.parametrize('name', list(CONFIGS))
def test_the_restatement_in_float64_is_the_reference(golden, name):
    d = CONFIGS[name]
    sd = state_dict(golden, name, torch.float64)
    z, hard, soft = latents(golden, name)
    taps, images = bigganref.forward(sd, z.double(), hard, d)
    assert list(taps) == bigganref.layer_names(d)
    for key, value in taps.items():
        close32(f'{name} {key}', value[:1], golden[f'{name}/hard/{key}'])
    close32(f'{name} images (hard y)', images, golden[f'{name}/hard/images'])
    _, images = bigganref.forward(sd, z.double(), soft.double(), d)
    close32(f'{name} images (soft y)', images, golden[f'{name}/soft/images'])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_generator_loads_strictly_and_its_eager_path_matches(golden, name):
    g = model(golden, name)
    z, hard, soft = latents(golden, name)
    with torch.no_grad():
        close32(f'{name} forward_eager', g.forward_eager(z, hard, embed=True),
                golden[f'{name}/hard/images'])
        # forward() on the CPU is the eager path; y given embedded, as pretorched's default
        close32(f'{name} forward', g(z, soft @ g.shared.weight), golden[f'{name}/soft/images'])
        seq = generators.SeqBigGAN(g)
        inputs = generators.GInputs(z, hard)
        assert not seq.runs_natively(inputs)
        close32(f'{name} sequential', seq(inputs), golden[f'{name}/hard/images'])
        for layer in seq.layers:
            bag, images = seq.generate(inputs, layer=layer, images=False)
            assert images is None and len(bag.ys) == len(g.blocks)
            close32(f'{name} generate {layer}', bag.h[:1], golden[f'{name}/hard/{layer}'])
        bag, images = seq.generate(inputs, layer=seq.layers[0])
        close32(f'{name} generate images', images, golden[f'{name}/hard/images'])
        assert torch.equal(bag.h, seq.generate(inputs, seq.layers[0], images=False)[0].h)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_children_names_and_order(golden, name):
    g = model(golden, name)
    seq = generators.SeqBigGAN(g)
    assert [k for k, _ in seq.named_children()] == list(golden[f'{name}/children'])
    assert list(seq.layers) == bigganref.layer_names(CONFIGS[name])
    assert list(seq.layers) == [k for k in golden[f'{name}/children']
                                if k not in ('preprocess', 'output')]


def test_a_config_mapping_builds_the_same_module(golden):
    d = CONFIGS['c32']
    seq = generators.SeqBigGAN(dict(G_ch=d['ch'], dim_z=d['dim_z'], resolution=32, G_attn='16',
                                    n_classes=10, shared_dim=16, hier=True, BN_eps=1e-4))
    seq.generator.load_state_dict(state_dict(golden, 'c32'), strict=True)
    assert set(seq.generator.state_dict()) == set(state_dict(golden, 'c32'))
    assert generators.infer_config(state_dict(golden, 'c32')) == dict(
        G_ch=8, dim_z=32, bottom_width=4, resolution=32, G_attn='16', n_classes=10,
        shared_dim=16, hier=True, G_param='SN')
    assert generators.infer_config(state_dict(golden, 'c64'))['resolution'] == 64


@pytest.mark.parametrize('name', list(CONFIGS))
def test_spectral_norm_folding_is_the_references_eval_weight(golden, name):
    g = model(golden, name)
    folded = g.folded_state_dict()
    assert not any(k.endswith(('.u0', '.sv0')) for k in folded)
    sd64 = state_dict(golden, name, torch.float64)
    for key in golden.files:
        if not key.startswith(f'{name}/sn/'):
            continue
        layer = key[len(f'{name}/sn/'):]
        want = golden[key]
        close32(f'{name} folded {layer}', folded[layer + '.weight'], want, ulps=8)
        close32(f'{name} module {layer}', g.get_submodule(layer).normalised_weight(), want,
                ulps=8)
        close32(f'{name} bigganref {layer}',
                bigganref.sn_weight(sd64[layer + '.weight'], sd64[layer + '.u0']), want, ulps=8)
    # unnormalised tensors pass through
    assert torch.equal(folded['shared.weight'], g.shared.weight)
    assert torch.equal(folded['linear.bias'], g.linear.bias)


def test_a_plain_conv_generator_has_no_sn_buffers():
    d = bigganref.make_dims(32, 4, 0, 16, 8, 5, hier=False, sn=False)
    sd = bigganref.weights(d, 3)
    assert not any(k.endswith('.u0') for k in sd)
    assert not generators.from_state_dict(bigganref.cast(sd, torch.float32)).training
    g = generators.Generator(**generators.infer_config(sd), BN_eps=1e-4).double()
    g.load_state_dict(sd, strict=True)
    g.eval()
    assert not g.sn and g.attn_resolution == 0 and g.layers == ('layer0', 'layer1', 'layer2')
    folded = g.folded_state_dict()
    assert all(torch.equal(folded[k], v) for k, v in sd.items())
    z, hard, _ = bigganref.latents(d, 2, 4)
    want = bigganref.forward(sd, z, hard, d)[1]
    with torch.no_grad():  # both in float64: only the order of the sums differs
        got = g(z, hard, embed=True)
    assert float((got - want).abs().max()) < 1e-9


# ---- the architectures and bottom widths that no golden covers -------------------------------
def eager_of(name):
    """The eager Generator of a bigganref.SHAPE_CASES entry in float32, loaded strictly."""
    dims, sd, _ = bigganref.shape_case(name)
    g = generators.from_state_dict(bigganref.cast(sd, torch.float32), BN_eps=dims['bn_eps'],
                                   bottom_width=dims['bottom_width'])
    assert (g.ch, g.bottom_width, g.resolution) == (dims['ch'], dims['bottom_width'],
                                                    dims['resolution'])
    return g


@pytest.mark.parametrize('name', ['r128', 'r256flat', 'r512', 'bw3'])
def test_the_eager_generator_matches_float64_off_the_golden(name):
    """The Python ARCH rows for 128, 256 and 512 and a bottom width other than 4: the eager
    modules against bigganref in float64, inside the bound of the native walk."""
    dims, batch = bigganref.SHAPE_CASES[name]
    _, _, (z, hard, _) = bigganref.shape_case(name)
    (taps64, images64), (taps32, images32) = bigganref.shape_reference(name)
    g = eager_of(name)
    side = bigganref.image_side(dims)
    with torch.no_grad():
        images = g.forward_eager(z.float(), hard, embed=True)
        assert images.shape == (batch, 3, side, side) and g.image_side == side
        bigganref.check(f'host {name} forward_eager', images, images64, images32)
        seq = generators.SeqBigGAN(g)
        assert list(seq.layers) == bigganref.layer_names(dims)
        inputs = generators.GInputs(z.float(), hard)
        for layer in seq.layers:  # the hook-free eager path of generate, tap by tap
            bag, _ = seq.generate(inputs, layer=layer, images=False)
            bigganref.check(f'host {name} eager {layer}', bag.h, taps64[layer], taps32[layer])


@pytest.mark.parametrize('bottom_width', [1, 3, 4, 5])
@pytest.mark.parametrize('resolution', [32, 64, 128, 256, 512])
def test_layer_names_tap_shapes_and_image_side(resolution, bottom_width):
    """Shape arithmetic of the module, of the binding (what GanContext allocates) and of
    bigganref agree: block i ends at side bottom_width << (i + 1), the images at
    bottom_width << blocks, whatever `resolution` says."""
    blocks = len(bigganref.ARCH[resolution][0])
    for attn in [0] + [8 << i for i in range(blocks)]:
        dims = bigganref.make_dims(resolution, 8, attn, 16, 8, 3, bottom_width=bottom_width)
        g = generators.Generator(G_ch=8, dim_z=16, bottom_width=bottom_width,
                                 resolution=resolution, G_attn=str(attn), n_classes=3,
                                 shared_dim=8, hier=True, skip_init=True)
        names, shapes = bigganref.layer_names(dims), bigganref.tap_shapes(dims)
        assert list(g.layers) == names and len(shapes) == len(names) == blocks + bool(attn)
        assert hip.gan_tap_shapes(g.dims()) == shapes
        side = bigganref.image_side(dims)
        assert hip.gan_image_side(g.dims()) == g.image_side == side == bottom_width << blocks
        assert shapes[-1][1] == side and (side == resolution) == (bottom_width == 4)
        if attn:  # 8 << k: after block k, with that block's shape
            k = attn.bit_length() - 4
            assert names[k + 1] == f'attn{k}' and shapes[k + 1] == shapes[k]


def test_infer_config_reads_the_bottom_width():
    for name in ('bw3', 'bw1', 'r128'):
        dims, sd, _ = bigganref.shape_case(name)
        config = generators.infer_config(sd)
        assert (config['G_ch'], config['bottom_width']) == (dims['ch'], dims['bottom_width'])
        assert config['resolution'] == dims['resolution'] and config['dim_z'] == dims['dim_z']
    broken = dict(bigganref.shape_case('bw3')[1])
    broken['linear.weight'] = broken['linear.weight'][:-1]
    with pytest.raises(ValueError, match='no G_ch and bottom_width'):
        generators.infer_config(broken)


def _first_tap_outside(name, sd32, z32, hard):
    """The first tap of the float32 reference on changed inputs that leaves bound(), or None."""
    dims = bigganref.SHAPE_CASES[name][0]
    (taps64, _), (taps32, _) = bigganref.shape_reference(name)
    with torch.no_grad():
        taps, _ = bigganref.forward(sd32, z32, hard, dims)
    for layer, got in taps.items():
        limit, _ = bigganref.bound(taps64[layer], taps32[layer])
        err = float((got.double() - taps64[layer]).abs().max())
        print(f'BIGGAN host mutation {layer}: max|err| {err:.3g}, bound {limit:.3g}')
        if err > limit:
            return layer
    return None


def test_the_bound_is_not_slack_on_r128():
    """Three plausible mistakes of a walk, applied to the float32 reference itself, each leave
    the bound on some tap, at the block where they first act; the reference unchanged does
    not."""
    name = 'r128'
    dims, sd, (z, hard, _) = bigganref.shape_case(name)
    sd32, z32 = bigganref.cast(sd, torch.float32), z.float()
    assert _first_tap_outside(name, sd32, z32, hard) is None
    # block i conditioned on z chunk i instead of i + 1: the chunks shifted by one
    chunks = list(torch.split(z32, dims['chunk'], 1))
    shifted = torch.cat([chunks[0]] + chunks[:-1], 1)
    assert _first_tap_outside(name, sd32, shifted, hard) == 'layer0'
    # the shortcut conv without its bias, in the last block only
    no_bias = dict(sd32)
    no_bias['blocks.4.0.conv_sc.bias'] = torch.zeros_like(sd32['blocks.4.0.conv_sc.bias'])
    assert _first_tap_outside(name, no_bias, z32, hard) == 'layer4'
    # gamma not applied: o + x instead of gamma * o + x
    no_gamma = dict(sd32)
    no_gamma['blocks.3.1.gamma'] = torch.ones_like(sd32['blocks.3.1.gamma'])
    assert _first_tap_outside(name, no_gamma, z32, hard) == 'attn3'


def test_unsupported_widths_decline_the_native_path_with_a_message(golden):
    z, hard, _ = latents(golden, 'c64')
    g = model(golden, 'c64')  # 8 attention channels
    with torch.no_grad():
        # (on the CPU the device is the first objection; the width is checked regardless)
        assert 'not on the GPU' in g.native_refusal(z, hard)
        meta = g.native_refusal()
    assert '8 channels' in meta and 'multiple of 32' in meta
    wide = generators.Generator(G_ch=100, resolution=32, G_attn='16', n_classes=3, dim_z=8)
    with torch.no_grad():
        assert '400 channels' in wide.eval().native_refusal()
    odd = generators.Generator(G_ch=10, resolution=32, G_attn='16', n_classes=3, dim_z=8)
    with torch.no_grad():
        assert '40 channels' in odd.eval().native_refusal()
    fine = model(golden, 'c32')
    with torch.no_grad():
        assert fine.native_refusal() is None
        assert 'forward hook' not in str(fine.native_refusal())
    assert 'grad is enabled' in fine.native_refusal()
    assert 'training mode' in fine.train().native_refusal()
    with pytest.raises(ValueError, match='resolution 48'):
        generators.Generator(resolution=48)
    with pytest.raises(NotImplementedError, match='one attention block'):
        generators.Generator(resolution=128, G_attn='32_64')


def test_a_hook_declines_the_native_path(golden):
    g = model(golden, 'c32')
    seq = generators.SeqBigGAN(g)
    handle = seq.layer1.register_forward_hook(lambda *a: None)
    with torch.no_grad():
        assert 'forward hook' in g.native_refusal(roots=(seq,))
        handle.remove()
        assert g.native_refusal(roots=(seq,)) is None


class _Recorder:
    """Stands in for exemplars.compute: calls both functions once on one batch."""

    def __init__(self):
        self.calls = []

    def __call__(self, hiddens_only, both, dataset, **kwargs):
        batch = dataset
        self.calls.append(('hiddens', hiddens_only(*batch)))
        self.calls.append(('both', both(*batch)))
        return self.calls


def run_generative(monkeypatch, model_, batch, layer, **kwargs):
    recorder = _Recorder()
    monkeypatch.setattr(exemplars, 'compute', recorder)
    monkeypatch.setattr(exemplars.hip, 'require_device', lambda device: torch.device('cpu'))
    monkeypatch.setattr(exemplars, 'map_location', lambda items, device: tuple(items))
    exemplars.generative(model_, batch, layer, device='cpu', **kwargs)
    return recorder.calls


def test_generative_asks_a_model_that_generates(golden, monkeypatch):
    g = model(golden, 'c32')
    seq = generators.SeqBigGAN(g)
    asked = []
    original = seq.generate

    def spy(inputs, layer=None, images=True):
        asked.append((layer, images))
        return original(inputs, layer=layer, images=images)

    seq.generate = spy
    z, hard, _ = latents(golden, 'c32')
    calls = run_generative(monkeypatch, seq, (z, hard), 'layer1',
                           transform_inputs=lambda *xs: (generators.GInputs(*xs),),
                           transform_hiddens=lambda hiddens: hiddens.h)
    assert asked == [('layer1', False), ('layer1', True)]
    assert not any(m._forward_hooks for m in seq.modules())
    close32('generative hiddens', calls[0][1][:1], golden['c32/hard/layer1'])
    hiddens, images = calls[1][1]
    assert torch.equal(hiddens, calls[0][1])
    close32('generative images', images, golden['c32/hard/images'])
    with pytest.raises(KeyError, match='layer9'):
        run_generative(monkeypatch, seq, (z, hard), 'layer9',
                       transform_inputs=lambda *xs: (generators.GInputs(*xs),))


def test_generative_with_a_hooked_plain_module_still_takes_the_hook_path(monkeypatch):
    torch.manual_seed(0)
    plain = nn.Sequential(collections.OrderedDict(
        first=nn.Linear(4, 6), act=nn.Tanh(), last=nn.Linear(6, 3))).eval()
    fired = []
    plain.first.register_forward_hook(lambda *a: fired.append(1))
    x = torch.randn(5, 4)
    calls = run_generative(monkeypatch, plain, (x,), 'first')
    assert len(fired) == 2  # the model ran twice, whole, with the hook in place
    with torch.no_grad():
        assert torch.equal(calls[0][1], plain.first(x))
        assert torch.equal(calls[1][1][0], plain.first(x))
        assert torch.equal(calls[1][1][1], plain(x))
