"""GPU tests of milan_amd.generators' native walk (milan_gan_run): every tap and the images
against tests/bigganref.py in float64 and against the reference's golden, the walk's
properties (taps alone, batch invariance, early stop, the choice between the two forwards,
the context) and a dissection end to end through exemplars.generative.

Bound: max|got - want| <= max(4 x e32, FEATURE_CLASS x max|want|), e32 = the error of
bigganref in float32 on the CPU against bigganref in float64 on that same case
(bigganref.check).  The tests print the measured multiple of the bound per tensor
(`BIGGAN ...` lines); DESIGN 4.26 quotes the worst.

Cases: the golden's 32 x 32 generator (hierarchical z, attention at 16 x 16 with 32
channels); a 64 x 64 generator with G_ch 48, whose attention block has the production width
(C = 192, dk = 24, dv = 96) at 32 x 32 pixels; a 32 x 32 generator without spectral norm,
hierarchy or attention.  The golden's 64 x 64 generator has 8 attention channels, which the
kernel does not take: it must run eagerly, and match.
"""
import functools
import io
import types

import numpy
import pytest
import torch
from torch.utils import data

import bigganref
from conftest import GOLDEN_DIR
from milan_amd import exemplars, generators, hip
from oracle import exemplars_oracle as E

pytestmark = pytest.mark.gpu

CASES = {
    'c32': (bigganref.make_dims(32, 8, 16, 32, 16, 10, hier=True, bn_eps=1e-4), 2),
    'wide64': (bigganref.make_dims(64, 48, 32, 40, 24, 12, hier=True, bn_eps=1e-4), 2),
    'plain32': (bigganref.make_dims(32, 12, 0, 18, 8, 5, hier=False, bn_eps=1e-5, sn=False), 2),
}


@functools.lru_cache(maxsize=None)
def golden():
    return numpy.load(GOLDEN_DIR / 'reference_goldens_biggan.npz')


def golden_state_dict(name, dtype):
    prefix = f'{name}/sd/'
    g = golden()
    return {key[len(prefix):]: torch.from_numpy(g[key].astype(numpy.float32)).to(dtype)
            for key in g.files if key.startswith(prefix)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dims, float64 weights, (z, hard y, soft y), float64 (taps, images) for hard and for
    soft y, the float32 ones): computed once per case and left unchanged."""
    dims, batch = CASES[name]
    if name == 'c32':  # the golden's weights and latents
        g = golden()
        sd = golden_state_dict(name, torch.float64)
        z, hard, soft = (torch.from_numpy(g[f'{name}/{k}']) for k in ('z', 'y_hard', 'y_soft'))
        z, soft = z.double(), soft.double()
    else:
        sd = bigganref.weights(dims, seed=300 + len(name))
        z, hard, soft = bigganref.latents(dims, batch, seed=400 + len(name))
    sd32 = bigganref.cast(sd, torch.float32)
    with torch.no_grad():
        want = [bigganref.forward(sd, z, y, dims) for y in (hard, soft)]
        ref32 = [bigganref.forward(sd32, z.float(), y, dims) for y in (hard, soft.float())]
    return dims, sd, (z, hard, soft), want, ref32


def model_of(name, **kwargs):
    dims, sd, *_ = reference(name)
    model = generators.from_state_dict(bigganref.cast(sd, torch.float32), BN_eps=dims['bn_eps'],
                                       **kwargs)
    return generators.SeqBigGAN(model.cuda())


def guarded(seq):
    """The eager paths raise: whatever returns came from the native walk."""
    def refuse(*args, **kwargs):
        raise AssertionError('the eager path ran')
    seq.forward_eager = refuse
    seq.generator.forward_eager = refuse
    for child in seq.children():
        child.forward = refuse
    return seq


def inputs_of(name, soft=False, rows=slice(None)):
    z, hard, soft_y = reference(name)[2]
    y = soft_y.float() if soft else hard
    return generators.GInputs(z.float()[rows].cuda(), y[rows].cuda())


@pytest.mark.parametrize('name', list(CASES))
def test_taps_and_images_against_float64(name):
    dims, _, _, want, ref32 = reference(name)
    seq = guarded(model_of(name))
    for kind, soft in (('hard', False), ('soft', True)):
        inputs = inputs_of(name, soft)
        (taps64, images64), (taps32, images32) = want[soft], ref32[soft]
        with torch.no_grad():
            assert seq.runs_natively(inputs), seq.native_refusal(inputs)
            for layer in seq.layers:
                bag, images = seq.generate(inputs, layer=layer, images=True)
                bigganref.check(f'{name} {kind} y {layer}', bag.h, taps64[layer], taps32[layer])
                bigganref.check(f'{name} {kind} y images with {layer}', images, images64, images32)
                if not soft:
                    break  # (every layer once is enough; the taps-alone test covers the rest)
            bigganref.check(f'{name} {kind} y forward', seq(inputs), images64, images32)
            y = inputs.y @ seq.generator.shared.weight if soft else seq.generator.shared(inputs.y)
            bigganref.check(f'{name} {kind} y Generator.forward', seq.generator(inputs.z, y),
                            images64, images32)
            bigganref.check(f'{name} {kind} y Generator.forward(embed)',
                            seq.generator(inputs.z, inputs.y, embed=True), images64, images32)


def test_every_tap_against_float64_at_the_production_attention_width():
    name = 'wide64'
    _, _, _, want, ref32 = reference(name)
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    assert seq.layers == ('layer0', 'layer1', 'layer2', 'attn2', 'layer3')
    assert seq.generator.attention_channels == 192
    with torch.no_grad():
        for layer in seq.layers:
            bag, _ = seq.generate(inputs, layer=layer, images=False)
            bigganref.check(f'{name} {layer}', bag.h, want[0][0][layer], ref32[0][0][layer])


def test_the_golden_of_the_reference():
    """|got - golden| <= the bound + the golden's own distance from float64 (it is a float32
    run of the reference's modules)."""
    name = 'c32'
    g = golden()
    _, _, _, want, ref32 = reference(name)
    seq = guarded(model_of(name))
    with torch.no_grad():
        for layer in seq.layers:
            bag, images = seq.generate(inputs_of(name), layer=layer)
            gold = torch.from_numpy(g[f'{name}/hard/{layer}']).double()
            limit, _ = bigganref.bound(want[0][0][layer], ref32[0][0][layer])
            slack = float((gold - want[0][0][layer][:1]).abs().max())
            err = float((bag.h[:1].cpu().double() - gold).abs().max())
            print(f'BIGGAN golden {layer}: max|err| {err:.3g}, bound {limit:.3g} + {slack:.3g}')
            assert err <= limit + slack, layer
        for kind, soft in (('hard', False), ('soft', True)):
            gold = torch.from_numpy(g[f'{name}/{kind}/images']).double()
            limit, _ = bigganref.bound(want[soft][1], ref32[soft][1])
            slack = float((gold - want[soft][1]).abs().max())
            err = float((seq(inputs_of(name, soft)).cpu().double() - gold).abs().max())
            print(f'BIGGAN golden {kind} images: max|err| {err:.3g}, bound {limit:.3g} + {slack:.3g}')
            assert err <= limit + slack, kind


def test_the_narrow_golden_generator_runs_eagerly_and_matches():
    g = golden()
    dims = bigganref.make_dims(64, 2, 32, 20, 12, 7, hier=False, bn_eps=1e-5)
    model = generators.from_state_dict(golden_state_dict('c64', torch.float32), BN_eps=1e-5)
    seq = generators.SeqBigGAN(model.cuda())
    z, hard = (torch.from_numpy(g[f'c64/{k}']).cuda() for k in ('z', 'y_hard'))
    with torch.no_grad():
        assert '8 channels' in seq.native_refusal(generators.GInputs(z, hard))
        images = seq(generators.GInputs(z, hard))
    sd = golden_state_dict('c64', torch.float64)
    want = bigganref.forward(sd, z.cpu().double(), hard.cpu(), dims)[1]
    ref32 = torch.from_numpy(g['c64/hard/images'])
    bigganref.check('c64 eager images on the GPU', images, want, ref32)
    with pytest.raises(ValueError, match='ch 2 must be a multiple of 4'):
        hip.GanContext(model.dims(), model.folded_state_dict(), torch.device('cuda'))


def test_every_tap_alone_equals_the_all_taps_call():
    seq = guarded(model_of('c32'))
    inputs = inputs_of('c32')
    gen = seq.generator
    with torch.no_grad():
        every, images = gen._native(inputs.z, inputs.y, embedded=False,
                                    taps=range(len(seq.layers)), want_images=True)
        for index, layer in enumerate(seq.layers):
            bag, none = seq.generate(inputs, layer=layer, images=False)
            assert none is None and torch.equal(bag.h, every[index]), layer
            bag, pictures = seq.generate(inputs, layer=layer, images=True)
            assert torch.equal(bag.h, every[index]) and torch.equal(pictures, images), layer
            assert len(bag.ys) == 3 and bag.ys[0].shape == (2, 16 + 8)
        assert torch.equal(seq(inputs), images)


def test_a_sample_does_not_depend_on_its_batch_or_on_max_images():
    for name in ('c32', 'plain32'):
        seq = guarded(model_of(name))
        inputs = inputs_of(name)
        n, last = inputs.z.shape[0], seq.layers[-1]
        with torch.no_grad():
            bag, images = seq.generate(inputs, layer=last)
            for i in range(n):
                one = generators.GInputs(inputs.z[i:i + 1], inputs.y[i:i + 1])
                alone, picture = seq.generate(one, layer=last)
                assert torch.equal(alone.h, bag.h[i:i + 1]), (name, i)
                assert torch.equal(picture, images[i:i + 1]), (name, i)
            seq.generator.max_images = 1  # one pass per sample
            split, pictures = seq.generate(inputs, layer=last)
            assert torch.equal(split.h, bag.h) and torch.equal(pictures, images)
            assert torch.equal(seq(inputs), images)


def test_the_walk_stops_after_the_deepest_tap():
    """With every later block, the attention and the output layer set to NaN, layer0 is
    unchanged and finite: nothing after it ran."""
    seq = guarded(model_of('c32'))
    inputs = inputs_of('c32')
    with torch.no_grad():
        before = seq.generate(inputs, layer='layer0', images=False)[0].h.clone()
        for key, value in seq.generator.state_dict().items():
            if key.startswith(('blocks.1.', 'blocks.2.', 'output_layer.')) and '.u0' not in key:
                value.fill_(float('nan'))
        after = seq.generate(inputs, layer='layer0', images=False)[0].h
        assert torch.isnan(seq(inputs)).all()  # the new weights are in the context
    assert torch.equal(after, before) and bool(torch.isfinite(after).all())


def test_a_forward_hook_or_training_mode_selects_the_eager_path():
    seq = model_of('c32')
    inputs = inputs_of('c32')
    ran = []
    original = seq.generator.blocks[0][0].forward

    def spy(x, y):
        ran.append(1)
        return original(x, y)

    seq.generator.blocks[0][0].forward = spy
    with torch.no_grad():
        native = seq(inputs)
        assert not ran
        fired = []
        handle = seq.layer1.register_forward_hook(lambda m, i, o: fired.append(o.h.shape))
        assert 'hook' in seq.native_refusal(inputs)
        hooked = seq(inputs)
        assert ran and fired == [(2, 32, 16, 16)]
        handle.remove()
        assert seq.runs_natively(inputs)
        seq.train()
        assert 'training' in seq.native_refusal(inputs)
        seq.eval()
    assert 'grad' in seq.native_refusal(inputs)
    _, _, _, want, ref32 = reference('c32')
    bigganref.check('c32 hooked (eager) images', hooked, want[0][1], ref32[0][1])
    bigganref.check('c32 native images', native, want[0][1], ref32[0][1])


def test_errors_and_a_second_finalize():
    seq = guarded(model_of('c32'))
    inputs = inputs_of('c32')
    with torch.no_grad():
        seq(inputs)
        ctx = seq.generator._context()
        with pytest.raises(RuntimeError, match='already finalized'):
            hip._check(ctx._fn('finalize_weights')(ctx._h, 0))
        with pytest.raises(IndexError, match='class index'):
            seq(generators.GInputs(inputs.z, torch.full_like(inputs.y, 10)))
        with pytest.raises(ValueError, match=r'z must be \(n, 32\)'):
            ctx.run(inputs.z[:, :31], inputs.y, taps=(0,))
        with pytest.raises(ValueError, match='neither a tap nor the images'):
            ctx.run(inputs.z, inputs.y)
        with pytest.raises(KeyError, match='layer7'):
            seq.generate(inputs, layer='layer7')
        # the context still works
        _, _, _, want, ref32 = reference('c32')
        bigganref.check('c32 images after the errors', seq(inputs), want[0][1], ref32[0][1])
    missing = seq.generator.folded_state_dict()
    del missing['blocks.1.1.gamma']
    with pytest.raises(RuntimeError, match='blocks.1.1.gamma was not uploaded'):
        hip.GanContext(seq.generator.dims(), missing, torch.device('cuda'))


# ---- dissect end to end ----------------------------------------------------------------------
def test_dissect_a_generator_natively(tmp_path):
    """exemplars.generative against the oracle's `compute` fed the model's own hiddens and
    images for the same batches: only the plumbing is under test, bit for bit."""
    seq = guarded(model_of('c32'))
    dims = CASES['c32'][0]
    z, hard, _ = bigganref.latents(dims, 23, seed=2306)
    dataset = data.TensorDataset(z.float(), hard)
    layer = 'layer1'
    renormalizer = types.SimpleNamespace(mean=[.5, .5, .5], std=[.5, .5, .5])  # [-1, 1] -> bytes
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    asked = []
    generate = seq.generate

    def spy(inputs, layer=None, images=True):
        asked.append(images)
        return generate(inputs, layer=layer, images=images)

    seq.generate = spy
    torch.manual_seed(31)
    topk, rq = exemplars.generative(seq, dataset, layer,
                                    transform_inputs=lambda *xs: (generators.GInputs(*xs),),
                                    transform_hiddens=lambda hiddens: hiddens.h,
                                    renormalizer=renormalizer, image_size=32, num_workers=0,
                                    save_viz=False, results_dir=tmp_path, **kwargs)
    assert asked[:5] == [False] * 5 and all(asked[5:]) and len(asked) > 5

    def both(zs, ys):
        with torch.no_grad():
            bag, images = generate(generators.GInputs(zs.cuda(), ys.cuda()), layer=layer)
        return bag.h.cpu(), images.cpu()

    def topk_and_quantile(zs, ys):
        h = both(zs, ys)[0]
        b, c = h.shape[:2]
        return h.view(b, c, -1).max(dim=2)[0], h.permute(0, 2, 3, 1).reshape(-1, c)

    mul, add = exemplars.byte_renormalization(renormalizer)
    torch.manual_seed(31)
    want = E.compute(topk_and_quantile, both, dataset, mul=tuple(mul), add=tuple(add),
                     stable_ties=True, **kwargs)
    out = tmp_path / layer
    assert torch.equal(torch.from_numpy(numpy.load(out / 'images.npy')), want['images'])
    assert torch.equal(torch.from_numpy(numpy.load(out / 'masks.npy')), want['masks'])
    assert int(want['masks'].sum()) > 0 and int(want['images'].max()) > 0
    values, ids = topk.result()
    assert torch.equal(ids.cpu(), want['ids']) and want['ids'].shape == (32, 3)
    assert torch.equal(values.cpu(), want['activations'])
    text = io.StringIO()
    numpy.savetxt(text, want['activations'].numpy(), delimiter=',', fmt='%.5e')
    assert (out / 'activations.csv').read_text() == text.getvalue()
    assert torch.equal(rq.quantiles(.9).cpu().reshape(-1), want['levels'].reshape(-1))
    assert sum(len(m._forward_hooks) for m in seq.modules()) == 0
