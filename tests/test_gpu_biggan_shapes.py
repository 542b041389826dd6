"""GPU tests of the native BigGAN walk (milan_gan_run) off the shapes of test_gpu_biggan.py:
every block table (128, 256 and 512 have no golden), bottom widths other than 4, batches that
are odd or end in a remainder, and the GEMM and row-kernel paths those never took.

Oracle and bound are test_gpu_biggan.py's: tests/bigganref.py in float64, max|got - want| <=
max(4 x e32, FEATURE_CLASS x max|want|) with e32 the error of bigganref in float32 on the CPU on
that same case (bigganref.check, unchanged).  Spectral norm stays on in every case: without it
the taps reach 3e4 and the relative half of the bound goes slack.  Every model is `guarded`:
an eager fallback fails the test.  The `BIGGAN ...` lines print the measured multiple of the
bound; DESIGN 4.26 quotes the worst.

Cases (bigganref.SHAPE_CASES; make_dims(resolution, ch, attn, dim_z, shared_dim, n_classes)):
  r128      the 128 table; attention at its released slot (64 x 64), C = 32; final N = 16; n = 3
  r256      the 256 table; attention at 128 x 128: 16384 queries, 4096 keys; layer0 .. layer5
  r256flat  not hierarchical, with attention; N = 8 and 4 in ordinary convs; Cin 4 / 8 / 16
  r512      the 512 table, 7 blocks; chunk 3, shared_dim 5 (neither a multiple of 4)
  bw3       bottom_width 3: P = 36 / 144 / 576 pixels (partial nchw tiles), M = 5 x 36, 24 x 24
            images
  bw5       bottom_width 5: attention after block 0 at 10 x 10 (25 keys); 40 x 40 images, which
            overran a (n, 3, 32, 32) tensor before GanContext.run took its side from the walk
  bw1       bottom_width 1: M = 7 in the first shortcut conv; chunk 2; one class; 16 x 16 images
  n80       N = 80 > 64 with Cin = 80, not a multiple of 32: the wide tile's per-lane taps
The refusal test's own generator (ch 4, bottom_width 1) adds z chunks of one column.
"""
import pytest
import torch

import bigganref
from milan_amd import generators, hip
from test_gpu_biggan import guarded

pytestmark = pytest.mark.gpu

CASES = bigganref.SHAPE_CASES


def model_of(name, **kwargs):
    dims, sd, _ = bigganref.shape_case(name)
    # (bottom_width given, not inferred: a released checkpoint's is 4 and these are not)
    model = generators.from_state_dict(bigganref.cast(sd, torch.float32), BN_eps=dims['bn_eps'],
                                       bottom_width=dims['bottom_width'], **kwargs)
    assert model.bottom_width == dims['bottom_width'] and model.ch == dims['ch']
    return generators.SeqBigGAN(model.cuda())


def inputs_of(name, soft=False, rows=slice(None)):
    z, hard, soft_y = bigganref.shape_case(name)[2]
    y = soft_y.float() if soft else hard
    return generators.GInputs(z.float()[rows].cuda(), y[rows].cuda())


def everything(seq, inputs):
    """({tap index: tensor} of every tap, the images) of one native call."""
    return seq.generator._native(inputs.z, inputs.y, embedded=False,
                                 taps=range(len(seq.layers)), want_images=True)


@pytest.mark.parametrize('name', list(CASES))
def test_every_tap_and_the_images_against_float64(name):
    dims, batch = CASES[name]
    (taps64, images64), (taps32, images32) = bigganref.shape_reference(name)
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    side = bigganref.image_side(dims)
    assert list(seq.layers) == bigganref.layer_names(dims) == list(taps64)
    with torch.no_grad():
        assert seq.runs_natively(inputs), seq.native_refusal(inputs)
        taps, images = everything(seq, inputs)
    ctx = seq.generator._context()
    assert ctx.tap_shapes == bigganref.tap_shapes(dims)
    assert ctx.image_side == seq.generator.image_side == side
    assert images.shape == (batch, 3, side, side)
    for index, layer in enumerate(seq.layers):
        assert taps[index].shape == (batch, *[(c, s, s) for c, s in ctx.tap_shapes][index])
        bigganref.check(f'{name} {layer}', taps[index], taps64[layer], taps32[layer])
    bigganref.check(f'{name} images', images, images64, images32)


@pytest.mark.parametrize('name', ['bw3', 'bw5'])
def test_images_by_the_three_routes(name):
    """SeqBigGAN, Generator.forward with y embedded outside and with embed=True, hard and soft
    labels: (n, 3, R, R) with R = bottom_width << blocks, all against float64."""
    dims, batch = CASES[name]
    side = bigganref.image_side(dims)
    assert side == {'bw3': 24, 'bw5': 40}[name]
    seq = guarded(model_of(name))
    gen = seq.generator
    for kind, soft in (('hard', False), ('soft', True)):
        (_, images64), (_, images32) = bigganref.shape_reference(name, soft)
        inputs = inputs_of(name, soft)
        with torch.no_grad():
            y = inputs.y @ gen.shared.weight if soft else gen.shared(inputs.y)
            routes = (('SeqBigGAN', seq(inputs)), ('Generator.forward', gen(inputs.z, y)),
                      ('Generator.forward(embed)', gen(inputs.z, inputs.y, embed=True)),
                      ('generate', seq.generate(inputs, layer='layer0')[1]))
        for route, images in routes:
            assert images.shape == (batch, 3, side, side), (route, images.shape)
            bigganref.check(f'{name} {kind} y {route}', images, images64, images32)


@pytest.mark.parametrize('name', ['r128', 'bw3', 'bw1'])
def test_a_sample_does_not_depend_on_its_batch_or_on_a_remainder_chunk(name):
    """Bitwise, every tap and the images: a sample alone equals its slice of the batch, and
    max_images = 2 over n = 3, 5 or 7 (whole chunks and a remainder of one) equals one call."""
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    n = inputs.z.shape[0]
    assert n % 2 == 1 and seq.generator.max_images >= n
    with torch.no_grad():
        taps, images = everything(seq, inputs)
        for i in range(n):
            alone, picture = everything(seq, inputs_of(name, rows=slice(i, i + 1)))
            for index, layer in enumerate(seq.layers):
                assert torch.equal(alone[index], taps[index][i:i + 1]), (name, i, layer)
            assert torch.equal(picture, images[i:i + 1]), (name, i)
        seq.generator.max_images = 2
        split, pictures = everything(seq, inputs)
        for index, layer in enumerate(seq.layers):
            assert torch.equal(split[index], taps[index]), (name, layer)
        assert torch.equal(pictures, images) and torch.equal(seq(inputs), images)


def test_every_tap_alone_equals_the_all_taps_call():
    name = 'r256flat'
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    assert len(seq.layers) == 7
    with torch.no_grad():
        every, images = everything(seq, inputs)
        for index, layer in enumerate(seq.layers):
            bag, none = seq.generate(inputs, layer=layer, images=False)
            assert none is None and torch.equal(bag.h, every[index]), layer
            bag, pictures = seq.generate(inputs, layer=layer, images=True)
            assert torch.equal(bag.h, every[index]) and torch.equal(pictures, images), layer


@pytest.mark.parametrize('stop', ['layer2', 'layer3', 'attn3'])
def test_the_walk_stops_after_the_deepest_tap(stop):
    """r128, whose attention follows block 3.  With everything after `stop` set to NaN -- the
    later blocks, the attention when `stop` is before it, the output layer -- the tap is
    unchanged and finite: nothing after it ran."""
    name = 'r128'
    later = {'layer2': ('blocks.3.', 'blocks.4.', 'output_layer.'),
             'layer3': ('blocks.3.1.', 'blocks.4.', 'output_layer.'),
             'attn3': ('blocks.4.', 'output_layer.')}[stop]
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    assert seq.layers == ('layer0', 'layer1', 'layer2', 'layer3', 'attn3', 'layer4')
    with torch.no_grad():
        before = seq.generate(inputs, layer=stop, images=False)[0].h.clone()
        filled = 0
        for key, value in seq.generator.state_dict().items():
            if key.startswith(later) and '.u0' not in key:
                value.fill_(float('nan'))
                filled += 1
        assert filled
        after = seq.generate(inputs, layer=stop, images=False)[0].h
        assert torch.isnan(seq(inputs)).all()  # the new weights are in the context
    assert torch.equal(after, before) and bool(torch.isfinite(after).all())


def largest_activation(dims):
    """Floats per sample of the walk's largest tensor: a block's upsampled input or its output."""
    return max(4 * (dims['bottom_width'] << i)**2 * max(cin, cout)
               for i, (cin, cout, _) in enumerate(bigganref.blocks_of(dims)))


def workspace_bytes(ctx, n):
    """milan_gan_workspace_bytes and, where it is 0, the message: no launch, no allocation."""
    size = int(ctx.lib.milan_gan_workspace_bytes(ctx._h, n))
    return size, (ctx.lib.milan_last_error().decode() if size == 0 else '')


def test_a_batch_the_walk_cannot_take_is_refused_before_any_launch():
    # past the 2^31-element range of the GEMM's indices, far below the grid's z limit
    name = 'r128'
    dims = CASES[name][0]
    seq = guarded(model_of(name))
    inputs = inputs_of(name)
    (_, images64), (_, images32) = bigganref.shape_reference(name)
    with torch.no_grad():
        bigganref.check(f'{name} images before the refusals', seq(inputs), images64, images32)
        ctx = seq.generator._context()
        assert workspace_bytes(ctx, 8)[0] > 0
        floats = largest_activation(dims)
        first_bad = -(-2**31 // floats)
        assert 8 < first_bad <= 65535
        assert workspace_bytes(ctx, first_bad - 1)[0] > 0
        size, message = workspace_bytes(ctx, first_bad)
        assert size == 0 and 'split the batch' in message and '2^31' in message, message
        for n in (0, -1):
            assert workspace_bytes(ctx, n)[0] == 0
        bigganref.check(f'{name} images after the refusals', seq(inputs), images64, images32)

    # past the grid's z limit on a generator too narrow to reach 2^31 elements first (and with
    # z chunks of one column and a shared_dim of 3, which no other case has)
    narrow = bigganref.make_dims(32, 4, 0, 4, 3, 2, hier=True, bottom_width=1)
    assert narrow['chunk'] == 1 and 65536 * largest_activation(narrow) < 2**31
    sd = bigganref.weights(narrow, seed=760)
    z, hard, _ = bigganref.latents(narrow, 2, seed=860)
    model = generators.from_state_dict(bigganref.cast(sd, torch.float32), BN_eps=narrow['bn_eps'],
                                       bottom_width=1)
    seq = guarded(generators.SeqBigGAN(model.cuda()))
    with torch.no_grad():
        ctx = seq.generator._context()
        assert workspace_bytes(ctx, 65535)[0] > 0
        size, message = workspace_bytes(ctx, 65536)
        assert size == 0 and 'split the batch' in message and '65535' in message, message
        assert '2^31' not in message
        # GanContext.run reports it the same way (the outputs asked for are 16 MB)
        many = torch.zeros(65536, narrow['dim_z'], device='cuda')
        with pytest.raises(ValueError, match='split the batch'):
            ctx.run(many, torch.zeros(65536, dtype=torch.int64, device='cuda'), taps=(0,))
        del many
        want = bigganref.forward(sd, z, hard, narrow)
        ref32 = bigganref.forward(bigganref.cast(sd, torch.float32), z.float(), hard, narrow)
        taps, got = everything(seq, generators.GInputs(z.float().cuda(), hard.cuda()))
    assert got.shape == (2, 3, 8, 8)
    for index, layer in enumerate(seq.layers):
        bigganref.check(f'narrow {layer} after the refusals', taps[index], want[0][layer],
                        ref32[0][layer])
    bigganref.check('narrow images after the refusals', got, want[1], ref32[1])
