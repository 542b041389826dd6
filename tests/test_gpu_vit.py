"""GPU tests of milan_amd.vits.VisionTransformer's native walk (milan_vit_run): the fc1
taps and the CLS output against tests/vitref.py in float64, the walk's properties (taps alone,
batch invariance, early stop, the choice between the two forwards, the context cache) and a
dissection end to end through exemplars.discriminative.

Bound: max|got - want| <= max(4 x e32, FEATURE_CLASS x max|want|), e32 = the error of vitref
in float32 on the CPU against vitref in float64 on that same case (vitref.check).  The tests
print the measured multiple of the bound per tensor (`VIT ...` lines); DESIGN 4.24 quotes
the worst.
"""
import functools
import io

import numpy
import pytest
import torch
from torch.utils import data

import vitref
from milan_amd import exemplars, vits
from oracle import exemplars_oracle as E

pytestmark = pytest.mark.gpu

#        res patch  W heads depth hidden batch
CASES = [(16, 8, 32, 2, 2, 64, 3),       # T = 5: fewer tokens than any tile
         (40, 8, 48, 3, 3, 192, 5),
         (64, 8, 64, 2, 2, 256, 2),      # T = 65
         (112, 8, 64, 1, 1, 256, 2),     # T = 197
         (224, 8, 32, 2, 1, 128, 1),     # the full 785 tokens at toy width
         (224, 8, 384, 6, 12, 1536, 1)]  # the true ViT-S/8


@functools.lru_cache(maxsize=None)
def reference(index):
    """(dims, float64 weights, float64 images, float64 taps and output, float32 ones): computed
    once per case and left unchanged."""
    *shape, batch = CASES[index]
    dims = vitref.make_dims(*shape)
    sd = vitref.weights(dims, seed=100 + index)
    x = vitref.images(dims, batch, seed=200 + index)
    with torch.no_grad():
        want = vitref.forward(sd, x, dims)
        ref32 = vitref.forward(vitref.cast(sd, torch.float32), x.float(), dims)
    return dims, sd, x, want, ref32


def model_of(index, **kwargs):
    dims, sd, *_ = reference(index)
    model = vits.from_state_dict(vitref.cast(sd, torch.float32), num_heads=dims['heads'],
                                 **kwargs)
    return model.cuda()


def guarded(model):
    """The eager path raises: whatever returns came from the native walk."""
    def refuse(images):
        raise AssertionError('the eager path ran')
    model.forward_eager = refuse
    return model


@pytest.mark.parametrize('index', range(len(CASES)))
def test_taps_and_forward_against_float64(index):
    dims, sd, x, (taps64, out64), (taps32, out32) = reference(index)
    model = guarded(model_of(index))
    images = x.float().cuda()
    with torch.no_grad():
        assert model.runs_natively(images)
        acts = model.activations(images, model.layers)
        out = model(images)
    assert list(acts) == list(model.layers)
    for i, name in enumerate(model.layers):
        vitref.check(f'case {index + 1} {name}', acts[name], taps64[i], taps32[i])
    vitref.check(f'case {index + 1} forward', out, out64, out32)


def test_every_tap_alone_equals_the_all_layers_call():
    model = guarded(model_of(1))
    images = reference(1)[2].float().cuda()
    with torch.no_grad():
        every = model.activations(images, model.layers)
        for name in model.layers:
            assert torch.equal(model.activations(images, name)[name], every[name]), name
        pair = model.activations(images, [model.layers[2], model.layers[0]])
    assert list(pair) == [model.layers[2], model.layers[0]]
    assert all(torch.equal(pair[name], every[name]) for name in pair)


def test_an_image_does_not_depend_on_its_batch():
    model = guarded(model_of(1))
    images = reference(1)[2].float().cuda()
    with torch.no_grad():
        batch = model.activations(images[:3], model.layers)
        out = model(images[:3])
        for i in range(3):
            alone = model.activations(images[i:i + 1], model.layers)
            for name in model.layers:
                assert torch.equal(alone[name], batch[name][i:i + 1]), (i, name)
            assert torch.equal(model(images[i:i + 1]), out[i:i + 1])
        # 5 images in passes of 2, 2 and 1
        whole = model.activations(images, model.layers)
        whole_out = model(images)
        model.max_images = 2
        split = model.activations(images, model.layers)
        for name in model.layers:
            assert torch.equal(split[name], whole[name]), name
        assert torch.equal(model(images), whole_out)


def test_the_walk_stops_after_the_deepest_tap():
    """With blocks 1 and 2 and blocks.0.mlp.fc2 set to NaN, the tap of blocks.0.mlp.fc1 is
    unchanged and finite: nothing after it ran."""
    model = guarded(model_of(1))
    images = reference(1)[2].float().cuda()
    name = 'blocks.0.mlp.fc1'
    with torch.no_grad():
        before = model.activations(images, name)[name].clone()
        for key, value in model.state_dict().items():
            if key.startswith(('blocks.1.', 'blocks.2.', 'blocks.0.mlp.fc2.')):
                value.fill_(float('nan'))
        after = model.activations(images, name)[name]
        assert torch.isnan(model(images)).all()  # the new weights are in the context
    assert torch.equal(after, before) and bool(torch.isfinite(after).all())


def test_a_forward_hook_selects_the_eager_path():
    model = model_of(0)
    images = reference(0)[2].float().cuda()
    with torch.no_grad():
        native = model.activations(images, 'blocks.1.mlp.fc1')['blocks.1.mlp.fc1']
    seen = []
    handle = model.blocks[1].mlp.fc1.register_forward_hook(
        lambda module, inputs, output: seen.append(output.detach()))
    try:
        with torch.no_grad():
            assert not model.runs_natively(images)
            model(images)
            assert len(seen) == 1
            model.activations(images, 'blocks.0.mlp.fc1')
            assert len(seen) == 2
    finally:
        handle.remove()
    with torch.no_grad():
        assert model.runs_natively(images)
    # the two paths agree to fp32 rounding (both are held to float64 elsewhere)
    assert (seen[0] - native).abs().max() <= 1e-4 * native.abs().max()


def test_training_mode_and_grad_are_differentiable():
    model = model_of(0)
    images = reference(0)[2].float().cuda()
    assert not model.runs_natively(images)  # grad is enabled here
    model(images).sum().backward()
    assert float(model.blocks[0].attn.qkv.weight.grad.abs().sum()) > 0
    model.zero_grad()
    model.train()
    with torch.no_grad():
        assert not model.runs_natively(images)
    out = model(images)
    assert out.requires_grad


def test_a_cpu_tensor_takes_the_eager_path():
    dims, sd, x, (taps64, out64), (taps32, out32) = reference(0)
    model = vits.from_state_dict(vitref.cast(sd, torch.float32), num_heads=dims['heads'])
    with torch.no_grad():
        assert not model.runs_natively(x.float())
        vitref.check('cpu forward', model(x.float()), out64, out32)


def test_errors():
    model = guarded(model_of(0))
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match='interpolation'):
            model(torch.zeros(1, 3, 24, 24, device='cuda'))
        with pytest.raises(NotImplementedError, match='interpolation'):
            model.activations(torch.zeros(1, 3, 24, 24, device='cuda'), 'blocks.0.mlp.fc1')
        with pytest.raises(KeyError):
            model.activations(torch.zeros(1, 3, 16, 16, device='cuda'), 'blocks.9.mlp.fc1')
        # head size 20 has no attention kernel: an error that names it, not a fault
        odd = vits.VisionTransformer(img_size=16, patch_size=8, embed_dim=40, depth=1,
                                     num_heads=2).cuda().eval()
        with pytest.raises(ValueError, match='head size 20'):
            odd(torch.zeros(1, 3, 16, 16, device='cuda'))
    torch.cuda.synchronize()


def test_new_weights_reach_the_native_path():
    """load_state_dict changes the tensors' versions: the cached context is rebuilt."""
    dims, sd, x, *_ = reference(0)
    model = guarded(model_of(0))
    images = x.float().cuda()
    with torch.no_grad():
        first = model(images)
        other = vitref.weights(dims, seed=999)
        model.load_state_dict(vitref.cast(other, torch.float32), strict=True)
        second = model(images)
        taps64, out64 = vitref.forward(other, x, dims)
        taps32, out32 = vitref.forward(vitref.cast(other, torch.float32), x.float(), dims)
    assert not torch.equal(first, second)
    vitref.check('reloaded forward', second, out64, out32)


# ---- dissect end to end (the helper of tests/test_gpu_activations.py, restated) ---------
def dissect(model, dataset, layer, tmp_path, source):
    """exemplars.discriminative against the oracle's `compute` fed `source(images)` = the
    layer's spatialized activations for the same batches."""
    kwargs = dict(k=3, quantile=.9, output_size=16, batch_size=5)
    torch.manual_seed(31)
    topk, rq = exemplars.discriminative(model, dataset, layer=layer, image_size=40,
                                        transform_hiddens=exemplars.spatialize_vit_mlp,
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


def test_dissect_a_vit_natively(tmp_path):
    model = guarded(model_of(1))
    g = torch.Generator().manual_seed(2306)
    dataset = data.TensorDataset(torch.rand(23, 3, 40, 40, generator=g))
    layer = 'blocks.1.mlp.fc1'

    def source(images):
        with torch.no_grad():
            assert model.runs_natively(images)
            return exemplars.spatialize_vit_mlp(model.activations(images, layer)[layer])

    want = dissect(model, dataset, layer, tmp_path, source)
    assert want['ids'].shape == (192, 3)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
