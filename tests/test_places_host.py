"""CPU tests of the two Places365 networks: tests/placesref.py against the reference's goldens,
`classifiers.PlacesAlexNetClassifier`'s module tree and eager forward, `OldResNet152`'s key
translation, aliases and eager forward, and the new entry points' declarations.

The float32 restatement is held to the goldens within the margin FEATURE_CLASS stands for
(fp32 GEMM class), measured against the float64 run of the same restatement; the tests print
the measured multiple (DESIGN 4.27 quotes it).
"""
import ctypes
import inspect
import pathlib
import re

import pytest
import torch

import placesref
from featclass import FEATURE_CLASS
from milan_amd import classifiers, hip

REPO = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def gold():
    tensors, meta = placesref.load_goldens()
    return tensors, meta


@pytest.fixture(scope='module')
def alex(gold):
    """The full-width seeded model, its images and the float64 logits with / without the LRN."""
    _, meta = gold
    sd = placesref.state_dict(meta)
    x = placesref.images(meta)
    want = {lrn: placesref.forward(x.double(), sd, include_lrn=lrn)[0] for lrn in (False, True)}
    return sd, x, want


def ratio_of(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('lrn', (False, True))
def test_restatement_reproduces_the_reference(gold, alex, lrn):
    tensors, _ = gold
    sd, x, want = alex
    golden = tensors[f'alexnet.lrn{int(lrn)}.logits']
    got, taps = placesref.forward(x, sd, include_lrn=lrn)
    assert got.dtype == torch.float32 and got.shape == golden.shape == (2, 365)
    assert [tuple(t.shape[1:]) for t in taps.values()] == [
        (96, 55, 55), (256, 27, 27), (384, 13, 13), (384, 13, 13), (256, 13, 13)]
    # three fp32 runs of one network -- the reference, the restatement, and both against the
    # float64 restatement -- sit within the fp32 GEMM class of each other
    for what, a, b in (('reference fp32 vs float64', golden, want[lrn]),
                       ('restatement fp32 vs float64', got, want[lrn]),
                       ('restatement fp32 vs reference fp32', got, golden.double())):
        ratio = ratio_of(a, b)
        print(f'PLACES host lrn={int(lrn)} {what}: {ratio / FEATURE_CLASS:.3f} x bound')
        assert ratio <= FEATURE_CLASS, (what, ratio)
    # the LRN is live: the two logit sets differ by far more than the bound
    assert ratio_of(want[True], want[False]) > 100 * FEATURE_CLASS


def test_lrn_pads_with_zeros_and_divides_by_the_window():
    x = torch.arange(1.0, 7.0, dtype=torch.float64).view(1, 6, 1, 1)
    got = placesref.lrn(x, 5, 0.5, 0.75).view(-1)
    sq = [v * v for v in range(1, 7)]
    for c in range(6):
        total = sum(sq[j] for j in range(max(0, c - 2), min(6, c + 3)))
        assert abs(float(got[c]) - (c + 1) / (1 + 0.5 * total / 5)**0.75) < 1e-12
    module = classifiers.LRN(5, 0.5, 0.75)
    assert torch.allclose(module(x), placesref.lrn(x, 5, 0.5, 0.75), rtol=1e-14, atol=0)


@pytest.mark.parametrize('lrn', (False, True))
@pytest.mark.parametrize('groups', (False, True))
@pytest.mark.parametrize('dropout', (False, True))
def test_module_tree_is_the_reference_one(gold, lrn, groups, dropout):
    _, meta = gold
    variant = meta['alexnet']['variants'][
        f'lrn={int(lrn)},groups={int(groups)},dropout={int(dropout)}']
    model = classifiers.PlacesAlexNetClassifier(include_lrn=lrn, split_groups=groups,
                                                include_dropout=dropout, hidden=64, width=32)
    assert [name for name, _ in model.named_children()] == variant['modules']
    # (hidden 64 keeps the test light: the fc shapes scale, everything else is the reference's)
    want = [(k, tuple(64 if d == 4096 else d for d in s)) for k, s in variant['state_dict']]
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == want
    assert model.layers == ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')
    assert isinstance(model, classifiers.NativeClassifier)


def test_classifier_defaults_and_arguments():
    sig = inspect.signature(classifiers.PlacesAlexNetClassifier.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert defaults == dict(num_classes=365, width=32, hidden=4096, include_lrn=False,
                            split_groups=True, include_dropout=False, precision='auto')
    with pytest.raises(ValueError):
        classifiers.PlacesAlexNetClassifier(width=12, hidden=8)
    with pytest.raises(ValueError):
        classifiers.PlacesAlexNetClassifier(width=8, hidden=8, precision='f16')


@pytest.mark.parametrize('lrn,groups', ((False, True), (True, True), (True, False)))
def test_eager_forward_equals_the_restatement(lrn, groups):
    sd = placesref.make_state_dict(5, 8, 72, 10, split_groups=groups)
    model = classifiers.PlacesAlexNetClassifier(10, 8, 72, include_lrn=lrn, split_groups=groups,
                                                include_dropout=True)
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = placesref.make_images(5, 3, (227, 227))
    with torch.no_grad():
        got = model(x)
    want, taps = placesref.forward(x.double(), sd, include_lrn=lrn)
    assert ratio_of(got, want) <= FEATURE_CLASS
    # the taps of the torch path (forward hooks) are the restatement's
    for layer in ('conv2', 'conv5'):
        tap = model.activations(x, layer)[layer]
        assert ratio_of(tap, taps[layer]) <= FEATURE_CLASS
    # no adaptive pool: another size fails in fc6, as the reference's Vectorize + fc6 do
    with pytest.raises(RuntimeError), torch.no_grad():
        model(x[:, :, :224, :224])


def test_rekey_maps_the_reference_keys_one_to_one(gold):
    _, meta = gold
    old = [(k, tuple(s)) for k, s in meta['resnet152']['state_dict']]
    assert old[0][0] == '0.weight' and old[-1][0] == '10.1.bias'
    stand_in = {k: torch.empty(s) for k, s in old}
    new = classifiers.rekey_old_resnet152(stand_in)
    assert len(new) == len(old)
    own = classifiers.ResNetClassifier('resnet152', 365).state_dict()
    assert {k: tuple(v.shape) for k, v in new.items()} == {k: tuple(v.shape)
                                                           for k, v in own.items()}
    # the same order, so values can be paired by position
    assert list(new.keys()) == list(own.keys())
    assert new['layer3.35.conv2.weight'] is stand_in['6.35.0.0.3.weight']
    assert new['layer2.0.downsample.1.running_var'] is stand_in['5.0.0.1.1.running_var']
    # torchvision's names pass through, nonsense does not
    assert list(classifiers.rekey_old_resnet152(dict(own)).keys()) == list(own.keys())
    for bad in ('2.weight', '4.0.0.0.2.weight', '4.0.0.1.2.weight', '10.0.weight', 'features.0'):
        with pytest.raises(KeyError):
            classifiers.rekey_old_resnet152({bad: torch.empty(1)})


def test_old_resnet152_eager_logits_and_aliases(gold):
    tensors, meta = gold
    r = meta['resnet152']
    tv = placesref.make_resnet152_state_dict(r['seed'], r['width'], r['classes'])
    model = classifiers.OldResNet152()
    own = list(model.state_dict().keys())
    old_names = [k for k, _ in r['state_dict']]
    # a checkpoint in the old names, without num_batches_tracked (a Torch7 conversion has none)
    old_sd = {old: tv[new] for old, new in zip(old_names, own)
              if not new.endswith('num_batches_tracked')}
    model.load_state_dict(old_sd, strict=True)
    model.eval()
    x = placesref.make_images(r['seed'], r['n_images'], tuple(r['geometry']))
    with torch.no_grad():
        got = model(x)
    ratio = ratio_of(got, tensors['resnet152.logits'].double())
    print(f'PLACES host OldResNet152 eager vs reference fp32: {ratio / FEATURE_CLASS:.3f} x bound')
    assert ratio <= FEATURE_CLASS
    # the fixed 7 x 7 pool: a smaller image fails, as the reference does
    with pytest.raises(RuntimeError), torch.no_grad():
        model(x[:, :, :192, :192])
    # aliases
    assert isinstance(model, classifiers.ResNetClassifier)
    for alias in ('0', '4', '5', '6', '7'):
        assert alias in model.layers
    small = x[:1]   # (the torch path runs the whole forward, the fixed pool included)
    by_alias = model.activations(small, ['5', 0, 'layer2'])
    assert set(by_alias) == {'5', 0, 'layer2'}
    assert torch.equal(by_alias['5'], by_alias['layer2'])
    assert tuple(by_alias[0].shape) == (1, 64, 112, 112)
    assert torch.equal(model.activations(small, 7)[7], model.activations(small, 'layer4')['layer4'])
    for unknown in ('3', 8, 'layer5', ''):
        with pytest.raises(KeyError):
            model.activations(small, unknown)


def test_entry_points_are_declared_and_exported():
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    assert re.search(r'\bMILAN_TRUNK_ALEXNET_PLACES\s*=\s*4\b', header)
    lib = hip.load_library()
    for name in ('milan_set_alexnet_lrn', 'milan_lrn'):
        assert re.search(rf'\b{name}\s*\(', header), name
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert hip.TRUNK_ALEXNET_PLACES == 4
    assert callable(hip.Context.set_alexnet_lrn)
    assert hip.Context.ALEXNET_LEVELS == ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')


def test_make_dims_recognises_the_places_trunk():
    sd = {'encoder.encoder.model.' + k: v
          for k, v in placesref.make_state_dict(3, 16, 8, 4).items() if k.startswith('conv')}
    dims = hip.make_dims(sd, 1)
    assert dims.trunk_kind == hip.TRUNK_ALEXNET_PLACES
    assert dims.trunk_width == 16 and dims.feature_size == 43 * 16
    # a ResNet's conv1 is still a ResNet's
    rsd = {'encoder.encoder.model.conv1.weight': torch.empty(8, 3, 7, 7)}
    assert hip.make_dims(rsd, 1, blocks=(2, 2, 2, 2)).trunk_kind == hip.TRUNK_BASIC


def test_lrn_setter_refuses_a_null_context():
    """(a context of another trunk kind needs a GPU to exist: tests/test_gpu_places.py)"""
    lib = hip.load_library()
    assert lib.milan_set_alexnet_lrn(None, 5, ctypes.c_float(1e-4),
                                     ctypes.c_float(0.75)) == hip.ERR_ARG
    assert b'milan_set_alexnet_lrn' in lib.milan_last_error()
