"""CPU tests of the VGG classifiers: `classifiers.VGGClassifier`'s module tree, keys and layers
against torchvision's (written out below: torchvision is not needed), the `features.N` ->
`vgg.B.J` renaming, `rekey_vgg16_places`, `hip.level_shapes` / `make_dims` for the new trunk
kind, the eager forward against tests/vggref.py bit for bit, the hook path of
`ablations.ablated` / `activations`, and the new entry points' declarations.
"""
import ctypes
import inspect
import pathlib
import re

import pytest
import torch

import vggref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, hip, synthetic

REPO = pathlib.Path(__file__).resolve().parent.parent
CONFIGS = ('vgg11', 'vgg13', 'vgg16', 'vgg19')

# torchvision.models.vggNN().features, module by module: C = Conv2d, R = ReLU, M = MaxPool2d
FEATURES = {
    'vgg11': 'CRM CRM CRCRM CRCRM CRCRM',
    'vgg13': 'CRCRM CRCRM CRCRM CRCRM CRCRM',
    'vgg16': 'CRCRM CRCRM CRCRCRM CRCRCRM CRCRCRM',
    'vgg19': 'CRCRM CRCRM CRCRCRCRM CRCRCRCRM CRCRCRCRM',
}
# ... the indices of its convs, and the reference's LAYERS.VGGnn (src/exemplars/models.py)
CONVS = {
    'vgg11': (0, 3, 6, 8, 11, 13, 16, 18),
    'vgg13': (0, 2, 5, 7, 10, 12, 15, 17, 20, 22),
    'vgg16': (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28),
    'vgg19': (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34),
}
LAYERS = {
    'vgg11': ('features.0', 'features.3', 'features.8', 'features.13', 'features.18'),
    'vgg13': ('features.2', 'features.7', 'features.12', 'features.17', 'features.22'),
    'vgg16': ('features.2', 'features.7', 'features.14', 'features.21', 'features.28'),
    'vgg19': ('features.2', 'features.7', 'features.16', 'features.25', 'features.34'),
}
# the library's names of the same convs
TRUNK_KEYS = {
    'vgg11': ('1.0', '2.0', '3.0', '3.1', '4.0', '4.1', '5.0', '5.1'),
    'vgg13': ('1.0', '1.1', '2.0', '2.1', '3.0', '3.1', '4.0', '4.1', '5.0', '5.1'),
    'vgg16': ('1.0', '1.1', '2.0', '2.1', '3.0', '3.1', '3.2', '4.0', '4.1', '4.2', '5.0', '5.1',
              '5.2'),
    'vgg19': ('1.0', '1.1', '2.0', '2.1', '3.0', '3.1', '3.2', '3.3', '4.0', '4.1', '4.2', '4.3',
              '5.0', '5.1', '5.2', '5.3'),
}
KINDS = {'C': torch.nn.Conv2d, 'R': torch.nn.ReLU, 'M': torch.nn.MaxPool2d}


def ratio_of(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('config', CONFIGS)
def test_module_tree_and_keys_are_torchvisions(config):
    model = classifiers.VGGClassifier(config, num_classes=10, width=8, hidden=24)
    assert isinstance(model, classifiers.NativeClassifier)
    assert [name for name, _ in model.named_children()] == ['features', 'avgpool', 'classifier']
    letters = FEATURES[config].replace(' ', '')
    assert len(model.features) == len(letters)
    for module, letter in zip(model.features, letters):
        assert type(module) is KINDS[letter]
    assert [i for i, letter in enumerate(letters) if letter == 'C'] == list(CONVS[config])
    cin, widths = 3, iter(m * 8 for m, group in zip((1, 2, 4, 8, 8), FEATURES[config].split())
                          for _ in range(group.count('C')))
    for index in CONVS[config]:
        conv, cout = model.features[index], next(widths)
        assert (conv.in_channels, conv.out_channels) == (cin, cout)
        assert (conv.kernel_size, conv.stride, conv.padding) == ((3, 3), (1, 1), (1, 1))
        assert model.features[index + 1].inplace
        cin = cout
    for module in model.features:
        if isinstance(module, torch.nn.MaxPool2d):
            assert (module.kernel_size, module.stride, module.padding) == (2, 2, 0)
    assert isinstance(model.avgpool, torch.nn.AdaptiveAvgPool2d)
    assert tuple(model.avgpool.output_size) == (7, 7)
    assert [type(m).__name__ for m in model.classifier] == [
        'Linear', 'ReLU', 'Dropout', 'Linear', 'ReLU', 'Dropout', 'Linear']
    want_keys = [f'features.{i}.{leaf}' for i in CONVS[config] for leaf in ('weight', 'bias')]
    want_keys += [f'classifier.{i}.{leaf}' for i in (0, 3, 6) for leaf in ('weight', 'bias')]
    assert list(model.state_dict().keys()) == want_keys
    assert tuple(model.state_dict()['classifier.0.weight'].shape) == (24, 64 * 49)
    assert tuple(model.state_dict()['classifier.6.weight'].shape) == (10, 24)
    # a torchvision-keyed state dict loads
    model.load_state_dict(vggref.make_state_dict(1, config, 8, 24, 10), strict=True)
    assert model.layers == LAYERS[config] == vggref.LAYERS[config]
    assert hip.vgg_level_names(synthetic.VGG_BLOCKS[config]) == LAYERS[config]
    # features.N -> vgg.B.J and back
    keys = model.trunk_keys()
    assert list(keys) == [f'features.{i}' for i in CONVS[config]]
    assert list(keys.values()) == [f'vgg.{name}' for name in TRUNK_KEYS[config]]
    back = {new: old for old, new in keys.items()}
    assert len(back) == len(keys) and all(back[keys[old]] == old for old in keys)
    # the last conv of a block is the block's layer
    for level, layer in enumerate(LAYERS[config]):
        block, conv = keys[layer].split('.')[1:]
        assert int(block) == level + 1
        assert int(conv) == synthetic.VGG_BLOCKS[config][level] - 1


def test_tables_and_defaults():
    assert synthetic.VGG_BLOCKS == {'vgg11': (1, 1, 2, 2, 2), 'vgg13': (2, 2, 2, 2, 2),
                                    'vgg16': (2, 2, 3, 3, 3), 'vgg19': (2, 2, 4, 4, 4)}
    assert synthetic.VGG_CHANNELS == (1, 2, 4, 8, 8)
    sig = inspect.signature(classifiers.VGGClassifier.__init__)
    defaults = {k: p.default for k, p in sig.parameters.items() if k != 'self'}
    assert defaults == dict(config='vgg16', num_classes=1000, width=64, hidden=4096,
                            precision='auto')
    for bad in (dict(config='vgg16_bn'), dict(width=12), dict(precision='f16')):
        with pytest.raises(ValueError):
            classifiers.VGGClassifier(**{'hidden': 8, 'width': 8, **bad})
    sd = synthetic.vgg_state_dict('vgg13', seed=3, width=8, hidden=16, classes=5)
    assert vggref.config_of(sd) == 'vgg13'
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        k: tuple(v.shape) for k, v in vggref.make_state_dict(3, 'vgg13', 8, 16, 5).items()}


def test_rekey_vgg16_places():
    own = classifiers.VGGClassifier('vgg16', num_classes=365, width=8, hidden=16).state_dict()
    names = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2', 'conv3_1', 'conv3_2', 'conv3_3',
             'conv4_1', 'conv4_2', 'conv4_3', 'conv5_1', 'conv5_2', 'conv5_3']
    places = {}
    for name, index in zip(names, CONVS['vgg16']):
        for leaf in ('weight', 'bias'):
            places[f'features.{name}.{leaf}'] = own[f'features.{index}.{leaf}']
    for name, index in (('fc6', 0), ('fc7', 3), ('fc8a', 6)):
        for leaf in ('weight', 'bias'):
            places[f'classifier.{name}.{leaf}'] = own[f'classifier.{index}.{leaf}']
    new = classifiers.rekey_vgg16_places(places)
    assert list(new.keys()) == list(own.keys())
    assert all(new[k] is own[k] for k in own)
    # fc8 is the other name of the last layer; torchvision's names pass through
    again = dict(places)
    again['classifier.fc8.weight'] = again.pop('classifier.fc8a.weight')
    assert set(classifiers.rekey_vgg16_places(again)) == set(own)
    assert list(classifiers.rekey_vgg16_places(dict(own)).keys()) == list(own.keys())
    model = classifiers.VGGClassifier('vgg16', num_classes=365, width=8, hidden=16)
    model.load_state_dict(new, strict=True)
    for bad in ('features.conv6_1.weight', 'features.conv1_3.weight', 'features.1.weight',
                'classifier.fc9.weight', 'classifier.1.bias', 'avgpool.weight',
                'features.conv1_1.running_mean', 'features.conv1_1', 'conv1_1.weight'):
        with pytest.raises(KeyError):
            classifiers.rekey_vgg16_places({bad: torch.empty(1)})
    with pytest.raises(KeyError, match='two keys'):
        classifiers.rekey_vgg16_places({'classifier.fc8.weight': torch.empty(1),
                                        'classifier.fc8a.weight': torch.empty(1)})


@pytest.mark.parametrize('config', ('vgg11', 'vgg16'))
@pytest.mark.parametrize('geo', ((32, 32), (45, 38), (224, 224)))
def test_level_shapes_are_what_forward_hooks_see(config, geo):
    model = classifiers.VGGClassifier(config, num_classes=4, width=8, hidden=8).eval()
    x = torch.zeros(1, 3, *geo)
    taps = model.activations(x, model.layers)
    shapes = hip.level_shapes(hip.TRUNK_VGG, 8, *geo)
    assert [tuple(taps[layer].shape[1:]) for layer in model.layers] == shapes
    assert shapes[0] == (8, *geo) and shapes[4][0] == 64


def test_make_dims_recognises_the_vgg_trunk():
    pre = 'encoder.encoder.model.'
    model = classifiers.VGGClassifier('vgg11', num_classes=4, width=16, hidden=8)
    sd = {}
    for old, new in model.trunk_keys().items():
        sd[f'{pre}{new}.weight'] = model.state_dict()[f'{old}.weight']
    dims = hip.make_dims(sd, 1)
    assert dims.trunk_kind == hip.TRUNK_VGG == 5
    assert dims.trunk_width == 16 and dims.feature_size == 23 * 16
    # torchvision's own `features.0.weight` still means AlexNet
    asd = {pre + k: v for k, v in synthetic.alexnet_state_dict(seed=1, width=8).items()}
    assert hip.make_dims(asd, 1).trunk_kind == hip.TRUNK_ALEXNET


@pytest.mark.parametrize('config', CONFIGS)
def test_eager_forward_is_the_restatement_bit_for_bit(config):
    sd = vggref.make_state_dict(7, config, 8, 24, 10)
    model = classifiers.VGGClassifier(config, 10, 8, 24)
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = vggref.make_images(7, 2, (45, 38))
    want_logits, want_taps = vggref.forward(x, sd)
    with torch.no_grad():
        assert not model.runs_natively(x)
        got = model(x)
    assert got.dtype == torch.float32 and torch.equal(got, want_logits)
    taps = model.activations(x, model.layers)
    for layer, want in zip(model.layers, want_taps):
        assert torch.equal(taps[layer], want)
    # ... and sits in the fp32 class of its own float64 run
    want64 = vggref.forward(x.double(), sd)[0]
    ratio = ratio_of(got, want64)
    print(f'VGG host {config} eager fp32 vs float64: {ratio / FEATURE_CLASS:.3f} x bound')
    assert ratio <= FEATURE_CLASS


def test_hook_path_of_ablated_and_activations():
    sd = vggref.make_state_dict(9, 'vgg13', 8, 24, 10)
    model = classifiers.VGGClassifier('vgg13', 10, 8, 24)
    model.load_state_dict(sd, strict=True)
    model.eval()
    x = vggref.make_images(9, 2, (40, 33))
    units = [('features.7', 3), ('features.22', 0), ('features.22', 63)]
    want_logits, want_taps = vggref.forward(x, sd, units)
    with torch.no_grad(), ablations.ablated(model, units):
        got = model(x)
        taps = model.activations(x, ['features.22', 'features.7'])
    assert torch.equal(got, want_logits)
    assert torch.equal(taps['features.7'], want_taps[1])
    assert torch.equal(taps['features.22'], want_taps[4])
    assert not bool(taps['features.7'][:, 3].any()) and bool(want_taps[1][:, 2].any())
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
    with pytest.raises(KeyError):
        model.activations(x, 'features.99')
    with pytest.raises(ValueError):
        with ablations.ablated(model, [('features.5', 0)]):
            pass
    # the restatement takes level numbers as well as names, and says when there is no logit
    assert torch.equal(vggref.forward(x, sd, [(1, 3), (4, 0), (4, 63)])[0], want_logits)
    logits, few = vggref.forward(x[:, :, :20, :20], sd)
    assert logits is None and len(few) == 5 and tuple(few[4].shape[2:]) == (1, 1)
    assert len(vggref.forward(x[:, :, :7, :9], sd)[1]) == 3


def test_entry_points_are_declared_and_exported():
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    assert re.search(r'\bMILAN_TRUNK_VGG\s*=\s*5\b', header)
    assert re.search(r'#define MILAN_ABI_VERSION 11\b', header)
    lib = hip.load_library()
    for name in ('milan_set_vgg_head', 'milan_vgg_trace'):
        assert re.search(rf'\b{name}\s*\(', header), name
        assert name in hip.SIGNATURES and name in hip.PROBED and hasattr(lib, name)
    assert hip.TRUNK_VGG == 5 and hip._FEATURE_MULT[hip.TRUNK_VGG] == 23
    assert callable(hip.Context.set_vgg_head) and callable(hip.Context.vgg_trace)
    assert 'vgg_head' in inspect.signature(hip.Context.__init__).parameters
    # (a context needs a GPU to exist: the refusals are in tests/test_gpu_vgg.py)
    assert lib.milan_vgg_trace(None, None, None) == hip.ERR_ARG
    none = ctypes.c_void_p()
    assert lib.milan_set_vgg_head(none, *([None, None, 1, 1] * 3), None) == hip.ERR_ARG
    assert b'milan_set_vgg_head' in lib.milan_last_error()
