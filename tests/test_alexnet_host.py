"""Host tests of classifiers.AlexNetClassifier under milan_amd.ablations: the torch path (CPU)
against the reference's goldens (tests/golden/reference_goldens_alexnet.*, made by the
reference's own src/utils/ablations.py over an `alexnet_seq`-shaped stand-in) and against the
restatement tests/alexref.py; and `hip.level_shapes` of the three trunk families against the
shapes forward hooks see on the eager modules."""
import collections

import pytest
import torch
from torch import nn
from torch.utils import data

import alexref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, hip

SMALL = ((63, 63), (95, 127))   # (the two large geometries run on the GPU)


@pytest.fixture(scope='module')
def gold():
    tensors, meta = alexref.load_goldens()
    return tensors, meta, alexref.state_dict(meta)


def make_model(meta, sd, **kwargs):
    model = classifiers.AlexNetClassifier(meta['classes'], meta['width'], meta['hidden'],
                                          **kwargs)
    model.load_state_dict(sd, strict=True)
    return model.eval()


def cases_of(meta):
    return {name: [tuple(u) for u in units] for name, units in meta['cases'].items()}


def test_module_tree_is_alexnet_seq(gold):
    _, meta, sd = gold
    model = make_model(meta, sd)
    assert [name for name, _ in model.named_children()] == meta['modules']
    assert list(model.state_dict().keys()) == meta['state_dict_keys']
    assert model.layers == alexref.LAYERS == ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')
    assert [m.out_channels for m in (model.conv1, model.conv2, model.conv3, model.conv4,
                                     model.conv5)] == list(alexref.channels(meta['width']))
    named = dict(model.named_modules())
    assert all(layer in named for layer in ('fc6', 'fc7', 'linear8'))
    # torchvision's sizes by default
    full = classifiers.AlexNetClassifier()
    assert full.fc6.weight.shape == (4096, 9216) and full.linear8.weight.shape == (1000, 4096)
    assert sum(p.numel() for p in full.parameters()) == 61100840
    with pytest.raises(ValueError, match='precision'):
        classifiers.AlexNetClassifier(precision='f16')
    # the ResNet class still refuses the name
    with pytest.raises(ValueError, match='not supported'):
        classifiers.ResNetClassifier('alexnet')


def test_checkpoint_of_the_editing_experiment_loads(gold):
    """experiments/edit.py saves ImageClassifier(alexnet_seq).state_dict(): `model.` + names."""
    _, meta, sd = gold
    classifier = ablations.ImageClassifier(
        classifiers.AlexNetClassifier(meta['classes'], meta['width'], meta['hidden']))
    classifier.load_state_dict({'model.' + k: v for k, v in sd.items()}, strict=True)
    assert torch.equal(classifier.model.linear8.bias, sd['linear8.bias'])


@pytest.mark.parametrize('geo', SMALL)
def test_eager_and_hooks_against_goldens(gold, geo):
    tensors, meta, sd = gold
    model = make_model(meta, sd)
    images = alexref.images(meta, geo)
    tag = f'{geo[0]}x{geo[1]}'
    classifier = ablations.ImageClassifier(model)
    dataset = data.TensorDataset(images, tensors[f'{tag}.targets'])
    for name, case in cases_of(meta).items():
        want = tensors[f'{tag}.{name}.logits']
        with ablations.ablated(model, case) as edited, torch.no_grad():
            assert not edited.runs_natively(images)
            got = edited(images)
        # the same torch kernels on the same operands as the reference ran
        torch.testing.assert_close(got, want, rtol=0, atol=FEATURE_CLASS * float(want.abs().max()))
        kwargs = dict(batch_size=5, ablate=case, display_progress_as=None)
        assert torch.equal(classifier.predict(dataset, **kwargs),
                           tensors[f'{tag}.{name}.predictions'])
        result = meta['results'][f'{tag}.{name}']
        assert classifier.accuracy(dataset, **kwargs) == result['accuracy']
        accuracies = classifier.accuracies(dataset, **kwargs)
        assert {str(k): v for k, v in accuracies.items()} == result['accuracies']
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0
    with torch.no_grad():
        assert torch.equal(model.forward_eager(images), model(images))


@pytest.mark.parametrize('geo', SMALL)
def test_alexref_float32_against_goldens(gold, geo):
    tensors, meta, sd = gold
    images = alexref.images(meta, geo)
    for name, case in cases_of(meta).items():
        want = tensors[f'{geo[0]}x{geo[1]}.{name}.logits']
        got, _ = alexref.forward(images, sd, case)
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= FEATURE_CLASS, (geo, name, err)
        assert torch.equal(got.argmax(dim=-1), tensors[f'{geo[0]}x{geo[1]}.{name}.predictions'])


def test_activations_on_cpu_equal_alexref(gold):
    _, meta, sd = gold
    model = make_model(meta, sd)
    images = alexref.images(meta, (95, 127))
    case = cases_of(meta)['mixed']
    _, want = alexref.forward(images, sd, case)
    with ablations.ablated(model, case):
        got = model.activations(images, alexref.LAYERS)
        fc = model.activations(images, 'fc6')['fc6']
    assert list(got) == list(alexref.LAYERS)
    for layer in alexref.LAYERS:
        # post-ReLU and post-mask: what the next layer reads
        assert float(got[layer].min()) >= 0
        torch.testing.assert_close(got[layer], want[layer], rtol=0,
                                   atol=FEATURE_CLASS * float(want[layer].abs().max()))
    for layer, unit in case:
        assert not got[layer][:, unit].any()
    assert fc.shape == (len(images), meta['hidden'])
    with pytest.raises(KeyError):
        model.activations(images, 'layer1')
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


def test_fc_layers_cannot_be_zeroed(gold):
    _, meta, sd = gold
    model = make_model(meta, sd)
    images = alexref.images(meta, (63, 63))
    # the native check knows the five edit points
    with pytest.raises(ValueError, match='not found in model'):
        with ablations.ablated(model, [('fc6', 0)]):
            pass
    with pytest.raises(ValueError, match='not found in model'):
        with ablations.ablated(model, [('layer1', 0)]):
            pass
    # the torch path of a foreign module: `zero` refuses 2-D features, as the reference's does
    foreign = nn.Sequential(collections.OrderedDict(model.named_children()))
    with ablations.ablated(foreign, [('fc6', 0)]) as edited, torch.no_grad():
        with pytest.raises(ValueError, match='expected 4D'):
            edited(images)
    with ablations.ablated(foreign, [('conv3', 2)]) as edited, torch.no_grad():
        got = edited(images)
    with ablations.ablated(model, [('conv3', 2)]) as edited, torch.no_grad():
        assert torch.equal(edited(images), got)
    # a custom rule edits in training mode only
    with pytest.raises(ValueError, match='zero'):
        with ablations.ablated(model, [('conv3', 2)], rule=lambda units: (lambda x: x * 2)):
            pass


def test_fit_trains_the_three_linear_layers_only(gold):
    _, meta, sd = gold
    model = make_model(meta, sd)
    classifier = ablations.ImageClassifier(model)
    g = torch.Generator().manual_seed(3)
    dataset = data.TensorDataset(torch.randn(8, 3, 63, 63, generator=g),
                                 torch.randint(meta['classes'], (8,), generator=g))
    torch.manual_seed(5)
    classifier.fit(dataset, batch_size=4, max_epochs=2, hold_out=[6, 7],
                   layers=['fc6', 'fc7', 'linear8'], ablate=[('conv5', 1)],
                   display_progress_as=None)
    after = model.state_dict()
    for key, before in sd.items():
        changed = not torch.equal(after[key], before)
        assert changed == key.startswith(('fc6', 'fc7', 'linear8')), key
    with pytest.raises(KeyError, match='fc8'):
        classifier.fit(dataset, hold_out=[6, 7], layers=['fc8'], display_progress_as=None)


def test_unit_scores_on_cpu_is_the_loop(gold):
    tensors, meta, sd = gold
    model = make_model(meta, sd)
    classifier = ablations.ImageClassifier(model)
    dataset = data.TensorDataset(alexref.images(meta, (63, 63)), tensors['63x63.targets'])
    units = [('conv1', 0), ('conv5', 31)]
    scores = classifier.unit_scores(dataset, units, batch_size=5, display_progress_as=None)
    assert scores == [classifier.accuracy(dataset, batch_size=5, ablate=[unit],
                                          display_progress_as=None) for unit in units]


LEVEL_SHAPE_CASES = (
    (lambda: classifiers.AlexNetClassifier(4, 8, 8), hip.TRUNK_ALEXNET, ((63, 63), (95, 127))),
    (lambda: classifiers.PlacesAlexNetClassifier(4, 8, 8), hip.TRUNK_ALEXNET_PLACES,
     ((35, 38), (99, 131), (227, 227))),
    (lambda: classifiers.ResNetClassifier('resnet18', 4, 8), hip.TRUNK_BASIC, ((33, 47),)),
    (lambda: classifiers.ResNetClassifier('resnet50', 4, 8), hip.TRUNK_BOTTLENECK, ((33, 47),)),
)


@pytest.mark.parametrize('make,kind,geometries', LEVEL_SHAPE_CASES,
                         ids=('alexnet', 'places', 'resnet18', 'resnet50'))
def test_level_shapes_are_what_forward_hooks_see(make, kind, geometries):
    """`hip.level_shapes` (the tensors `Context.activations` allocates) against the eager
    modules of the three trunk families at width 8."""
    model = make().eval()
    seen = []
    for layer in model.layers:
        getattr(model, layer).register_forward_hook(
            lambda module, inputs, output: seen.append(tuple(output.shape[1:])))
    for h, w in geometries:
        del seen[:]
        x = torch.zeros(1, 3, h, w)
        with torch.no_grad():
            # (the trunk alone: the Places365 net's fc6 takes 227 x 227 only)
            for name, module in model.named_children():
                x = module(x)
                if name == model.layers[-1]:
                    break
        assert hip.level_shapes(kind, 8, h, w) == seen, (h, w)
