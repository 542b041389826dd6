"""CPU tests of milan_amd.ablations / milan_amd.classifiers and the C surface of the
classify entry points.  The goldens come from the reference's own src/utils/ablations.py
(tests/golden/make_golden_ablations.py); the torch paths here run the same ops in the same
order on the CPU, so they are compared with torch.equal."""
import copy
import ctypes
import pathlib
import re

import pytest
import torch
from torch import nn
from torch.utils import data

import ablref
from featclass import FEATURE_CLASS
from milan_amd import ablations, classifiers, hip, synthetic

REPO = pathlib.Path(__file__).resolve().parent.parent
NEW_ENTRY_POINTS = ('milan_set_ablation', 'milan_classify_workspace_bytes', 'milan_classify',
                    'milan_classify_sweep')


@pytest.fixture(scope='module')
def gold():
    return ablref.load_goldens()


def geometries(meta):
    return [tuple(g) for g in meta['geometries']]


def native_model(config, tensors, meta):
    model = classifiers.ResNetClassifier(config, num_classes=meta['configs'][config]['classes'],
                                         width=meta['width'])
    model.load_state_dict(ablref.state_dict(config, tensors, meta), strict=True)
    return model.eval()


class Foreign(nn.Module):
    """The same network behind a class the package knows nothing about: the hook path."""

    def __init__(self, inner):
        super().__init__()
        for name, child in inner.named_children():
            self.add_module(name, child)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def cases_of(meta, config):
    return {name: [(layer, unit) for layer, unit in units]
            for name, units in meta['configs'][config]['cases'].items()}


@pytest.mark.parametrize('foreign', [False, True], ids=['eager', 'hooks'])
@pytest.mark.parametrize('config', ['resnet18', 'resnet50'])
def test_torch_paths_reproduce_the_reference(gold, config, foreign):
    tensors, meta = gold
    model = native_model(config, tensors, meta)
    if foreign:
        model = Foreign(model).eval()
    classifier = ablations.ImageClassifier(model)
    for h, w in geometries(meta):
        tag = f'{config}.{h}x{w}'
        images = tensors[f'images.{h}x{w}']
        dataset = data.TensorDataset(images, tensors[f'{tag}.targets'])
        for name, case in cases_of(meta, config).items():
            with ablations.ablated(model, case) as edited, torch.no_grad():
                logits = edited(images)
            assert torch.equal(logits, tensors[f'{tag}.{name}.logits']), (tag, name)
            kwargs = dict(batch_size=5, ablate=case, display_progress_as=None)
            assert torch.equal(classifier.predict(dataset, **kwargs),
                               tensors[f'{tag}.{name}.predictions'])
            want = meta['results'][f'{tag}.{name}']
            assert classifier.accuracy(dataset, **kwargs) == want['accuracy']
            got = classifier.accuracies(dataset, **kwargs)
            assert {str(k): v for k, v in got.items()} == want['accuracies']
        # nothing stays behind
        with torch.no_grad():
            assert torch.equal(model(images), tensors[f'{tag}.none.logits'])


@pytest.mark.parametrize('config', ['resnet18', 'resnet50'])
def test_ablref_float32_is_in_the_fp32_class(gold, config):
    tensors, meta = gold
    sd = ablref.state_dict(config, tensors, meta)
    for h, w in geometries(meta):
        for name, case in cases_of(meta, config).items():
            want = tensors[f'{config}.{h}x{w}.{name}.logits']
            got = ablref.forward(tensors[f'images.{h}x{w}'], sd,
                                 synthetic.RESNET_BLOCKS[config], case)
            assert got.dtype == torch.float32
            err = float((got - want).abs().max())
            assert err <= FEATURE_CLASS * float(want.abs().max()), (config, h, w, name, err)


def test_error_types(gold):
    tensors, meta = gold
    model = native_model('resnet18', tensors, meta)
    images = tensors['images.7x9']
    with pytest.raises(ValueError, match='expected 4D features'):
        ablations.zero([0])(torch.zeros(2, 3))
    for m in (model, Foreign(model)):
        with pytest.raises(ValueError, match='not found in model'):
            with ablations.ablated(m, [('layer9', 0)]):
                pass
        with pytest.raises(IndexError):
            with ablations.ablated(m, [('layer1', meta['width'])]) as edited:
                with torch.no_grad():
                    edited(images)
    with pytest.raises(ValueError, match='conv1'):
        with ablations.ablated(model, [('fc', 0)]):   # a module, but not one of the five
            pass
    with pytest.raises(ValueError, match='zero'):
        with ablations.ablated(model, [('layer1', 0)], rule=lambda units: (lambda x: x)):
            pass
    dataset = data.TensorDataset(images, tensors['resnet18.7x9.targets'])
    with pytest.raises(KeyError, match='could not find layers'):
        ablations.ImageClassifier(model).fit(dataset, layers=['fc', 'nope'],
                                             display_progress_as=None)
    with pytest.raises(ValueError, match='not supported'):
        classifiers.ResNetClassifier('alexnet')


def test_fit_trains_only_the_named_layers_and_cleans_up(gold):
    tensors, meta = gold
    torch.manual_seed(0)
    model = native_model('resnet18', tensors, meta)
    classifier = ablations.ImageClassifier(model)
    images = tensors['images.33x47']
    dataset = data.TensorDataset(images, tensors['resnet18.33x47.targets'])
    before = copy.deepcopy(model.state_dict())
    case = [('layer2', 1), ('conv1', 3)]
    classifier.fit(dataset, batch_size=4, max_epochs=2, hold_out=[0, 5, 9], layers=['fc'],
                   ablate=case, optimizer_kwargs=dict(lr=1e-2), display_progress_as=None)
    after = model.state_dict()
    changed = {k for k in before if not torch.equal(before[k], after[k])}
    assert changed, 'fit changed nothing'
    for key in changed:
        assert key.startswith('fc.') or key.rsplit('.', 1)[-1] in (
            'running_mean', 'running_var', 'num_batches_tracked'), key
    assert {'fc.weight', 'fc.bias'} <= changed
    # hooks and the ablation set are gone: the model equals a fresh one with its weights
    assert model._ablation == () and model._ablation_native
    assert all(not m._forward_hooks for m in model.modules())
    fresh = classifiers.ResNetClassifier('resnet18', num_classes=10, width=meta['width'])
    fresh.load_state_dict(after)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(images), fresh.eval()(images))


def test_fit_restores_the_best_state_on_early_stop(gold):
    tensors, meta = gold
    torch.manual_seed(0)
    model = native_model('resnet18', tensors, meta)
    classifier = ablations.ImageClassifier(model)
    images = tensors['images.7x9']
    dataset = data.TensorDataset(images, tensors['resnet18.7x9.targets'])
    hold = [0, 1, 2, 3]
    seen = []

    class Recording(torch.optim.SGD):
        """Ascends: the held-out loss only gets worse, so the first epoch stays the best."""

        def step(self, closure=None):
            out = super().step(closure)
            seen.append(copy.deepcopy(model.fc.state_dict()))
            return out

    classifier.fit(dataset, batch_size=8, max_epochs=10, patience=1, hold_out=hold,
                   layers=['fc'], optimizer_t=Recording,
                   optimizer_kwargs=dict(lr=0.5, maximize=True), display_progress_as=None)
    # one step per epoch (8 training images); patience 1 stops after the third epoch
    assert len(seen) == 3
    assert torch.equal(model.fc.weight, seen[0]['weight'])
    assert not torch.equal(seen[2]['weight'], seen[0]['weight'])


def test_unit_scores_on_a_foreign_model_is_the_loop(gold):
    tensors, meta = gold
    model = Foreign(native_model('resnet18', tensors, meta)).eval()
    classifier = ablations.ImageClassifier(model)
    dataset = data.TensorDataset(tensors['images.7x9'], tensors['resnet18.7x9.targets'])
    units = [('conv1', 0), ('layer1', 7), ('layer3', 30), ('layer4', 63), ('layer4', 2)]
    base = [('layer2', 4)]
    got = classifier.unit_scores(dataset, units, batch_size=5, ablate=base,
                                 display_progress_as=None)
    want = [classifier.accuracy(dataset, batch_size=5, ablate=[*base, u],
                                display_progress_as=None) for u in units]
    assert got == want and len(set(got)) > 1


def test_new_entry_points_are_declared_bound_and_probed():
    header = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'milan_hip.h').read_text(),
                    flags=re.S)
    lib = hip.load_library()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in hip.SIGNATURES and name in hip.PROBED
        assert hasattr(lib, name)
    assert hip.ABI_VERSION == 11 == lib.milan_abi_version()
    assert hip.ERR_INDEX == -6 and 'MILAN_ERR_INDEX = -6' in header
    # a null context is rejected before anything touches a device
    assert lib.milan_set_ablation(None, None, None, 0, None) == hip.ERR_ARG
    assert lib.milan_classify(None, None, 1, 8, 8, None, None, None, 0, None) == hip.ERR_ARG
    assert lib.milan_classify_sweep(None, None, 1, 8, 8, None, None, 0, None, None, None, None,
                                    0, None) == hip.ERR_ARG
    assert lib.milan_classify_workspace_bytes(None, 1, 8, 8, 0) == 0
    with pytest.raises(IndexError):
        lib.milan_last_error()  # (any call first: the message buffer is thread-local)
        hip._check(hip.ERR_INDEX)


def test_the_package_exports_both_modules():
    import milan_amd
    assert milan_amd.ablations is ablations and milan_amd.classifiers is classifiers
    assert milan_amd.ImageClassifier is ablations.ImageClassifier
    assert milan_amd.ResNetClassifier is classifiers.ResNetClassifier
    assert classifiers.ResNetClassifier.layers == ablref.LAYERS
