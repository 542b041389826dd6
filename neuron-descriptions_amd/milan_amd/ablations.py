"""Altering unit activations on the fly: the reference's `src/utils/ablations.py`.

Same surface -- `zero`, `ablated`, `ImageClassifier` with `forward` / `fit` / `predict` /
`accuracy` / `accuracies`, arguments, defaults and return types as in ablations.py:20-367
-- plus `ImageClassifier.unit_scores`, the one-unit-at-a-time loop of the editing
experiment (`experiments/edit.py:295-301`) as one call.

Two kinds of model:
  - a `classifiers.ResNetClassifier` or `classifiers.AlexNetClassifier` (a
    `classifiers.NativeClassifier`): in eval mode under `no_grad` on the GPU the ablation
    set is installed in libmilan_hip (`hip.Context.set_ablation`) and the forward runs there;
    in training mode the same set acts through forward hooks on the torch path;
  - any other `nn.Module`: the named modules' outputs are edited through forward hooks, what
    the reference does with nethook's `InstrumentedModel.edit_layer`.

Both CNNs of `experiments/edit.py --cnn` are built; `zero` refuses 2-D features, so
AlexNet's `fc6` / `fc7` are trained (`fit(layers=...)`) but never edited.  Not built: the
Places365 AlexNet of `src/deps/alexnet.py` (grouped convs, an unpadded conv1, `fc8`), a
different network.  One deliberate difference: `fit` keeps a COPY of the best state (the
reference keeps `self.state_dict()`, whose tensors alias the live parameters, so its
restore on early stopping restores nothing).
"""
import collections
import contextlib
import copy
from typing import (Any, Callable, Dict, Iterator, List, Mapping, Optional,
                    Sequence, Sized, Tuple, Type, Union, cast)

import torch
from torch import nn, optim
from torch.utils import data

from milan_amd import classifiers, training

Layer = Union[int, str]
Unit = Tuple[Layer, int]
Device = Union[str, torch.device]
Rule = Callable[[torch.Tensor], torch.Tensor]
RuleFactory = Callable[[Sequence[int]], Rule]


def _progress(iterable, desc: Optional[str]):
    if desc is None:
        return iterable
    try:
        from tqdm.auto import tqdm
    except ImportError:
        return iterable
    return tqdm(iterable, desc=desc)


def zero(units: Sequence[int]) -> Rule:
    """Zero the given units (ablations.py:20-42): features * mask, mask[:, units] = 0."""

    def fn(features: torch.Tensor) -> torch.Tensor:
        if features.dim() != 4:
            raise ValueError(f'expected 4D features, got {features.dim()}')
        # a mask, not an in-place edit: autograd stays intact
        shape = (*features.shape[:2], 1, 1)
        mask = features.new_ones(*shape)
        mask[:, units] = 0
        return features * mask

    return fn


class _Retain:
    """The forward hooks of one `ablated` block (nethook's edit_layer, outputs only)."""

    def __init__(self, model: nn.Module, edits: Mapping[str, Rule]):
        modules = dict(model.named_modules())
        for layer in edits:
            if layer not in modules:
                raise ValueError(f'Layer {layer} not found in model')
        self.handles = [
            modules[layer].register_forward_hook(self._hook(rule))
            for layer, rule in edits.items()
        ]

    @staticmethod
    def _hook(rule: Rule):
        return lambda module, inputs, output: rule(output)

    def close(self) -> None:
        for handle in self.handles:
            handle.remove()
        self.handles = []


@contextlib.contextmanager
def ablated(model: nn.Module,
            units: Sequence[Unit],
            rule: RuleFactory = zero) -> Iterator[nn.Module]:
    """Ablate the given (layer, unit) pairs according to `rule` (ablations.py:45-70).

    Yields the model itself, configured to ablate the units until the block exits.
    """
    edits: Dict[str, List[int]] = collections.defaultdict(list)
    for layer, unit in units:
        edits[str(layer)].append(unit)
    native = isinstance(model, classifiers.NativeClassifier)
    if native:
        for layer in edits:
            if layer not in model.layers:
                raise ValueError(f'Layer {layer} not found in model: a '
                                 f'{type(model).__name__} is edited at {model.layers}')
        if rule is not zero and not model.training:
            raise ValueError('only the `zero` rule has a kernel: a custom rule cannot '
                             f'edit a {type(model).__name__} in eval mode')
    retain = _Retain(model, {layer: rule(sorted(uns)) for layer, uns in edits.items()})
    if native:
        saved = (model._ablation, model._ablation_native)
        model._ablation = tuple((layer, int(u)) for layer, uns in edits.items() for u in uns)
        model._ablation_native = rule is zero
    try:
        yield model
    finally:
        retain.close()
        if native:
            model._ablation, model._ablation_native = saved


class ImageClassifier(nn.Module):
    """Wraps an image classifier and adds some ablation utilities."""

    def __init__(self, model: nn.Module):
        super().__init__()
        self.model = model

    def forward(self, *args: Any, **kwargs: Any) -> Any:
        """Call `self.model.forward`."""
        return self.model(*args, **kwargs)

    def fit(self,
            dataset: data.Dataset,
            image_index: int = 0,
            target_index: int = 1,
            batch_size: int = 128,
            max_epochs: int = 100,
            patience: int = 4,
            hold_out: Union[float, Sequence[int]] = .1,
            optimizer_t: Type[optim.Optimizer] = optim.AdamW,
            optimizer_kwargs: Optional[Mapping[str, Any]] = None,
            num_workers: int = 0,
            ablate: Optional[Sequence[Unit]] = None,
            layers: Optional[Sequence[Layer]] = None,
            device: Optional[Device] = None,
            display_progress_as: Optional[str] = 'train classifer') -> None:
        """Train the classifier on the dataset (ablations.py:90-216), optionally under an
        ablation and restricted to the parameters of `layers`; early stopping on the
        held-out loss restores the best state."""
        if device is not None:
            self.to(device)
        if optimizer_kwargs is None:
            optimizer_kwargs = {}

        if isinstance(hold_out, float):
            train, val = training.random_split(dataset, hold_out=hold_out)
        else:
            train, val = training.fixed_split(dataset, hold_out)

        train_loader = data.DataLoader(train,
                                       batch_size=batch_size,
                                       num_workers=num_workers,
                                       shuffle=True)
        val_loader = data.DataLoader(val,
                                     batch_size=batch_size,
                                     num_workers=num_workers)

        if layers is None:
            parameters = list(self.parameters())
        else:
            missing = {str(layer) for layer in layers}
            parameters = []
            for name, submodule in self.model.named_modules():
                if name in missing:
                    parameters += list(submodule.parameters())
                    missing -= {name}
            if missing:
                raise KeyError(f'could not find layers: {sorted(missing)}')

        optimizer = optimizer_t(parameters, **optimizer_kwargs)
        criterion = nn.CrossEntropyLoss()
        stopper = training.EarlyStopping(patience=patience)

        progress = _progress(range(max_epochs), display_progress_as)

        with ablated(self.model, ablate or []) as model:
            best = copy.deepcopy(self.state_dict())
            for _ in progress:
                model.train()
                train_loss = 0.
                for batch in train_loader:
                    images = batch[image_index].to(device)
                    targets = batch[target_index].to(device)
                    predictions = model(images)
                    loss = criterion(predictions, targets)
                    loss.backward()
                    optimizer.step()
                    optimizer.zero_grad()
                    train_loss += loss.item()
                train_loss /= len(train_loader)

                model.eval()
                val_loss = 0.
                for batch in val_loader:
                    images = batch[image_index].to(device)
                    targets = batch[target_index].to(device)
                    with torch.no_grad():
                        predictions = model(images)
                        loss = criterion(predictions, targets)
                    val_loss += loss.item()
                val_loss /= len(val_loader)

                if hasattr(progress, 'set_description'):
                    progress.set_description(f'{display_progress_as} '
                                             f'[train_loss={train_loss:.3f}, '
                                             f'val_loss={val_loss:.3f}]')

                if stopper(val_loss):
                    self.load_state_dict(best)
                    break

                if stopper.improved:
                    best = copy.deepcopy(self.state_dict())

    def predict(
        self,
        dataset: data.Dataset,
        image_index: int = 0,
        batch_size: int = 128,
        num_workers: int = 0,
        ablate: Optional[Sequence[Unit]] = None,
        device: Optional[Device] = None,
        display_progress_as: Optional[str] = 'classify images',
    ) -> torch.Tensor:
        """Class predictions, shape (len(dataset),), for every element of the dataset
        (ablations.py:218-269), optionally under an ablation."""
        if device is not None:
            self.to(device)
        loader = _progress(
            data.DataLoader(dataset, num_workers=num_workers, batch_size=batch_size),
            display_progress_as)
        predictions = []
        with ablated(self.model, ablate or []) as model:
            for batch in loader:
                images = batch[image_index].to(device)
                with torch.no_grad():
                    predictions.append(model(images).argmax(dim=-1))
        return torch.cat(predictions)

    def _targets(self, dataset: data.Dataset, target_index: int,
                 device: Optional[Device]) -> torch.Tensor:
        size = len(cast(Sized, dataset))
        return torch.tensor([dataset[index][target_index] for index in range(size)],
                            dtype=torch.long,
                            device=device)

    def accuracy(
        self,
        dataset: data.Dataset,
        predictions: Optional[torch.Tensor] = None,
        target_index: int = 1,
        device: Optional[Device] = None,
        display_progress_as: Optional[str] = 'test classifer',
        **kwargs: Any,
    ) -> float:
        """Accuracy on the dataset (ablations.py:271-312); **kwargs go to `predict`."""
        if predictions is None:
            predictions = self.predict(dataset,
                                       device=device,
                                       display_progress_as=display_progress_as,
                                       **kwargs)
        size = len(cast(Sized, dataset))
        targets = self._targets(dataset, target_index, device)
        correct = predictions.eq(targets).sum().item()
        return correct / size

    def accuracies(
        self,
        dataset: data.Dataset,
        predictions: Optional[torch.Tensor] = None,
        target_index: int = 1,
        device: Optional[Device] = None,
        display_progress_as: Optional[str] = 'test classifer (class-wise)',
        **kwargs: Any,
    ) -> Mapping[int, float]:
        """Class-by-class accuracy (ablations.py:314-367); **kwargs go to `predict`."""
        if predictions is None:
            predictions = self.predict(dataset,
                                       device=device,
                                       display_progress_as=display_progress_as,
                                       **kwargs)
        targets = self._targets(dataset, target_index, device)
        correct: Dict[int, int] = collections.defaultdict(int)
        total: Dict[int, int] = collections.defaultdict(int)
        for prediction, target in zip(predictions.tolist(), targets.tolist()):
            correct[target] += prediction == target
            total[target] += 1
        assert correct.keys() == total.keys()
        return {target: correct[target] / total[target] for target in correct.keys()}

    def unit_scores(
        self,
        dataset: data.Dataset,
        units: Sequence[Unit],
        image_index: int = 0,
        target_index: int = 1,
        batch_size: int = 128,
        num_workers: int = 0,
        ablate: Optional[Sequence[Unit]] = None,
        device: Optional[Device] = None,
        display_progress_as: Optional[str] = 'score units',
    ) -> List[float]:
        """The accuracy with each unit ablated on its own, on top of `ablate`:

            [self.accuracy(dataset, ablate=[*(ablate or []), u]) for u in units]

        the loop of `experiments/edit.py:295-301`.  On a `NativeClassifier` on the GPU every
        batch goes through `hip.Context.classify_sweep`: all units of one layer share the
        forward pass up to that layer, and the numbers are those of the loop, bit for bit.
        Any other model runs the loop itself.
        """
        units = list(units)
        if device is not None:
            self.to(device)
        model = self.model
        native = (isinstance(model, classifiers.NativeClassifier) and
                  next(model.parameters()).device.type == 'cuda')
        if not native:
            return [
                self.accuracy(dataset,
                              target_index=target_index,
                              device=device,
                              display_progress_as=None,
                              image_index=image_index,
                              batch_size=batch_size,
                              num_workers=num_workers,
                              ablate=[*(ablate or []), unit]) for unit in _progress(
                                  units, display_progress_as)
            ]
        for layer, _ in units:
            if str(layer) not in model.layers:
                raise ValueError(f'Layer {layer} not found in model: a '
                                 f'{type(model).__name__} is edited at {model.layers}')
        size = len(cast(Sized, dataset))
        loader = _progress(
            data.DataLoader(dataset, num_workers=num_workers, batch_size=batch_size),
            display_progress_as)
        correct = torch.zeros(len(units), dtype=torch.int64)
        was_training = model.training
        model.eval()
        try:
            with ablated(model, ablate or []), torch.no_grad():
                for batch in loader:
                    images = batch[image_index].to(device)
                    targets = batch[target_index].to(device)
                    if not units:
                        continue
                    _, counts = model.classify_sweep(
                        images, [(str(layer), unit) for layer, unit in units], targets)
                    correct += counts.cpu().to(torch.int64)
        finally:
            model.train(was_training)
        return [count / size for count in correct.tolist()]
