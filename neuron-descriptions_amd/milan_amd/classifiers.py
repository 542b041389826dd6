"""Image classifiers whose eval-mode forward runs on the HIP trunk.

`ResNetClassifier` and `AlexNetClassifier` are the two CNNs `experiments/edit.py --cnn`
offers.  `AlexNetClassifier` has the module tree of the reference's `alexnet_seq`
(`src/deps/ext/torchvision/models.py`: `conv1 .. conv5`, `fc6`, `fc7`, `linear8`), so a
checkpoint that experiment saved loads with `load_state_dict` and
`ImageClassifier.fit(layers=['fc6', 'fc7', 'linear8'])` finds its layers; it is edited and
tapped at `conv1 .. conv5`.

`PlacesAlexNetClassifier` and `OldResNet152` are the two Places365 networks of the reference's
model zoo (`src/deps/alexnet.py`, `src/deps/resnet152.py`): the first is a network of its own
(grouped convs, an unpadded conv1, an optional LRN, `fc8`), the second the v1.5 bottleneck
ResNet-152 under Torch7-converted key and layer names.

`VGGClassifier` is torchvision's VGG-11 / 13 / 16 / 19 without batch norm, the VGGs of the
reference's audit experiment (`experiments/audit.py`) and, after `rekey_vgg16_places`, its
`vgg16/places365`; it is edited and tapped at the last conv of each block (`LAYERS.VGG11` ..
`VGG19`).

`ResNetClassifier` is the CNN the reference's experiments dissect and edit
(`experiments/analyze.py`, `experiments/edit.py`: a torchvision ResNet handed to
`src/utils/ablations.ImageClassifier`).  It is an `nn.Module` with torchvision's module
tree and key names (`conv1.weight`, `bn1.*`, `layerL.B.convK.weight`, `downsample.0/1`,
`fc.weight/bias`), so a torchvision checkpoint loads with `load_state_dict`,
`named_modules()` finds `fc`, `conv1` and `layer1..4`, and
`ImageClassifier.fit(layers=['fc'])` works.

`forward(images)`:
  - eval mode, under `no_grad`, GPU tensor: `hip.Context.classify` -- the whole forward in
    libmilan_hip, with the ablation set `ablations.ablated` installed;
  - otherwise (training mode, grad required, CPU tensors): the torch modules below, the
    same arithmetic the reference's torchvision model runs (batch-statistic BatchNorm in
    training mode).  That path is what `fit` trains through.
"""
from typing import Dict, Optional, Sequence, Tuple

import re

import torch
from torch import nn
from torch.nn import functional as F

from milan_amd import hip, synthetic

LAYERS = ('conv1', 'layer1', 'layer2', 'layer3', 'layer4')
ALEXNET_LAYERS = ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')


class _BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class NativeClassifier(nn.Module):
    """What the classifiers with a HIP forward share: the choice between the two forwards,
    the taps, the context cache and the ablation set `ablations.ablated` installs.  A
    subclass sets `layers`, calls `_init_native` last in its `__init__`, and provides
    `forward_eager` and `_make_context`."""

    layers: Tuple[str, ...] = ()

    def _init_native(self) -> None:
        self._ctx: Optional[hip.Context] = None
        self._ctx_key = None
        # the set `ablations.ablated` installed: (layer, unit) pairs for the native path
        # (the eager path sees the same set through forward hooks), and whether its rule
        # is one the library has a kernel for
        self._ablation: Sequence[Tuple[str, int]] = ()
        self._ablation_native = True
        self._ctx_ablation = None

    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _make_context(self, device: torch.device) -> hip.Context:
        raise NotImplementedError

    def runs_natively(self, images: torch.Tensor) -> bool:
        return (not self.training and not torch.is_grad_enabled() and
                images.device.type == 'cuda')

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        if not self.runs_natively(images):
            return self.forward_eager(images)
        return self._native_context().classify(images)

    def activations(self, images: torch.Tensor, layers) -> Dict[str, torch.Tensor]:
        """The outputs of the named modules for `images`, under the current ablation set and
        after its edit (what the next layer reads; what `nethook.retain_layers` retains).

        `layers`: a name or a sequence of names from `named_modules()`.  When the forward
        would run natively (`runs_natively`) and every name is one of `self.layers`, the
        tensors come from `hip.Context.activations`: one walk of the HIP trunk up to the
        deepest layer asked for.  Anything else -- CPU tensors, training mode, grad enabled,
        a layer such as 'layer2.0.conv1' or 'fc' -- runs `forward_eager` under `no_grad`
        with forward hooks.  An unknown name is a KeyError."""
        names = [layers] if isinstance(layers, str) else list(layers)
        modules = dict(self.named_modules())
        for name in names:
            if not name or name not in modules:
                raise KeyError(f'layer not found: {name}')
        if self.runs_natively(images) and all(name in self.layers for name in names):
            return self._native_context().activations(images, names)
        retained: Dict[str, torch.Tensor] = {}
        handles = []

        def retain(name):
            def hook(module, inputs, output):
                # (nethook's retain: detached, not copied -- an in-place ReLU that follows
                # the module shows in it, as it does there)
                retained[name] = output.detach()
            return hook

        # (registered now: after the hooks of an `ablations.ablated` block around this call,
        # so they see the edited output)
        for name in dict.fromkeys(names):
            handles.append(modules[name].register_forward_hook(retain(name)))
        try:
            with torch.no_grad():
                self.forward_eager(images)
        finally:
            for handle in handles:
                handle.remove()
        return {name: retained[name] for name in names}

    # -- HIP context, rebuilt when device or weights change ---------------------------
    def _context(self) -> hip.Context:
        device = hip.require_device(next(self.parameters()).device)
        tensors = list(self.parameters()) + list(self.buffers())
        key = (device, tuple(t._version for t in tensors),
               tuple(t.data_ptr() for t in tensors))
        if self._ctx is None or self._ctx_key != key:
            self._ctx = self._make_context(device)
            if self.precision == 'auto':
                self._ctx.set_precision('split_f16')
                self._ctx.on_saturation = 'f32'
            else:
                self._ctx.set_precision(self.precision)
            self._ctx_key = key
            self._ctx_ablation = None
        return self._ctx

    def _native_context(self) -> hip.Context:
        """The context with this module's current ablation set installed."""
        if not self._ablation_native:
            raise ValueError('only the `zero` rule has a kernel: a custom ablation rule '
                             'runs in training mode / with grad enabled (the torch path), '
                             'not in the native eval-mode forward')
        ctx = self._context()
        wanted = tuple(sorted(set(self._ablation)))
        if self._ctx_ablation != wanted:
            ctx.set_ablation(wanted)
            self._ctx_ablation = wanted
        return ctx

    def classify_sweep(self, images: torch.Tensor, units, targets=None):
        """`hip.Context.classify_sweep` under this module's current ablation set."""
        return self._native_context().classify_sweep(images, list(units), targets)


class ResNetClassifier(NativeClassifier):
    """torchvision-shaped ResNet (v1.5 blocks) with a native eval-mode forward.

    `config`: 'resnet18' / 'resnet34' (basic blocks) or 'resnet50' / 'resnet101' /
    'resnet152' (bottlenecks); `width` 64 is torchvision's.  `precision`: 'auto' (split-f16
    with an exact-fp32 rerun of a call that saturated), 'split_f16' or 'f32'.  Weights start
    as `nn.Conv2d` / `nn.Linear` leave them; load a checkpoint with `load_state_dict`.
    """

    layers: Tuple[str, ...] = LAYERS

    def __init__(self,
                 config: str = 'resnet18',
                 num_classes: int = 1000,
                 width: int = 64,
                 precision: str = 'auto'):
        super().__init__()
        if config not in synthetic.RESNET_BLOCKS:
            raise ValueError(f'classifier not supported: {config} (AlexNet is '
                             '`AlexNetClassifier`)')
        if precision not in ('auto', 'split_f16', 'f32'):
            raise ValueError(f'unknown precision: {precision}')
        self.config = config
        self.blocks = synthetic.RESNET_BLOCKS[config]
        self.width = int(width)
        self.num_classes = int(num_classes)
        self.precision = precision
        block = _BasicBlock if config in synthetic.BASIC_BLOCK_CONFIGS else _Bottleneck
        self.conv1 = nn.Conv2d(3, width, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = width
        for li, count in enumerate(self.blocks):
            planes = width * 2**li
            stage = []
            for bi in range(count):
                stride = 2 if (bi == 0 and li > 0) else 1
                downsample = None
                if stride != 1 or inplanes != planes * block.expansion:
                    downsample = nn.Sequential(
                        nn.Conv2d(inplanes, planes * block.expansion, 1, stride,
                                  bias=False),
                        nn.BatchNorm2d(planes * block.expansion))
                stage.append(block(inplanes, planes, stride, downsample))
                inplanes = planes * block.expansion
            setattr(self, f'layer{li + 1}', nn.Sequential(*stage))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(inplanes, num_classes)
        self._init_native()

    # -- the two forwards -----------------------------------------------------------
    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        """torchvision's `ResNet._forward_impl` on this module's own parameters."""
        x = self.maxpool(self.relu(self.bn1(self.conv1(images))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))

    def _make_context(self, device: torch.device) -> hip.Context:
        sd = {'encoder.encoder.model.' + k: v for k, v in self.state_dict().items()}
        dims = hip.make_dims(sd, 1, blocks=self.blocks)
        return hip.Context(dims, sd, device)


class AlexNetClassifier(NativeClassifier):
    """The reference's `alexnet_seq` (torchvision's AlexNet as one `nn.Sequential`-shaped
    tree) with a native eval-mode forward.

    Named children, in order: conv1, relu1, pool1, conv2, relu2, pool2, conv3, relu3, conv4,
    relu4, conv5, relu5, pool5, avgpool, flatten, dropout6, fc6, relu6, dropout7, fc7, relu7,
    linear8.  Channels are `width` x (1, 3, 6, 4, 4); `width` 64 and `hidden` 4096 are
    torchvision's.  `precision` as for `ResNetClassifier`.  Edited and tapped at
    `layers` = conv1 .. conv5: a conv's output is followed by an in-place ReLU, so what the
    next layer reads, and what a retain hook sees, is relu(conv + bias) x mask.  Images of at
    least 63 x 63.
    """

    layers: Tuple[str, ...] = ALEXNET_LAYERS

    def __init__(self,
                 num_classes: int = 1000,
                 width: int = 64,
                 hidden: int = 4096,
                 precision: str = 'auto'):
        super().__init__()
        if precision not in ('auto', 'split_f16', 'f32'):
            raise ValueError(f'unknown precision: {precision}')
        self.width = int(width)
        self.hidden = int(hidden)
        self.num_classes = int(num_classes)
        self.precision = precision
        ch = [c * self.width for c in synthetic.ALEXNET_CHANNELS]
        self.conv1 = nn.Conv2d(3, ch[0], 11, 4, 2)
        self.relu1 = nn.ReLU(inplace=True)
        self.pool1 = nn.MaxPool2d(3, 2)
        self.conv2 = nn.Conv2d(ch[0], ch[1], 5, 1, 2)
        self.relu2 = nn.ReLU(inplace=True)
        self.pool2 = nn.MaxPool2d(3, 2)
        self.conv3 = nn.Conv2d(ch[1], ch[2], 3, 1, 1)
        self.relu3 = nn.ReLU(inplace=True)
        self.conv4 = nn.Conv2d(ch[2], ch[3], 3, 1, 1)
        self.relu4 = nn.ReLU(inplace=True)
        self.conv5 = nn.Conv2d(ch[3], ch[4], 3, 1, 1)
        self.relu5 = nn.ReLU(inplace=True)
        self.pool5 = nn.MaxPool2d(3, 2)
        self.avgpool = nn.AdaptiveAvgPool2d((6, 6))
        self.flatten = nn.Flatten()
        self.dropout6 = nn.Dropout()
        self.fc6 = nn.Linear(ch[4] * 36, self.hidden)
        self.relu6 = nn.ReLU(inplace=True)
        self.dropout7 = nn.Dropout()
        self.fc7 = nn.Linear(self.hidden, self.hidden)
        self.relu7 = nn.ReLU(inplace=True)
        self.linear8 = nn.Linear(self.hidden, self.num_classes)
        self._init_native()

    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        """`alexnet_seq`'s forward: the named children in order."""
        x = images
        for module in self.children():
            x = module(x)
        return x

    def _make_context(self, device: torch.device) -> hip.Context:
        sd = {}
        for conv, index in zip(self.layers, (0, 3, 6, 8, 10)):
            module = getattr(self, conv)
            sd[f'encoder.encoder.model.features.{index}.weight'] = module.weight
            sd[f'encoder.encoder.model.features.{index}.bias'] = module.bias
        head = [t for fc in (self.fc6, self.fc7, self.linear8) for t in (fc.weight, fc.bias)]
        return hip.Context(hip.make_dims(sd, 1), sd, device, alexnet_head=head)


class LRN(nn.Module):
    """Across-channel local response normalisation as the Places365 AlexNet defines it:
    y = x / (1 + alpha * mean)^beta, `mean` the average of x^2 over the `local_size`
    neighbouring channels with zeros beyond both ends (the divisor is always `local_size`).
    The torch module takes any odd size; the native kernel behind `PlacesAlexNetClassifier`
    (`hip.Context.set_alexnet_lrn`) takes odd sizes up to 17."""

    def __init__(self, local_size: int = 5, alpha: float = 1e-4, beta: float = 0.75):
        super().__init__()
        if local_size < 1 or local_size % 2 == 0:
            raise ValueError(f'local_size must be odd, got {local_size}')
        self.local_size, self.alpha, self.beta = int(local_size), float(alpha), float(beta)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        half = self.local_size // 2
        squares = F.pad(x * x, (0, 0, 0, 0, half, half))
        total = sum(squares[:, j:j + x.shape[1]] for j in range(self.local_size))
        return x / (total / self.local_size * self.alpha + 1.0)**self.beta

    def extra_repr(self) -> str:
        return f'local_size={self.local_size}, alpha={self.alpha}, beta={self.beta}'


class PlacesAlexNetClassifier(NativeClassifier):
    """The Places365 AlexNet of the reference (`src/deps/alexnet.py`) with a native eval-mode
    forward.

    Named children, in order: conv1, relu1, pool1, [lrn1,] conv2, relu2, pool2, [lrn2,]
    conv3, relu3, conv4, relu4, conv5, relu5, pool5, flatten, fc6, relu6, [dropout6,] fc7,
    relu7, [dropout7,] fc8 -- the reference's, so its `state_dict` loads with
    `load_state_dict`.  Channels are `width` / 32 x (96, 256, 384, 384, 256), `width` a
    multiple of 8 (the reference: 32); conv2, conv4 and conv5 have two groups unless
    `split_groups` is off.  conv1 has no padding and there is no adaptive pool: the forward
    needs images that leave 6 x 6 after pool5 (227 x 227); `activations` takes any image of
    35 x 35 or more.  Edited and tapped at `layers` = conv1 .. conv5 with
    `AlexNetClassifier`'s semantics: relu(conv + bias) x mask, before the pool and the LRN.
    `precision` as for `ResNetClassifier`.
    """

    layers: Tuple[str, ...] = ALEXNET_LAYERS

    def __init__(self,
                 num_classes: int = 365,
                 width: int = 32,
                 hidden: int = 4096,
                 include_lrn: bool = False,
                 split_groups: bool = True,
                 include_dropout: bool = False,
                 precision: str = 'auto'):
        super().__init__()
        if precision not in ('auto', 'split_f16', 'f32'):
            raise ValueError(f'unknown precision: {precision}')
        if width < 8 or width % 8:
            raise ValueError(f'width must be a multiple of 8, got {width}')
        self.width = int(width)
        self.hidden = int(hidden)
        self.num_classes = int(num_classes)
        self.include_lrn = bool(include_lrn)
        self.precision = precision
        ch = [c * self.width for c in synthetic.PLACES_ALEXNET_CHANNELS]
        groups = synthetic.PLACES_ALEXNET_GROUPS if split_groups else (1, 1, 1, 1, 1)
        self.conv1 = nn.Conv2d(3, ch[0], 11, 4, groups=groups[0])
        self.relu1 = nn.ReLU(inplace=True)
        self.pool1 = nn.MaxPool2d(3, 2)
        if include_lrn:
            self.lrn1 = LRN(5, 1e-4, 0.75)
        self.conv2 = nn.Conv2d(ch[0], ch[1], 5, padding=2, groups=groups[1])
        self.relu2 = nn.ReLU(inplace=True)
        self.pool2 = nn.MaxPool2d(3, 2)
        if include_lrn:
            self.lrn2 = LRN(5, 1e-4, 0.75)
        self.conv3 = nn.Conv2d(ch[1], ch[2], 3, padding=1, groups=groups[2])
        self.relu3 = nn.ReLU(inplace=True)
        self.conv4 = nn.Conv2d(ch[2], ch[3], 3, padding=1, groups=groups[3])
        self.relu4 = nn.ReLU(inplace=True)
        self.conv5 = nn.Conv2d(ch[3], ch[4], 3, padding=1, groups=groups[4])
        self.relu5 = nn.ReLU(inplace=True)
        self.pool5 = nn.MaxPool2d(3, 2)
        self.flatten = nn.Flatten()
        self.fc6 = nn.Linear(ch[4] * 36, self.hidden)
        self.relu6 = nn.ReLU(inplace=True)
        if include_dropout:
            self.dropout6 = nn.Dropout()
        self.fc7 = nn.Linear(self.hidden, self.hidden)
        self.relu7 = nn.ReLU(inplace=True)
        if include_dropout:
            self.dropout7 = nn.Dropout()
        self.fc8 = nn.Linear(self.hidden, self.num_classes)
        self._init_native()

    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        """The reference's `nn.Sequential` forward: the named children in order."""
        x = images
        for module in self.children():
            x = module(x)
        return x

    def _make_context(self, device: torch.device) -> hip.Context:
        sd = {}
        for conv in self.layers:
            module = getattr(self, conv)
            sd[f'encoder.encoder.model.{conv}.weight'] = module.weight
            sd[f'encoder.encoder.model.{conv}.bias'] = module.bias
        head = [t for fc in (self.fc6, self.fc7, self.fc8) for t in (fc.weight, fc.bias)]
        ctx = hip.Context(hip.make_dims(sd, 1), sd, device, alexnet_head=head)
        if self.include_lrn:
            ctx.set_alexnet_lrn(self.lrn1.local_size, self.lrn1.alpha, self.lrn1.beta)
        return ctx


# the reference's `OldResNet152` is an `nn.Sequential` converted from Torch7: children 0 / 1
# are conv1 / bn1, 4..7 the four stages, 10.1 the Linear layer; inside a block `0.0.N` is the
# residual branch (conv, bn, relu three times over) and `0.1.N` the downsample branch
_OLD_BRANCH = {'0': 'conv1', '1': 'bn1', '3': 'conv2', '4': 'bn2', '6': 'conv3', '7': 'bn3'}
_OLD_KEY = re.compile(r'^([4-7])\.(\d+)\.0\.([01])\.(\d+)\.(\w+)$')
OLD_RESNET152_LAYERS = {'0': 'conv1', '4': 'layer1', '5': 'layer2', '6': 'layer3',
                        '7': 'layer4'}


def rekey_old_resnet152(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A state dict of the reference's `OldResNet152` (`0.weight`, `4.0.0.0.0.weight`,
    `10.1.weight`, ...) under torchvision's key names (`conv1.weight`,
    `layer1.0.conv1.weight`, `fc.weight`, ...), in the same order.  Keys that already are
    torchvision's pass through; anything else is a KeyError."""
    out = {}
    for key, value in state_dict.items():
        head, _, tail = key.partition('.')
        match = _OLD_KEY.match(key)
        if head in ('0', '1') and tail and '.' not in tail:
            new = f"{'conv1' if head == '0' else 'bn1'}.{tail}"
        elif key.startswith('10.1.') and key.count('.') == 2:
            new = 'fc.' + key[5:]
        elif match:
            stage, block, branch, index, leaf = match.groups()
            if branch == '0':
                if index not in _OLD_BRANCH:
                    raise KeyError(f'not a key of OldResNet152: {key}')
                module = _OLD_BRANCH[index]
            else:
                if index not in ('0', '1'):
                    raise KeyError(f'not a key of OldResNet152: {key}')
                module = f'downsample.{index}'
            new = f'layer{int(stage) - 3}.{block}.{module}.{leaf}'
        elif head in ('conv1', 'bn1', 'fc') or head.startswith('layer'):
            new = key
        else:
            raise KeyError(f'not a key of OldResNet152: {key}')
        if new in out:
            raise KeyError(f'two keys map to {new}')
        out[new] = value
    return out


class OldResNet152(ResNetClassifier):
    """The Places365 ResNet-152 of the reference (`src/deps/resnet152.py`): arithmetically the
    v1.5 bottleneck ResNet-152, so it is a `ResNetClassifier('resnet152')` that also

      - loads a state dict in the reference class's Torch7-style keys (`rekey_old_resnet152`;
        `num_batches_tracked` may be there or not),
      - answers to the reference's layer names 0, 4, 5, 6, 7 (ints or strings) as aliases of
        conv1, layer1 .. layer4 in `activations`, so `exemplars.discriminative(model, dataset,
        layer=5)` runs natively and writes to `.../5/`,
      - pools with the reference's fixed `AvgPool2d(7)`: the forward takes images that leave
        7 x 7 after layer4 (224 x 224) and nothing else.
    """

    layer_aliases = OLD_RESNET152_LAYERS

    def __init__(self, num_classes: int = 365, width: int = 64, precision: str = 'auto'):
        super().__init__('resnet152', num_classes=num_classes, width=width, precision=precision)
        self.avgpool = nn.AvgPool2d(7, 1)
        self.layers = LAYERS + tuple(self.layer_aliases)

    def load_state_dict(self, state_dict, strict: bool = True):
        state_dict = rekey_old_resnet152(state_dict)
        own = self.state_dict()
        # (a checkpoint converted from Torch7 has no num_batches_tracked; a later one does)
        for key, value in own.items():
            if key.endswith('num_batches_tracked') and key not in state_dict:
                state_dict[key] = value
        return super().load_state_dict(state_dict, strict=strict)

    def _canonical(self, name) -> str:
        return self.layer_aliases.get(str(name), name)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        if self.runs_natively(images):
            h, w = images.shape[-2:]
            for _ in range(5):
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            if (h, w) != (7, 7):
                raise ValueError(f'OldResNet152 pools with a fixed AvgPool2d(7): images of '
                                 f'{tuple(images.shape[-2:])} leave {h} x {w} after layer4, '
                                 'not 7 x 7 (224 x 224 images do)')
        return super().forward(images)

    def activations(self, images: torch.Tensor, layers) -> Dict[str, torch.Tensor]:
        names = [layers] if isinstance(layers, (str, int)) else list(layers)
        for name in names:
            if not isinstance(name, (str, int)) or (isinstance(name, int) and
                                                    str(name) not in self.layer_aliases):
                raise KeyError(f'layer not found: {name}')
        got = super().activations(images, [self._canonical(name) for name in names])
        return {name: got[self._canonical(name)] for name in names}


class VGGClassifier(NativeClassifier):
    """torchvision's VGG-11 / 13 / 16 / 19 (the variants without batch norm) with a native
    eval-mode forward: a third of the reference's audit models (`experiments/audit.py`) and,
    as `vgg16` with 365 classes, its `vgg16/places365`.

    The module tree and the keys are torchvision's: `features`, an `nn.Sequential` of
    `Conv2d(3x3, padding 1)` / `ReLU(inplace=True)` per conv and one `MaxPool2d(2, 2)` per
    block; `avgpool = AdaptiveAvgPool2d((7, 7))`; `classifier = Sequential(Linear, ReLU,
    Dropout, Linear, ReLU, Dropout, Linear)`.  A torchvision checkpoint loads with
    `load_state_dict` (a Places365 one after `rekey_vgg16_places`).  Channels are `width` x
    (1, 2, 4, 8, 8), `width` a multiple of 8; 64 and `hidden` 4096 are torchvision's.
    `precision` as for `ResNetClassifier`.  Edited and tapped at `layers`, the reference's
    `LAYERS.VGG11` .. `VGG19`: the last conv of each block, e.g. features.2 / 7 / 14 / 21 / 28
    on vgg16.  A conv's output is followed by an in-place ReLU, so what the pool reads, and
    what a retain hook sees, is relu(conv + bias) x mask.  The forward takes images of at
    least 32 x 32; level l of `activations` images of at least 2^l each way.
    """

    def __init__(self,
                 config: str = 'vgg16',
                 num_classes: int = 1000,
                 width: int = 64,
                 hidden: int = 4096,
                 precision: str = 'auto'):
        super().__init__()
        if config not in synthetic.VGG_BLOCKS:
            raise ValueError(f'classifier not supported: {config} (the VGGs are '
                             f'{sorted(synthetic.VGG_BLOCKS)}, without batch norm)')
        if precision not in ('auto', 'split_f16', 'f32'):
            raise ValueError(f'unknown precision: {precision}')
        if width < 8 or width % 8:
            raise ValueError(f'width must be a multiple of 8, got {width}')
        self.config = config
        self.blocks = synthetic.VGG_BLOCKS[config]
        self.width = int(width)
        self.hidden = int(hidden)
        self.num_classes = int(num_classes)
        self.precision = precision
        modules, cin = [], 3
        for mult, count in zip(synthetic.VGG_CHANNELS, self.blocks):
            for _ in range(count):
                modules += [nn.Conv2d(cin, mult * self.width, 3, padding=1),
                            nn.ReLU(inplace=True)]
                cin = mult * self.width
            modules.append(nn.MaxPool2d(2, 2))
        self.features = nn.Sequential(*modules)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(
            nn.Linear(cin * 49, self.hidden), nn.ReLU(True), nn.Dropout(),
            nn.Linear(self.hidden, self.hidden), nn.ReLU(True), nn.Dropout(),
            nn.Linear(self.hidden, self.num_classes))
        self.layers = hip.vgg_level_names(self.blocks)
        self._init_native()

    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        """torchvision's `VGG.forward`: the modules in order."""
        x = self.avgpool(self.features(images))
        return self.classifier(torch.flatten(x, 1))

    def trunk_keys(self) -> Dict[str, str]:
        """`features.N` -> the library's `vgg.B.J` (block B = 1..5, conv J within it) for
        every conv of this config."""
        return {f'features.{index}': f'vgg.{b + 1}.{j}'
                for b, indices in enumerate(synthetic.vgg_feature_indices(self.config))
                for j, index in enumerate(indices)}

    def _make_context(self, device: torch.device) -> hip.Context:
        sd = {}
        for old, new in self.trunk_keys().items():
            module = self.features[int(old.split('.')[1])]
            sd[f'encoder.encoder.model.{new}.weight'] = module.weight
            sd[f'encoder.encoder.model.{new}.bias'] = module.bias
        head = [t for index in (0, 3, 6)
                for t in (self.classifier[index].weight, self.classifier[index].bias)]
        return hip.Context(hip.make_dims(sd, 1), sd, device, vgg_head=head)


def rekey_vgg16_places(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A state dict of the Places365 VGG-16 checkpoint (`features.conv1_1.weight` ..
    `features.conv5_3.bias`, `classifier.fc6` / `fc7` / `fc8a`, or `fc8`) under torchvision's
    key names (`features.0.weight` .. `features.28.bias`, `classifier.0` / `3` / `6`), in the
    same order.  Keys that already are torchvision's pass through; anything else is a
    KeyError."""
    table = {f'conv{b + 1}_{j + 1}': str(index)
             for b, indices in enumerate(synthetic.vgg_feature_indices('vgg16'))
             for j, index in enumerate(indices)}
    convs = set(table.values())
    linear = {'fc6': '0', 'fc7': '3', 'fc8': '6', 'fc8a': '6'}
    out = {}
    for key, value in state_dict.items():
        parts = key.split('.')
        if len(parts) != 3 or parts[2] not in ('weight', 'bias'):
            raise KeyError(f'not a key of the Places365 VGG-16: {key}')
        group, name, leaf = parts
        if group == 'features' and name in table:
            name = table[name]
        elif group == 'classifier' and name in linear:
            name = linear[name]
        elif not ((group == 'features' and name in convs) or
                  (group == 'classifier' and name in ('0', '3', '6'))):
            raise KeyError(f'not a key of the Places365 VGG-16: {key}')
        new = f'{group}.{name}.{leaf}'
        if new in out:
            raise KeyError(f'two keys map to {new}')
        out[new] = value
    return out
