"""Reference for the ablation tests: torchvision's `ResNet._forward_impl` in eval mode with
unit ablation, restated on a state dict in the conventions of `oracle.milan_oracle` (the same
trunk, `resnet_trunk`, with the edit points opened up), then mask, mean and fc.

It computes in the dtype of its inputs: float64 for the GPU tests' bound, float32 to tie the
restatement itself to the reference's goldens.  Tests only.

Edit points (src/exemplars/models.py:48-52, nethook.py:226-241: a module's OUTPUT is edited):
'conv1' is the raw stem conv output before bn1 / ReLU / maxpool, 'layerN' the post-ReLU
output of the stage's last block.
"""
import json
import pathlib

import torch
import torch.nn.functional as F

from milan_amd import synthetic
from oracle import milan_oracle as O

LAYERS = ('conv1', 'layer1', 'layer2', 'layer3', 'layer4')
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
WIDTH = 8


def masks_of(ablate, like):
    """layer -> (1, C, 1, 1) 0/1 mask builder for `like`-typed tensors."""
    units = {}
    for layer, unit in ablate:
        if layer not in LAYERS:
            raise ValueError(f'Layer {layer} not found in model')
        units.setdefault(layer, []).append(int(unit))

    def apply(layer, x):
        if layer not in units:
            return x
        mask = x.new_ones(1, x.shape[1], 1, 1)
        mask[:, units[layer]] = 0
        return x * mask

    return apply


def forward(images, sd, blocks, ablate=(), prefix=''):
    """(n,3,H,W) -> (n, classes) logits under the ablation set [(layer, unit), ...]."""
    sd = {k: v.to(images.dtype) if v.dtype.is_floating_point else v for k, v in sd.items()}
    edit = masks_of(ablate, images)
    x = F.conv2d(images, sd[prefix + 'conv1.weight'], None, stride=2, padding=3)
    x = edit('conv1', x)
    x = F.relu(O._bn(x, sd, prefix + 'bn1'))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for li, nblocks in enumerate(blocks):
        for bi in range(nblocks):
            p = f'{prefix}layer{li + 1}.{bi}.'
            stride = 2 if (bi == 0 and li > 0) else 1
            identity = x
            if (p + 'conv3.weight') in sd:
                out = F.relu(O._bn(F.conv2d(x, sd[p + 'conv1.weight']), sd, p + 'bn1'))
                out = F.relu(O._bn(F.conv2d(out, sd[p + 'conv2.weight'], stride=stride,
                                            padding=1), sd, p + 'bn2'))
                out = O._bn(F.conv2d(out, sd[p + 'conv3.weight']), sd, p + 'bn3')
            else:
                out = F.relu(O._bn(F.conv2d(x, sd[p + 'conv1.weight'], stride=stride,
                                            padding=1), sd, p + 'bn1'))
                out = O._bn(F.conv2d(out, sd[p + 'conv2.weight'], padding=1), sd, p + 'bn2')
            if (p + 'downsample.0.weight') in sd:
                identity = O._bn(F.conv2d(x, sd[p + 'downsample.0.weight'], stride=stride),
                                 sd, p + 'downsample.1')
            x = F.relu(out + identity)
        x = edit(f'layer{li + 1}', x)
    pooled = x.mean(dim=(2, 3))
    return F.linear(pooled, sd[prefix + 'fc.weight'], sd[prefix + 'fc.bias'])


def level_channels(config, width=WIDTH):
    mult = (1, 1, 2, 4, 8) if config in synthetic.BASIC_BLOCK_CONFIGS else (1, 4, 8, 16, 32)
    return tuple(m * width for m in mult)


def ablation_cases(config, width=WIDTH):
    """The ablation sets of the goldens, by name."""
    ch = level_channels(config, width)
    return {
        'none': [],
        'conv1_ends': [('conv1', 0), ('conv1', ch[0] - 1)],
        'two_stages': [('layer1', 1), ('layer1', ch[1] - 2), ('layer2', 0), ('layer2', 5)],
        'layer3_thirds': [('layer3', u) for u in range(0, ch[3], 3)],
        'layer4_all': [('layer4', u) for u in range(ch[4])],
        'duplicate': [('layer2', 2), ('layer4', 1), ('layer2', 2)],
    }


def load_goldens():
    """(tensors, meta) of tests/golden/reference_goldens_ablations.*"""
    tensors = torch.load(GOLDEN / 'reference_goldens_ablations.pt')
    meta = json.loads((GOLDEN / 'reference_goldens_ablations.json').read_text())
    return tensors, meta


def state_dict(config, tensors, meta):
    """The model of a golden config: the seeded slim trunk plus the stored head."""
    sd = synthetic.resnet_state_dict(config, seed=meta['configs'][config]['seed'],
                                     width=meta['width'], with_fc=False)
    sd['fc.weight'] = tensors[f'{config}.fc.weight']
    sd['fc.bias'] = tensors[f'{config}.fc.bias']
    return sd
