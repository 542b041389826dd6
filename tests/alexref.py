"""Reference for the AlexNet tests: the reference's `alexnet_seq` (torchvision's AlexNet as one
sequential: conv1 .. conv5, fc6, fc7, linear8) in eval mode with unit ablation, restated on a
state dict with `classifiers.AlexNetClassifier`'s key names.

It computes in the dtype of its inputs: float64 for the GPU tests' bound, float32 to tie the
restatement itself to the reference's goldens.  Tests only.

Edit points (LAYERS.ALEXNET of src/exemplars/models.py; nethook edits a module's OUTPUT, and
every conv is followed by an in-place ReLU): what the next layer reads, and what a retain hook
sees, is relu(conv + bias) x mask.  `forward` returns those five tensors as the taps.

The goldens hold results only; the model and the images are regenerated from the seeds in the
.json (`state_dict`, `images`), as the ResNet goldens regenerate their trunks.
"""
import json
import pathlib

import torch
import torch.nn.functional as F

from milan_amd import synthetic

LAYERS = ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')
FEATURES = (0, 3, 6, 8, 10)          # torchvision's features.N of conv1..conv5
CONV = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))   # (stride, padding)
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'


def channels(width):
    return tuple(m * width for m in synthetic.ALEXNET_CHANNELS)


def forward(images, sd, ablate=()):
    """(n,3,H,W) -> ((n, classes) logits, {layer: tap}) under the set [(layer, unit), ...]."""
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    units = {}
    for layer, unit in ablate:
        if layer not in LAYERS:
            raise ValueError(f'Layer {layer} not found in model')
        units.setdefault(layer, []).append(int(unit))
    taps = {}
    x = images
    for index, layer in enumerate(LAYERS):
        stride, padding = CONV[index]
        x = F.relu(F.conv2d(x, sd[f'{layer}.weight'], sd[f'{layer}.bias'], stride=stride,
                            padding=padding))
        if layer in units:
            mask = x.new_ones(1, x.shape[1], 1, 1)
            mask[:, units[layer]] = 0
            x = x * mask
        taps[layer] = x
        if index in (0, 1, 4):
            x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = torch.flatten(F.adaptive_avg_pool2d(x, (6, 6)), 1)
    x = F.relu(F.linear(x, sd['fc6.weight'], sd['fc6.bias']))
    x = F.relu(F.linear(x, sd['fc7.weight'], sd['fc7.bias']))
    return F.linear(x, sd['linear8.weight'], sd['linear8.bias']), taps


def make_state_dict(seed, width, hidden, classes, head_scale=1.0):
    """Seeded model: `synthetic.alexnet_state_dict`'s convs under the classifier's names, Linear
    weights ~ N(0, 1 / fan_in) (linear8 times `head_scale`), small random biases."""
    tv = synthetic.alexnet_state_dict(seed=seed, width=width, with_classifier=False)
    sd = {}
    for layer, index in zip(LAYERS, FEATURES):
        sd[f'{layer}.weight'] = tv[f'features.{index}.weight']
        sd[f'{layer}.bias'] = tv[f'features.{index}.bias']
    g = torch.Generator().manual_seed(seed + 100)
    fan = channels(width)[4] * 36
    for name, out_f, in_f, scale in (('fc6', hidden, fan, 1.0), ('fc7', hidden, hidden, 1.0),
                                     ('linear8', classes, hidden, head_scale)):
        sd[f'{name}.weight'] = torch.randn(out_f, in_f, generator=g) * (scale * in_f**-0.5)
        sd[f'{name}.bias'] = 0.05 * torch.randn(out_f, generator=g)
    return sd


def make_images(seed, n, geo):
    g = torch.Generator().manual_seed(seed + 1000 * geo[0] + geo[1])
    return torch.randn(n, 3, *geo, generator=g)


def ablation_cases(width):
    """The ablation sets of the goldens, by name."""
    ch = channels(width)
    cases = {'none': []}
    for index, layer in enumerate(LAYERS):   # one unit per level
        cases[f'{layer}_one'] = [(layer, (3 * index + 1) % ch[index])]
    cases['mixed'] = [('conv1', 0), ('conv1', ch[0] - 1), ('conv2', 5), ('conv3', ch[2] - 2),
                      ('conv3', 7), ('conv5', 1), ('conv5', ch[4] - 1), ('conv3', 7)]
    cases['conv5_all'] = [('conv5', u) for u in range(ch[4])]
    return cases


def load_goldens():
    """(tensors, meta) of tests/golden/reference_goldens_alexnet.*"""
    tensors = torch.load(GOLDEN / 'reference_goldens_alexnet.pt')
    meta = json.loads((GOLDEN / 'reference_goldens_alexnet.json').read_text())
    return tensors, meta


def state_dict(meta):
    return make_state_dict(meta['seed'], meta['width'], meta['hidden'], meta['classes'],
                           meta['head_scale'])


def images(meta, geo):
    return make_images(meta['seed'], meta['n_images'], tuple(geo))
