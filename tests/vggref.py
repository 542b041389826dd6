"""Reference for the VGG tests: torchvision's VGG-11 / 13 / 16 / 19 without batch norm in eval
mode with unit ablation, restated with plain `torch.nn.functional` calls on a state dict under
torchvision's key names (`features.N`, `classifier.0 / 3 / 6`).  torchvision itself is not
needed: the structure is written out here, independently of `milan_amd.synthetic`.

It computes in the dtype of its input: float64 for the GPU tests' bound, float32 to tie
`classifiers.VGGClassifier.forward_eager` to it bit for bit.  Tests only.

Edit points: the last conv of each of the five blocks (the reference's LAYERS.VGG11 .. VGG19).
What the pool reads, and what a retain hook sees behind the in-place ReLU, is relu(conv + bias)
x mask; `forward` returns those five tensors as the taps.

Seeded init: conv and Linear weights randn * sqrt(2 / fan_in), biases 0.05 * randn, images
randn.  With it the fp32 CPU forward stays at or below 0.26 x FEATURE_CLASS on every tap and on
the logits against float64 (all four configs, widths 8 and 16, 32x32 .. 299x331), and
activations stay below 25.
"""
import torch
import torch.nn.functional as F

# convs per block; a block's channels per unit of width
BLOCKS = {
    'vgg11': (1, 1, 2, 2, 2),
    'vgg13': (2, 2, 2, 2, 2),
    'vgg16': (2, 2, 3, 3, 3),
    'vgg19': (2, 2, 4, 4, 4),
}
CHANNELS = (1, 2, 4, 8, 8)
# the reference's LAYERS.VGG11 .. VGG19 (src/exemplars/models.py), written out
LAYERS = {
    'vgg11': ('features.0', 'features.3', 'features.8', 'features.13', 'features.18'),
    'vgg13': ('features.2', 'features.7', 'features.12', 'features.17', 'features.22'),
    'vgg16': ('features.2', 'features.7', 'features.14', 'features.21', 'features.28'),
    'vgg19': ('features.2', 'features.7', 'features.16', 'features.25', 'features.34'),
}


def conv_indices(config):
    """Per block, the `features` indices of its convs (a ReLU behind each conv, a pool behind
    each block)."""
    out, at = [], 0
    for count in BLOCKS[config]:
        block = []
        for _ in range(count):
            block.append(at)
            at += 2
        out.append(block)
        at += 1
    return out


def config_of(sd):
    """The config whose conv keys the state dict has."""
    have = sorted(int(k.split('.')[1]) for k in sd if k.startswith('features.') and
                  k.endswith('.weight'))
    for config in BLOCKS:
        if have == [i for block in conv_indices(config) for i in block]:
            return config
    raise ValueError(f'not a VGG state dict: features {have}')


def channels(width):
    return tuple(m * width for m in CHANNELS)


def make_state_dict(seed, config, width, hidden, classes):
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for mult, block in zip(CHANNELS, conv_indices(config)):
        for index in block:
            cout = mult * width
            sd[f'features.{index}.weight'] = (torch.randn(cout, cin, 3, 3, generator=g) *
                                              (2.0 / (cin * 9))**0.5)
            sd[f'features.{index}.bias'] = 0.05 * torch.randn(cout, generator=g)
            cin = cout
    for index, fan, out in ((0, cin * 49, hidden), (3, hidden, hidden), (6, hidden, classes)):
        sd[f'classifier.{index}.weight'] = torch.randn(out, fan, generator=g) * (2.0 / fan)**0.5
        sd[f'classifier.{index}.bias'] = 0.05 * torch.randn(out, generator=g)
    return sd


def make_images(seed, n, geo):
    g = torch.Generator().manual_seed(seed + 1000 * geo[0] + geo[1])
    return torch.randn(n, 3, *geo, generator=g)


def forward(images, sd, ablated_units=()):
    """(n,3,H,W) -> ((n, classes) logits, [five taps]) under the set [(level 0..4 or its
    `features.N` name, unit), ...], masks applied after the ReLU.  The logits are None when
    the image is too small for pool5 to leave a pixel (the taps up to the last level that
    exists still come) or when the state dict has no classifier."""
    config = config_of(sd)
    sd = {k: v.to(images.dtype) for k, v in sd.items()}
    units = {}
    for level, unit in ablated_units:
        if isinstance(level, str):
            level = LAYERS[config].index(level)
        units.setdefault(int(level), []).append(int(unit))
    taps = []
    x = images
    for level, block in enumerate(conv_indices(config)):
        if level > 0:
            if min(x.shape[2:]) < 2:
                return None, taps
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for index in block:
            x = F.relu(F.conv2d(x, sd[f'features.{index}.weight'], sd[f'features.{index}.bias'],
                                stride=1, padding=1))
        if level in units:
            mask = x.new_ones(1, x.shape[1], 1, 1)
            mask[:, units[level]] = 0
            x = x * mask
        taps.append(x)
    if min(x.shape[2:]) < 2 or 'classifier.0.weight' not in sd:
        return None, taps
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = torch.flatten(F.adaptive_avg_pool2d(x, (7, 7)), 1)
    x = F.relu(F.linear(x, sd['classifier.0.weight'], sd['classifier.0.bias']))
    x = F.relu(F.linear(x, sd['classifier.3.weight'], sd['classifier.3.bias']))
    return F.linear(x, sd['classifier.6.weight'], sd['classifier.6.bias']), taps
