"""Reference for the activation-tap tests: `ablref.forward` restated so that it also returns
the five tensors an edit sits on, AFTER the edit -- what the next layer reads, what a retain
hook registered after the ablation hook sees.

The arithmetic is `ablref.forward`'s, call for call (test_activations_host.py ties the logits
to it bit for bit in float32).  It computes in the dtype of its inputs.  Tests only.
"""
import torch.nn.functional as F

import ablref
from oracle import milan_oracle as O

LAYERS = ablref.LAYERS


def forward(images, sd, blocks, ablate=(), prefix=''):
    """(n,3,H,W) -> (logits (n, classes), {layer: (n, C, h, w) edited output})."""
    sd = {k: v.to(images.dtype) if v.dtype.is_floating_point else v for k, v in sd.items()}
    edit = ablref.masks_of(ablate, images)
    taps = {}
    x = F.conv2d(images, sd[prefix + 'conv1.weight'], None, stride=2, padding=3)
    x = edit('conv1', x)
    taps['conv1'] = x
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
        taps[f'layer{li + 1}'] = x
    pooled = x.mean(dim=(2, 3))
    logits = F.linear(pooled, sd[prefix + 'fc.weight'], sd[prefix + 'fc.bias'])
    return logits, taps
