"""Border-class tiles of the tap-inner k x k convs (csrc/gemm.hip tap_classes / tap_tile;
DESIGN.md 4.1).

A 3x3 / pad 1 convolution multiplies zero padding: of the 9 taps of a border pixel 3 (edge) or
5 (corner) lie outside the image.  The ping-pong kernel groups the output pixels of a launch by
WHICH taps are inside (9 classes for 3x3 / pad 1), builds its 256-row tiles from pixels of one
class and steps over the taps no pixel of the tile has.  A skipped k-tile pair has an all-zero A
operand: per output value the same non-zero products are added in the same order, so the result
is bit for bit that of the linear tile order (`MILAN_TAP_SKIP=0`; test-hook precision
'split_f16_tap_linear').
"""
import os
import pathlib
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from milan_amd import hip

pytestmark = pytest.mark.gpu
REPO = pathlib.Path(__file__).resolve().parent.parent

# (n, h, w, cin, cout, k, stride, pad)
CASES = [
    (23, 14, 14, 64, 256, 3, 1, 1),  # 12-pixel edge classes cross a tile boundary (276 rows), two slices
    (5, 28, 28, 32, 128, 3, 1, 1),   # the 128-column form
    (3, 7, 7, 32, 256, 3, 1, 1),
    (2, 3, 3, 32, 128, 3, 1, 1),     # interior of one pixel
    (2, 2, 2, 32, 256, 3, 1, 1),     # no interior: four corners
    (3, 1, 1, 32, 256, 3, 1, 1),     # one pixel, one tap
    (2, 1, 5, 32, 128, 3, 1, 1),     # one row
    (4, 14, 14, 32, 256, 3, 2, 1),   # stride 2: leading classes only
    (3, 15, 15, 32, 256, 3, 2, 1),   # stride 2, odd size: a trailing class exists
    (2, 13, 13, 64, 256, 5, 1, 2),   # 25 classes: more than the table holds -> linear order
    (3, 14, 15, 32, 256, 3, 2, 1),   # stride 2, non-square: a trailing class on the x axis only
    (3, 15, 14, 32, 256, 3, 2, 1),   # ... on the y axis only
    (2, 7, 1, 32, 128, 3, 1, 1),     # one column
    (2, 28, 3, 32, 256, 3, 1, 1),    # no interior column
    (5, 13, 10, 64, 256, 3, 1, 1),   # 130-pixel images: the classes straddle the tiles unevenly
]
EPILOGUES = ['bias', 'relu', 'residual']


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _check(dev, case, epilogue):
    n, h, w, cin, cout, k, stride, pad = case
    g = torch.Generator().manual_seed(41 + sum(case))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k))**.5
    b = torch.randn(cout, generator=g)
    want = F.conv2d(x.double(), wt.double(), b.double(), stride=stride, padding=pad)
    res = None
    if epilogue == 'residual':
        res = torch.randn(want.shape, generator=g)
        want = (want + res.double()).relu()
        res = res.permute(0, 2, 3, 1).contiguous().to(dev)
    elif epilogue == 'relu':
        want = want.relu()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().to(dev)
    got = {}
    for prec in ('split_f16', 'split_f16_tap_linear', 'f32'):
        got[prec] = hip.conv2d_nhwc(x_nhwc, wt.to(dev), b.to(dev), stride, pad,
                                    relu=epilogue == 'relu', residual=res, precision=prec).cpu()
    scale = float(want.abs().max())
    err = {p: float((y.permute(0, 3, 1, 2).double() - want).abs().max()) for p, y in got.items()}
    print(case, epilogue, {p: f'{e / scale:.2e}' for p, e in err.items()})
    assert torch.equal(got['split_f16'], got['split_f16_tap_linear'])
    assert err['split_f16'] <= max(4 * err['f32'], 2e-6 * scale), err


@pytest.mark.parametrize('case', CASES)
def test_class_tiles_give_the_bits_of_the_linear_order(dev, case):
    """Every class geometry: full 3x3 classes over tile boundaries, both tile widths, images
    of 1 x 1 .. 3 x 3 pixels (classes of one pixel, no interior), one-row images, stride 2 with
    and without a trailing class, and a 5 x 5 kernel whose 25 classes do not fit the table.
    Equal bits to the linear order, fp32-class against fp64 (the bound of
    test_tap_inner_k_order_is_the_same_class_as_tap_major)."""
    _check(dev, case, 'bias')


@pytest.mark.parametrize('epilogue', ['relu', 'residual'])
def test_class_tiles_scatter_through_every_epilogue(dev, epilogue):
    """The epilogue stores (and reads its residual) through the tile's row table."""
    _check(dev, CASES[0], epilogue)


SNIPPET = r'''
import sys, hashlib, torch
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(pkg)r)
from milan_amd import hip, synthetic
nv, width, k, n, size = 60, 16, 5, 6, 96
blocks = synthetic.RESNET_BLOCKS['resnet50']
sd = synthetic.milan_state_dict(nv + 4, config='resnet50', seed=11, width=width, hidden_size=64,
                                embedding_size=16, lm_hidden_size=64, lm_embedding_size=16)
ctx = hip.Context(hip.make_dims(sd, nv, blocks=blocks), sd, torch.device('cuda:0'))
ctx.set_precision('split_f16')
images, masks = synthetic.exemplars(n, k=k, size=size, seed=5, zero_every=0)
masks = masks.clone()
masks[2, 3] = 0   # one all-zero mask: the live image count on the device is below the launch's
h = hashlib.sha256()
flat_i = images.reshape(n * k, 3, size, size).cuda()
flat_m = masks.reshape(n * k, 1, size, size).cuda()
h.update(ctx.encode(flat_i, flat_m).cpu().numpy().tobytes())
out = ctx.describe(images, masks, hip.RERANK, 8, 4, False, 0.2, want_features=True)
for key in ('features', 'tokens', 'scores', 'beam_tokens', 'beam_scores'):
    h.update(out[key].cpu().numpy().tobytes())
print('SHA', h.hexdigest())
'''


def _run(tap_skip):
    env = dict(os.environ, MILAN_TAP_SKIP=str(tap_skip), HSA_ENABLE_IPC_MODE_LEGACY='0')
    hip.release_workspaces()
    code = SNIPPET % dict(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd'))
    done = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True,
                          check=True)
    return [ln for ln in done.stdout.splitlines() if ln.startswith('SHA')][0]


def test_trunk_and_captions_keep_their_bits_with_a_live_count_on_the_device():
    """encode + describe of a slim bottleneck trunk with one empty mask among the exemplars
    (the launches are sized for all images, the kernel derives each class's tiles from the live
    count): MILAN_TAP_SKIP=0 and =1 give the same sha256 of features, tokens, scores, beams."""
    assert _run(1) == _run(0)
