"""A float64 yardstick for the full-width bottleneck trunk, the case generators of
tests/test_gpu_full_width.py and the mutants that show what the yardstick resolves.

Host only: torch on the CPU, no HIP import.  `encode64` is `oracle.milan_oracle.encode` with every
floating tensor of the state dict and every activation in float64.  Three things stay in float32
and are then promoted, because that is what the reference computes and what the HIP path
restates bit for bit: `byte_to_float`, the bilinear mask resize, and the "row
is all close to zero" validity rule.  The trunk is restated here (`resnet_trunk`) so that a hook
can reach single layers; tests/test_trunk_ref_host.py pins the restatement with `torch.equal`
against `milan_oracle.resnet_trunk` on the same float64 inputs.

The hook is one callable `hook(point, name, value, **context) -> value`; the points:

  'block_in'  name 'layerL.B'        value: the block's input x
  'conv2'     name 'layerL.B.conv2'  value: the raw 3x3 output; context x (its input), weight, stride
  'resize'    name level 0..4        value: the float32 resized masks; context masks, size
  'weights'   name level 0..4        value: the float64 normalised pooling weights; context resized
"""
import torch
import torch.nn.functional as F

from oracle import milan_oracle as O

PREFIX = 'encoder.encoder.model.'
WIDTH = 64

# (h, w): the path it forces
GEOMETRIES = [
    (224, 224),  # the real geometry: 112 / 56 / 28 / 14 / 7
    (97, 131),   # W % 4 != 0: no uint8 stem read, the pixel-pair path; odd sizes (49 x 66 .. 4 x 5)
    (200, 150),  # stage 3 is 13 x 10, stage 4 7 x 5: a stride-2 trailing row, no trailing column
    (150, 200),  # its transpose: a trailing column, no trailing row
    (64, 232),   # layer1 is 16 x 58 > kConvMaxW = 56: conv-front falls back, conv3_p64 and the chain run
    (33, 47),    # small: 17 x 24 .. 2 x 2
    (20, 52),    # the last stage is 1 x 2
    (7, 9),      # small: layer2 is 1 x 2, layer3 onwards 1 x 1
    (1, 1),      # the smallest possible
    (4, 300),    # a one-row last stage (1 x 10) and long rows (conv1 2 x 150)
]
KINDS = ['full', 'pixel', 'corners', 'ring', 'rowcol', 'sparse', 'soft', 'mixed', 'none']


def level_sizes(h, w):
    """(h, w) of the five taps: every stage halves, rounding up (k 7 / s 2 / p 3, k 3 / s 2 / p 1)."""
    out = []
    for _ in range(5):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def tail_runs(h, w, width=WIDTH):
    """The host's condition for the mask-aware tail (csrc/encoder.hip, section 3b), restated for
    a bottleneck trunk in split_f16 with masks: the scratch of a sparse block -- per level-4 pixel
    2 x c1.cin + c3.cout + 11 x c1.cout floats of the last block (c1.cin = c3.cout = 32 x width,
    c1.cout = 8 x width) -- must fit the raw conv1 tensor of one image, h1 x w1 x width floats.
    Where it does not, the last stage runs densely whatever the fusion bits say, and no row list
    is built."""
    sizes = level_sizes(h, w)
    p4 = sizes[4][0] * sizes[4][1]
    need = p4 * (2 * 32 * width + 32 * width + 11 * 8 * width)
    return 1 <= p4 <= 1024 and need <= sizes[0][0] * sizes[0][1] * width


# Batch sizes of the matrix.  The tail (and with it the row lists V / W at level 3, S0 at level 4)
# runs at the first five geometries but (97, 131); the others take the dense last stage, and their
# batch sizes only put many small images into one launch.  No batch exceeds 9 images of 240 x 240
# in pixels.
#   (h, w): n          tail: level-3 / level-4 rows with full masks
BATCHES = {
    (224, 224): 2,   # 392 / 98
    (97, 131): 4,    # no tail
    (200, 150): 2,   # 260 / 70
    (150, 200): 3,   # 390 / 105
    (64, 232): 4,    # 240 / 64
    (33, 47): 7,     # no tail
    (20, 52): 32,    # no tail
    (7, 9): 255,     # no tail
    (1, 1): 257,     # no tail
    (4, 300): 9,     # no tail
}
# List lengths around the 256-row tile, at geometries where `tail_runs`: with full masks every
# level-3 pixel is in V and W and every level-4 pixel in S0 (and in the two sets derived from it).
#   (30, 26): 15 x 13 .. 2 x 2, 1 x 1: S0 has n rows, V / W 4 n
#   (240, 272): level 3 is 15 x 17 = 255 pixels, level 4 8 x 9;  (256, 256): 16 x 16 = 256, 8 x 8
# 257 is prime: no batch of full masks gives V / W that length; 4 x 64 = 256, 1020 / 1024 / 1028
# (four tiles less / and four rows) and the single images stand for level 3.
# The two single images are the only inputs above 240 pixels on a side (272 and 256): level 3 has
# 255 or 256 pixels only from there on, and one image of that size costs less than the matrix's
# two of 224 x 224.
#   ((h, w), n, kind, level-3 rows, level-4 rows)
LIST_CASES = [
    ((30, 26), 1, 'full', 4, 1),
    ((30, 26), 64, 'full', 256, 64),
    ((30, 26), 255, 'full', 1020, 255),
    ((30, 26), 256, 'full', 1024, 256),
    ((30, 26), 257, 'full', 1028, 257),
    ((240, 272), 1, 'full', 255, 72),
    ((256, 256), 1, 'full', 256, 64),
]
# ... and the smallest batch of the smallest image, 257 single pixels without the tail
EXTRA_CASES = [((1, 1), 1, 'full'), ((7, 9), 257, 'pixel')] + [c[:3] for c in LIST_CASES]


def case_seed(h, w, n, kind):
    return 7919 * h + 131 * w + 17 * n + KINDS.index(kind)


def images_of(n, h, w, generator, as_float=False):
    images = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=generator)
    return O.byte_to_float(images) if as_float else images


def masks_of(kind, n, h, w, generator):
    """(n, 1, h, w) masks of one kind (uint8; float for 'soft'; None for 'none')."""
    g = generator
    if kind == 'none':
        return None
    m = torch.zeros(n, 1, h, w, dtype=torch.uint8)
    if kind == 'full':
        m[:] = 1
    elif kind == 'pixel':
        # half the images: (0, 0) or (h-1, w-1), which miss every centre of the last level
        for i in range(n):
            if i % 2 == 0:
                y, x = (0, 0) if i % 4 == 0 else (h - 1, w - 1)
            else:
                y = int(torch.randint(0, h, (1,), generator=g))
                x = int(torch.randint(0, w, (1,), generator=g))
            m[i, 0, y, x] = 1
    elif kind == 'corners':
        m[:, 0, 0, 0] = 1
        m[:, 0, 0, -1] = 1
        m[:, 0, -1, 0] = 1
        m[:, 0, -1, -1] = 1
    elif kind == 'ring':
        m[:, 0, 0, :] = 1
        m[:, 0, -1, :] = 1
        m[:, 0, :, 0] = 1
        m[:, 0, :, -1] = 1
    elif kind == 'rowcol':
        for i in range(n):
            m[i, 0, int(torch.randint(0, h, (1,), generator=g)), :] = 1
            m[i, 0, :, int(torch.randint(0, w, (1,), generator=g))] = 1
    elif kind == 'sparse':
        m = (torch.rand(n, 1, h, w, generator=g) > 0.995).to(torch.uint8)
    elif kind == 'soft':
        m = (torch.rand(n, 1, h, w, generator=g) > 0.9).float() * torch.rand(n, 1, h, w, generator=g)
    elif kind == 'mixed':
        for i in range(n):
            if i % 3 == 1:
                m[i, 0, h // 3:max(h // 3 + 1, h // 2), w // 4:] = 1
            elif i % 3 == 2:
                m[i] = 1
    else:
        raise KeyError(kind)
    return m


def make_case(h, w, n, kind, float_images=False):
    """The inputs of one matrix case, from its own seed."""
    g = torch.Generator().manual_seed(case_seed(h, w, n, kind))
    images = images_of(n, h, w, g, as_float=float_images)
    return images, masks_of(kind, n, h, w, g)


def matrix_cases():
    """[(h, w, n, kind)]: GEOMETRIES x KINDS at the geometry's batch size, then EXTRA_CASES."""
    cases = [(h, w, BATCHES[(h, w)], kind) for (h, w) in GEOMETRIES for kind in KINDS]
    return cases + [(h, w, n, kind) for (h, w), n, kind in EXTRA_CASES]


def case_id(case):
    h, w, n, kind = case
    return f'{h}x{w}-n{n}-{kind}'


# ---------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------
def _call(hook, point, name, value, **context):
    return value if hook is None else hook(point, name, value, **context)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'],
                        sd[p + '.bias'], False, 0.0, O.BN_EPS)


def resnet_trunk(x, sd, prefix=PREFIX, blocks=(3, 4, 6, 3), hook=None):
    """The bottleneck branch of `milan_oracle.resnet_trunk`, with the hook points."""
    taps = []
    x = F.conv2d(x, sd[prefix + 'conv1.weight'], None, stride=2, padding=3)
    taps.append(x)
    x = F.relu(_bn(x, sd, prefix + 'bn1'))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for li, nblocks in enumerate(blocks):
        for bi in range(nblocks):
            name = f'layer{li + 1}.{bi}'
            p = f'{prefix}{name}.'
            stride = 2 if (bi == 0 and li > 0) else 1
            x = _call(hook, 'block_in', name, x)
            identity = x
            out = F.relu(_bn(F.conv2d(x, sd[p + 'conv1.weight']), sd, p + 'bn1'))
            c2 = F.conv2d(out, sd[p + 'conv2.weight'], stride=stride, padding=1)
            c2 = _call(hook, 'conv2', name + '.conv2', c2, x=out, weight=sd[p + 'conv2.weight'],
                       stride=stride)
            out = F.relu(_bn(c2, sd, p + 'bn2'))
            out = _bn(F.conv2d(out, sd[p + 'conv3.weight']), sd, p + 'bn3')
            if (p + 'downsample.0.weight') in sd:
                identity = _bn(F.conv2d(x, sd[p + 'downsample.0.weight'], stride=stride), sd,
                               p + 'downsample.1')
            x = F.relu(out + identity)
        taps.append(x)
    return taps


def pool_weights(masks, sizes, hook=None):
    """Per level the float64 pooling weights (n, 1, h_l, w_l): resize and validity in float32
    (`milan_oracle.pyramid_pool`), the normalisation of the valid rows in float64."""
    out = []
    for level, size in enumerate(sizes):
        ms = F.interpolate(masks, size=size, mode='bilinear', align_corners=False)
        ms = _call(hook, 'resize', level, ms, masks=masks, size=size)
        valid = ~ms.isclose(torch.zeros_like(ms)).all(dim=-1).all(dim=-1).view(-1)
        wt = ms.double()
        wt[valid] = wt[valid] / wt[valid].sum(dim=(-1, -2), keepdim=True)
        out.append(_call(hook, 'weights', level, wt, resized=ms))
    return out


def double_state(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def encode64(images, masks, sd, blocks, hook=None, chunk=16):
    """(M, 3, H, W) uint8 or float images [+ (M, 1, H, W) masks or None] -> (M, F) float64."""
    sd64 = sd if sd[PREFIX + 'conv1.weight'].dtype == torch.float64 else double_state(sd)
    x = O.byte_to_float(images) if images.dtype == torch.uint8 else images.float()
    m, _, h, w = x.shape
    masks = x.new_ones(m, 1, h, w) if masks is None else masks.float()  # encoders.py:292-293
    mean = torch.tensor(O.IMAGENET_MEAN).view(1, 3, 1, 1).double()
    std = torch.tensor(O.IMAGENET_STD).view(1, 3, 1, 1).double()
    outs = []
    with torch.no_grad():
        for i in range(0, m, chunk):
            taps = resnet_trunk((x[i:i + chunk].double() - mean) / std, sd64, blocks=blocks, hook=hook)
            outs.append(taps)
        taps = [torch.cat([o[level] for o in outs]) for level in range(5)]
        weights = pool_weights(masks, [t.shape[-2:] for t in taps], hook=hook)
        return torch.cat([t.mul(wt).sum(dim=(-1, -2)) for t, wt in zip(taps, weights)], dim=-1)


def encode32(images, masks, sd, blocks):
    """The fp32 CPU oracle on the same flat inputs -> (M, F) float32."""
    x = O.byte_to_float(images) if images.dtype == torch.uint8 else images.float()
    m, _, h, w = x.shape
    masks = x.new_ones(m, 1, h, w) if masks is None else masks.float()
    with torch.no_grad():
        return O.encode(x[None], masks[None], sd, blocks=blocks, chunk=16)[0]


# ---------------------------------------------------------------------------
# Mutants: each is a bug of the kind the full-width tests are for, as a hook
# ---------------------------------------------------------------------------
def drop_lightest_pixel(level, row=None):
    """(a) one listed pixel -- the one with the smallest non-zero resized weight -- is missing
    from one row's pooling at `level` (the row: `row`, or the first with two listed pixels)."""
    def hook(point, name, value, **context):
        if point != 'weights' or name != level:
            return value
        ms = context['resized'].flatten(1)
        rows = [row] if row is not None else [i for i in range(len(ms)) if int((ms[i] != 0).sum()) > 1]
        assert rows, 'no row with two listed pixels at this level'
        r = rows[0]
        cand = torch.where(ms[r] != 0, ms[r], torch.full_like(ms[r], float('inf')))
        value = value.clone()
        value.flatten(1)[r, int(cand.argmin())] = 0
        return value
    return hook


def skip_inside_tap(conv, tap=(1, 2)):
    """(b) at the output pixel (0, 0) of every image one inside tap of `conv` ('layerL.B.conv2')
    is skipped: tap (ky, kx) reads input (ky - 1, kx - 1) there."""
    ky, kx = tap

    def hook(point, name, value, **context):
        if point != 'conv2' or name != conv:
            return value
        x, wt = context['x'], context['weight']
        assert x.shape[-2] > ky - 1 and x.shape[-1] > kx - 1, 'the tap is not inside'
        value = value.clone()
        value[:, :, 0, 0] -= x[:, :, ky - 1, kx - 1] @ wt[:, :, ky, kx].t()
        return value
    return hook


def outside_tap_as_inside(conv):
    """(b) at the output pixel (0, 0) the tap left of the image (ky 1, kx 0) is read as if it were
    inside, with a wrapped column index: it takes the last pixel of the image's first row."""
    def hook(point, name, value, **context):
        if point != 'conv2' or name != conv:
            return value
        x, wt = context['x'], context['weight']
        value = value.clone()
        value[:, :, 0, 0] += x[:, :, 0, -1] @ wt[:, :, 1, 0].t()
        return value
    return hook


def swapped_resize(level):
    """(c) the mask resize of `level` is built with h and w swapped: resized to (w_l, h_l) and
    read back row-major as (h_l, w_l)."""
    def hook(point, name, value, **context):
        if point != 'resize' or name != level:
            return value
        hl, wl = context['size']
        wrong = F.interpolate(context['masks'], size=(wl, hl), mode='bilinear', align_corners=False)
        return wrong.reshape(value.shape)
    return hook


def sibling_mask(slot, sibling):
    """(d) a duplicate-image slot is pooled with its sibling's mask, at every level."""
    def hook(point, name, value, **context):
        if point != 'resize':
            return value
        value = value.clone()
        value[slot] = value[sibling]
        return value
    return hook


def shifted_stride2_set(block='layer4.0'):
    """(e) `block` reads its stride-2 input set one column to the right: input column 2 x + 1
    where 2 x belongs, zeros past the last column."""
    def hook(point, name, value, **context):
        if point != 'block_in' or name != block:
            return value
        return F.pad(value[..., 1:], (0, 1))
    return hook


# ---------------------------------------------------------------------------
# Duplicate images (image sharing) and the fuzz draws
# ---------------------------------------------------------------------------
# (h, w, which): slot i shows distinct image which[i]; every slot has its own mask.  The tail
# runs at all three (`tail_runs`): with sharing its level-3 / level-4 lists are unions per class.
DUPLICATE_CASES = [
    (150, 200, (0, 1, 0, 2, 1, 0, 2)),
    (200, 150, (0, 0, 1, 0)),
    (64, 232, (0, 1, 2, 2, 1, 0, 0, 1, 2)),
]
DUPLICATE_KINDS = ('sparse', 'soft', 'rowcol', 'sparse', 'ring', 'sparse', 'pixel', 'soft', 'sparse')


def duplicate_case(h, w, which, seed=0):
    """Slots that show the same image under different sparse masks.  The root (first slot) of
    class 0 has an empty mask, and so has the last slot, which is no root."""
    g = torch.Generator().manual_seed(case_seed(h, w, len(which), 'sparse') + 1000003 * (seed + 1))
    distinct = images_of(max(which) + 1, h, w, g)
    images = distinct[list(which)].contiguous()
    masks = torch.cat([masks_of(DUPLICATE_KINDS[i % len(DUPLICATE_KINDS)], 1, h, w, g).float()
                       for i in range(len(which))])
    masks[0] = 0
    masks[-1] = 0
    assert which.index(which[-1]) != len(which) - 1
    return images, masks


def draw_fuzz(seed):
    """One seeded draw of test_fuzz_full_width: sizes from {1..12} U {13..240} per axis."""
    import random
    r = random.Random(seed)
    h = r.choice([r.randint(1, 12), r.randint(13, 240)])
    w = r.choice([r.randint(1, 12), r.randint(13, 240)])
    return dict(h=h, w=w, n=r.randint(1, 9), kind=r.choice(KINDS),
                duplicates=r.choice(['none', 'none', 'pairs', 'all_same', 'root_empty']),
                precision=r.choice(['split_f16', 'f32']))


def fuzz_case(seed):
    p = draw_fuzz(seed)
    n, h, w = p['n'], p['h'], p['w']
    g = torch.Generator().manual_seed(seed)
    images = images_of(n, h, w, g)
    masks = masks_of(p['kind'], n, h, w, g)
    if p['duplicates'] == 'pairs':
        images[n // 2:] = images[:n - n // 2].clone()
    elif p['duplicates'] in ('all_same', 'root_empty'):
        images[:] = images[0].clone()
        if p['duplicates'] == 'root_empty' and masks is not None:
            masks[0] = 0
    return p, images, masks


# ResNet-101 (22 chained layer3 blocks behind layer3.0): the real geometry and one odd one
CASES_101 = [(224, 224, 2, 'sparse'), (97, 131, 4, 'soft')]
# float images: one case of the matrix, its uint8 images converted on the host
FLOAT_CASE = (97, 131, 4, 'sparse')
# describe: 8 neurons x 2 exemplars of 150 x 200 under sparse masks
DESCRIBE_CASE = (150, 200, 16, 'sparse')
DESCRIBE_VOCAB = 60


def describe_state_dict():
    from milan_amd import synthetic
    return synthetic.milan_state_dict(DESCRIBE_VOCAB + 4, config='resnet50', seed=3, width=WIDTH,
                                      hidden_size=64, embedding_size=16, lm_hidden_size=64,
                                      lm_embedding_size=16)
