"""The mask-aware tail on row lists (MILAN_FUSE_TAIL_LISTS; csrc/gemm.hip LIST tiles, csrc/encoder.hip).

With the bit on, the pixel sets of the sparse tail go to the ping-pong GEMM tile as device-side
row lists -- a tile is 256 listed pixels of the dense tensors, nothing is gathered, scattered or
unfolded -- and the same treatment reaches the first block of the last stage (c1 at the pixels
its strided 3x3 reads, c2 and c3 + downsample at the pixels the tail needs) and c2 / c3 of the
last block of the stage before.  Contract: per output value the products, their order and the
roundings are those of the dense launch, so everything below is `torch.equal` -- against the
copy-kernel tail (`tail_lists=False`) and against the dense pass (`sparse_tail=False`).
"""
import pytest
import torch

from milan_amd import hip, synthetic

pytestmark = pytest.mark.gpu
PREFIX = 'encoder.encoder.model.'


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


@pytest.fixture(scope='module')
def trunks(dev):
    """One full-width context per architecture, shared by the encoder tests of this file."""
    made = {}

    def get(arch):
        if arch not in made:
            sd = synthetic.resnet_state_dict(arch, seed=3, width=64, prefix=PREFIX)
            ctx = hip.Context(hip.make_dims(sd, 10, blocks=synthetic.RESNET_BLOCKS[arch]), sd, dev)
            ctx.set_precision('split_f16')
            made[arch] = ctx
        return made[arch]

    yield get
    for ctx in made.values():
        ctx.close()


def _masks(kind, n, size, g):
    m = torch.zeros(n, 1, size, size, dtype=torch.uint8)
    for i in range(n):
        if kind == 'rect':
            a = int(torch.randint(max(1, size // 14), max(2, size * 4 // 7), (1,), generator=g))
            b = int(torch.randint(max(1, size // 14), max(2, size * 4 // 7), (1,), generator=g))
            y0 = int(torch.randint(0, size - a + 1, (1,), generator=g))
            x0 = int(torch.randint(0, size - b + 1, (1,), generator=g))
            m[i, 0, y0:y0 + a, x0:x0 + b] = 1
        elif kind == 'random':
            m[i] = (torch.rand(1, size, size, generator=g) > 0.995).to(torch.uint8)
        elif kind == 'full':
            m[i] = 1
        elif kind == 'pixel':
            if i % 2 == 0:
                # misses every centre of the last level (and of most others): the live slot's
                # level-4 list is empty and the dummy-pixel rule gives it its rows
                m[i, 0, 0 if i % 4 == 0 else size - 1, 0] = 1
            else:
                m[i, 0, int(torch.randint(0, size, (1,), generator=g)),
                  int(torch.randint(0, size, (1,), generator=g))] = 1
        elif kind == 'corner':
            m[i, 0, :max(1, size // 5), -max(1, size // 5):] = 1
        elif kind == 'mixed':
            if i % 3 == 0:
                pass                                   # empty: the image skips the trunk
            elif i % 3 == 1:
                m[i, 0, size // 3:size // 2, size // 4:] = 1
            else:
                m[i] = 1
    return m


def _three_ways(ctx, images, masks):
    """features with the lists, with the copy-kernel tail, and dense; the fusion is restored"""
    out = []
    try:
        for sparse_tail, tail_lists in ((True, True), (True, False), (False, False)):
            ctx.set_fusion(sparse_tail=sparse_tail, tail_lists=tail_lists)
            out.append(ctx.encode(images, masks))
            assert ctx.status() == 0, (sparse_tail, tail_lists)
    finally:
        ctx.set_fusion()
    return out


@pytest.mark.parametrize('arch,n,size,kind', [
    ('resnet50', 6, 224, 'rect'),      # 14 x 14 and 7 x 7
    ('resnet101', 3, 224, 'rect'),
    ('resnet50', 5, 224, 'random'),    # scattered pixels: ragged lists
    ('resnet50', 9, 224, 'full'),      # every set is everything: 1764 rows of W = 7 tiles, 441 of S0
    ('resnet50', 8, 224, 'pixel'),     # single pixels, half of them off every level-4 centre
    ('resnet50', 4, 224, 'corner'),
    ('resnet50', 9, 224, 'mixed'),     # with images that skip the trunk
    ('resnet50', 5, 200, 'rect'),      # odd stage-3 size: 13 -> 7, stride 2 with a trailing row
    ('resnet50', 2, 200, 'random'),
    ('resnet50', 3, 200, 'full'),
    ('resnet50', 5, 96, 'rect'),       # 6 x 6 -> 3 x 3
    ('resnet50', 4, 64, 'mixed'),      # 4 x 4 -> 2 x 2
    ('resnet50', 6, 64, 'pixel'),
    ('resnet50', 3, 20, 'full'),       # 2 x 2 -> a 1 x 1 last stage
])
def test_tail_lists_are_bitwise_the_copy_tail_and_the_dense_pass(trunks, arch, n, size, kind):
    ctx = trunks(arch)
    g = torch.Generator().manual_seed(size * 17 + n)
    images = torch.randint(0, 256, (n, 3, size, size), dtype=torch.uint8, generator=g)
    masks = _masks(kind, n, size, g)
    lists, copies, dense = _three_ways(ctx, images, masks)
    assert torch.isfinite(lists).all()
    assert torch.equal(lists, copies)
    assert torch.equal(lists, dense)


def test_a_tile_never_spans_more_slots_than_its_offsets_reach(trunks):
    """2800 images: a full mask on the first and the last, one mask pixel at (0, 0) -- off every
    level-4 centre -- on every image in between.  Their level-4 lists are empty; without the
    dummy pixel the tile that starts in the first image's rows would end 2799 slots further on,
    beyond what a 32-bit buffer offset reaches from the tile's base."""
    ctx = trunks('resnet50')
    n, size = 2800, 224
    g = torch.Generator(device='cuda').manual_seed(5)
    images = torch.randint(0, 256, (n, 3, size, size), dtype=torch.uint8, device='cuda', generator=g)
    masks = torch.zeros(n, 1, size, size, dtype=torch.uint8, device='cuda')
    masks[:, 0, 0, 0] = 1
    masks[0] = 1
    masks[-1] = 1
    try:
        ctx.set_fusion(tail_lists=True)
        lists = ctx.encode(images, masks)
        assert ctx.status() == 0
        ctx.set_fusion(tail_lists=False)
        copies = ctx.encode(images, masks)
        assert ctx.status() == 0
    finally:
        ctx.set_fusion()
    assert torch.isfinite(lists).all()
    assert torch.equal(lists, copies)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 600])
def test_list_lengths_around_the_tile_size(trunks, n):
    """Full masks at size 20: the last stage is 1 x 1, so every tail set has exactly n rows --
    1, one short of a tile, a tile, a tile and one row, 2 tiles and a ragged third -- and V and
    W (2 x 2 pixels per image) 4 n."""
    ctx = trunks('resnet50')
    g = torch.Generator().manual_seed(n)
    images = torch.randint(0, 256, (n, 3, 20, 20), dtype=torch.uint8, generator=g)
    masks = torch.ones(n, 1, 20, 20, dtype=torch.uint8)
    lists, copies, dense = _three_ways(ctx, images, masks)
    assert torch.isfinite(lists).all()
    assert torch.equal(lists, copies)
    assert torch.equal(lists, dense)


def test_describe_is_identical_with_sharing_and_under_graph_replay(dev):
    """describe (beam 50 + rerank, ResNet-101) on 16 neurons, a few of them with empty masks and
    a few exemplars showing the same image: bit on == bit off, also with image sharing, also as
    a captured graph replayed three times."""
    nv, k = 1000, 15
    blocks = synthetic.RESNET_BLOCKS['resnet101']
    sd = synthetic.milan_state_dict(nv + 4, config='resnet101', seed=3)
    ctx = hip.Context(hip.make_dims(sd, nv, blocks=blocks), sd, dev)
    ctx.set_precision('split_f16')
    images, masks = synthetic.exemplars(16, k=k, size=224, seed=7, device='cuda')
    images, masks = images.clone(), masks.clone()
    masks[1, 3] = 0
    masks[6, 14] = 0
    masks[9] = 0                          # a neuron without any work
    images[2, 1] = images[2, 0]           # the same image under two masks
    images[5] = images[5, :1].clone()     # one image, fifteen masks
    keys = ('tokens', 'scores', 'beam_tokens', 'beam_scores')
    call = lambda: ctx.describe(images, masks, hip.RERANK, 15, 50, False, 0.2, check=False)

    def run(tail_lists, sharing):
        ctx.set_fusion(tail_lists=tail_lists)
        ctx.set_image_sharing(sharing)
        out = call()
        torch.cuda.synchronize()
        assert ctx.status() == 0, (tail_lists, sharing)
        return {key: out[key].clone() for key in keys}

    want = run(False, False)
    for tail_lists, sharing in ((True, False), (False, True), (True, True)):
        got = run(tail_lists, sharing)
        for key in keys:
            assert torch.equal(got[key], want[key]), (tail_lists, sharing, key)

    ctx.set_fusion(tail_lists=True)
    ctx.set_image_sharing(False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()
        with torch.cuda.graph(graph, stream=side):
            out = call()
    torch.cuda.current_stream().wait_stream(side)
    for replay in range(3):
        for key in keys:
            out[key].fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for key in keys:
            assert torch.equal(out[key], want[key]), (replay, key)
        assert ctx.status() == 0, replay
    ctx.close()


def test_tail_lists_shorten_the_last_stage(dev):
    """In the manner of test_sparse_tail_skips_most_of_the_last_two_blocks: 64 x 15 images with
    the benchmark's masks, on / off / on / off in one process.  The row fractions of those masks
    (0.11 / 0.33 / 0.57 of the last stage, 0.61 of the one before) predict about 0.6 for the last
    stage; 0.85 leaves room for the row look-up and the fixed cost per launch."""
    blocks = synthetic.RESNET_BLOCKS['resnet101']
    sd = synthetic.resnet_state_dict('resnet101', seed=3, width=64, prefix=PREFIX)
    ctx = hip.Context(hip.make_dims(sd, 10, blocks=blocks), sd, dev)
    ctx.set_precision('split_f16')
    images, masks = synthetic.exemplars(64, k=15, size=224, seed=1, device='cuda')
    images, masks = images.flatten(0, 1), masks.flatten(0, 1)
    hip.profile_enable(True)
    times, l3 = {}, {}
    try:
        for flag in (True, False, True, False):
            ctx.set_fusion(tail_lists=flag)
            ctx.encode(images, masks, check=False)       # warm
            hip.profile_enable(True)
            ctx.encode(images, masks, check=False)
            torch.cuda.synchronize()
            st = hip.profile_read_stages()
            times.setdefault(flag, []).append(st['enc_layer4']['region_ms'])
            l3.setdefault(flag, []).append(st['enc_layer3']['region_ms'])
    finally:
        hip.profile_enable(False)
    print('layer4 ms per 960 images: lists', times[True], 'copies', times[False],
          'ratio %.3f' % (min(times[True]) / min(times[False])))
    print('layer3 ms per 960 images: lists', l3[True], 'copies', l3[False])
    assert min(times[True]) < 0.85 * min(times[False])
    ctx.close()
