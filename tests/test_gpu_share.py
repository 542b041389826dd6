"""Exemplar slots that show the same image share one trunk pass (opt-in image sharing).

The reference runs the trunk on the unmasked image and the masks enter at the pooling only
(src/milan/encoders.py:295-318): features of slot i = pool(trunk(image_i), mask_i).  With
`Context.set_image_sharing(True)` the slots of one encoder pass whose uint8 images are byte
for byte identical go through the trunk once (csrc/share.hip) and every slot pools its own
mask from that result.  Nothing may change by one bit, two different images must never be
merged (the hash only selects candidates for a byte comparison), the pass stays free of
synchronisation, and the device-side counters report exactly how many images the trunk ran.
"""
import os
import pathlib
import subprocess
import sys

import pytest
import torch

import milan_amd
from milan_amd import decoders, encoders, hip, lang, lms, synthetic
from oracle import milan_oracle as O
from featclass import FEATURE_CLASS, feature_error
from test_gpu_dtype_error import PREFIX

pytestmark = pytest.mark.gpu
REPO = pathlib.Path(__file__).resolve().parent.parent
BLOCKS = synthetic.RESNET_BLOCKS['resnet50']
PRECISIONS = ['split_f16', 'f32', 'f16']


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


def small_ctx(dev):
    sd = synthetic.resnet_state_dict('resnet50', seed=13, width=16, prefix=PREFIX)
    c = hip.Context(hip.make_dims(sd, 10, blocks=BLOCKS), sd, dev)
    c.sd = sd
    return c


@pytest.fixture(scope='module')
def ctx(dev):
    c = small_ctx(dev)
    yield c
    c.close()


@pytest.fixture(scope='module')
def base():
    """12 distinct 64 x 64 images with one non-empty rectangle mask each (never modified)."""
    images, masks = synthetic.exemplars(4, k=3, size=64, seed=17, zero_every=0)
    images, masks = images.reshape(12, 3, 64, 64), masks.reshape(12, 1, 64, 64)
    assert len({im.numpy().tobytes() for im in images}) == 12
    assert all(bool(m.any()) for m in masks)
    return images, masks


def bump(image, index):
    """the image with exactly one byte changed (index < 0 counts from the end)"""
    out = image.clone()
    flat = out.view(-1)
    flat[index] = (int(flat[index]) + 1) % 256
    return out


def make(pattern, base, hw=(64, 64)):
    """(images, masks) of one duplicate pattern, cropped to hw"""
    images, masks = (t[..., :hw[0], :hw[1]].contiguous().clone() for t in base)
    if pattern == 'none':
        pass
    elif pattern == 'pairs':
        images[3] = images[0]; images[7] = images[0]; images[11] = images[5]
    elif pattern == 'all_same':
        images[:] = images[0]
    elif pattern == 'same_image_same_mask':
        images[3] = images[0]; masks[3] = masks[0]
        images[9] = images[4]; masks[9] = masks[4]
    elif pattern == 'root_mask_empty':
        images[6] = images[2]; masks[2] = 0
    elif pattern == 'class_all_empty':
        images[6] = images[2]; masks[2] = 0; masks[6] = 0; masks[9] = 0
    elif pattern == 'near_duplicate':
        size = images[0].numel()
        # a byte of the last, partial 16-byte block where there is one (3 * 61 * 60 = 10980 =
        # 686 * 16 + 4), else of the last full block
        tail = size - 3 if size % 16 else size - 11
        images[3] = bump(images[0], 0)
        images[7] = bump(images[0], -1)
        images[11] = bump(images[0], tail)
        images[9] = images[4]          # (a true duplicate next to them is still found)
    else:
        raise KeyError(pattern)
    return images, masks


def live_classes(images, masks, skip_empty=True):
    """number of classes of byte-identical images with work, computed on the host: a class is
    live if a member's mask is not empty (every class when skip_empty is off or masks is None)"""
    live = {}
    for i, im in enumerate(images):
        key = im.cpu().numpy().tobytes()
        has = True if masks is None or not skip_empty else bool(masks[i].any())
        live[key] = live.get(key, False) or has
    return sum(live.values())


def on_vs_off(c, images, masks, expect_trunk, slots=None):
    """sharing on == off bit for bit; the counters are exact; returns the features"""
    c.set_image_sharing(False)
    want = c.encode(images, masks).cpu()
    c.set_image_sharing(True)
    assert c.image_sharing
    c.image_sharing_stats(clear=True)
    got = c.encode(images, masks).cpu()
    stats = c.image_sharing_stats(clear=True)
    c.set_image_sharing(False)
    assert torch.equal(got, want)
    assert stats == (len(images) if slots is None else slots, expect_trunk), stats
    assert c.image_sharing_stats() == (0, 0)
    return got


PATTERNS = ['none', 'pairs', 'all_same', 'same_image_same_mask', 'root_mask_empty',
            'class_all_empty', 'near_duplicate']
EXPECT = {'none': 12, 'pairs': 9, 'all_same': 1, 'same_image_same_mask': 10,
          'root_mask_empty': 11, 'class_all_empty': 9, 'near_duplicate': 11}


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_sharing_changes_no_bit_small_trunk(ctx, base, precision, pattern):
    images, masks = make(pattern, base)
    expect = live_classes(images, masks)
    assert expect == EXPECT[pattern]
    ctx.set_precision(precision)
    ctx.set_fusion()
    got = on_vs_off(ctx, images, masks, expect)
    if pattern == 'root_mask_empty':
        assert (got[2] == 0).all() and got[6].abs().max() > 0
    if pattern == 'class_all_empty':
        assert (got[[2, 6, 9]] == 0).all()
    if pattern == 'same_image_same_mask':
        assert torch.equal(got[3], got[0]) and torch.equal(got[9], got[4])


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('offset', [0, 1])
def test_near_duplicates_at_a_size_that_is_no_multiple_of_16(ctx, base, precision, offset):
    """61 x 60 pixels: 3 * H * W = 10980 is no multiple of 16 (a 4-byte tail) while W % 4 == 0
    keeps the uint8 stem; image i starts 4 i bytes past a 16-byte boundary.  `offset` 1: the
    whole buffer starts on an odd address (the byte-wise loads)."""
    images, masks = make('near_duplicate', base, hw=(61, 60))
    expect = live_classes(images, masks)
    assert len({im.numpy().tobytes() for im in images}) == 11 and 9 <= expect <= 11
    buf = torch.empty(images.numel() + 16, dtype=torch.uint8, device='cuda')
    dimg = buf[offset:offset + images.numel()].view(images.shape)
    dimg.copy_(images)
    assert dimg.data_ptr() % 16 == offset and dimg.is_contiguous()
    ctx.set_precision(precision)
    ctx.set_fusion()
    on_vs_off(ctx, dimg, masks, expect)


@pytest.fixture(scope='module')
def wide(dev):
    sd = synthetic.resnet_state_dict('resnet101', seed=5, width=64, prefix=PREFIX)
    c = hip.Context(hip.make_dims(sd, 10, blocks=synthetic.RESNET_BLOCKS['resnet101']), sd, dev)
    images, masks = synthetic.exemplars(1, k=14, size=224, seed=31, zero_every=0)
    which = [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 0, 0, 2, 3]
    images = images[0][which].contiguous()
    masks = masks[0].clone()
    # slots 0 and 4 show the same image under DISJOINT masks: the union box and the union
    # tail sets are strictly larger than either member's
    masks[0] = 0; masks[0, 0, 8:70, 12:80] = 1
    masks[4] = 0; masks[4, 0, 150:215, 130:220] = 1
    masks[9] = 0          # an empty slot of a live class
    yield c, images.cuda(), masks.cuda()
    c.close()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_sharing_changes_no_bit_full_width_kernels(wide, precision):
    """ResNet-101 at width 64 and 224 x 224, where the hand-scheduled kernels run: 14 slots
    built from 4 distinct images."""
    c, images, masks = wide
    assert live_classes(images, masks) == 4
    c.set_precision(precision)
    for sparse_tail in (True, False):
        for skip_empty in (True, False):
            c.set_fusion(sparse_tail=sparse_tail, skip_empty=skip_empty)
            got = on_vs_off(c, images, masks, 4)
            assert (got[9] == 0).all() and got[[0, 4]].abs().amax(dim=1).min() > 0
            assert not torch.equal(got[0], got[4])
    c.set_fusion()


@pytest.mark.parametrize('pattern', ['pairs', 'near_duplicate'])
def test_hash_collisions_never_merge_different_images(dev, base, pattern, monkeypatch):
    """MILAN_SHARE_HASH_BITS=0 (read when the context is created): every hash is equal, every
    pair of slots goes through the byte comparison -- the same bits and the same counts."""
    monkeypatch.setenv('MILAN_SHARE_HASH_BITS', '0')
    c = small_ctx(dev)
    try:
        images, masks = make(pattern, base)
        c.set_precision('split_f16')
        on_vs_off(c, images, masks, EXPECT[pattern])
    finally:
        c.close()


def test_shared_pass_matches_the_oracle(ctx, base):
    """... so the suite does not only compare the library with itself."""
    images, masks = make('pairs', base)
    with torch.no_grad():
        ref = O.encode(O.byte_to_float(images.reshape(4, 3, 3, 64, 64)),
                       masks.reshape(4, 3, 1, 64, 64).float(), ctx.sd, blocks=BLOCKS)
    ref = ref.reshape(12, -1)
    ctx.set_precision('split_f16')
    ctx.set_fusion()
    ctx.set_image_sharing(True)
    try:
        got = ctx.encode(images, masks).cpu()
    finally:
        ctx.set_image_sharing(False)
    e, where = feature_error(got, ref)
    assert e <= FEATURE_CLASS, (e, where)


def test_shared_encode_enqueues_without_synchronising(ctx, base):
    """The whole shared pass -- hash, classes, compaction, counters included -- is captured
    into a graph (a capture fails on any synchronisation or read-back); the class structure
    is data, not a launch parameter."""
    images, masks = make('pairs', base)
    images, masks = images.cuda(), masks.cuda()
    ctx.set_precision('split_f16')
    ctx.set_fusion()
    ctx.set_image_sharing(False)
    want = ctx.encode(images, masks, check=False).clone()   # (also sizes the workspace)
    ctx.set_image_sharing(True)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            ctx.encode(images, masks, check=False)
            with torch.cuda.graph(graph, stream=side):
                out = ctx.encode(images, masks, check=False)
        torch.cuda.current_stream().wait_stream(side)
        ctx.image_sharing_stats(clear=True)
        for replay in range(3):
            out.fill_(float(replay + 5))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), replay
        assert ctx.image_sharing_stats(clear=True) == (36, 27) and ctx.status() == 0
        # another duplicate pattern (and an empty mask) in the SAME buffers, the same graph
        other, other_masks = make('root_mask_empty', base)
        other[1] = other[0]; other[10] = other[9]
        images.copy_(other)
        masks.copy_(other_masks)
        graph.replay()
        torch.cuda.synchronize()
        assert ctx.image_sharing_stats(clear=True) == (12, 9)
    finally:
        ctx.set_image_sharing(False)
    again = ctx.encode(images, masks, check=False)
    assert torch.equal(out, again)
    assert (out[2] == 0).all()


def test_float_images_and_missing_masks(ctx, base):
    """Float images may carry NaN pixels: they take the full pass whatever the flag says
    (trunk_images == slots) and a NaN pixel under a zero mask still yields a NaN row.
    masks=None with duplicates: shared, one trunk image per distinct image."""
    images, masks = make('pairs', base)
    ctx.set_precision('split_f16')
    ctx.set_fusion()
    x = O.byte_to_float(images[:3]).clone()
    m = masks[:3].clone()
    x[2] = x[0]
    m[1] = 0
    x[1, 0, 3, 3] = float('nan')
    ctx.set_image_sharing(True)
    try:
        ctx.image_sharing_stats(clear=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got = ctx.encode(x, m).cpu()
        assert ctx.image_sharing_stats(clear=True) == (3, 3)
        assert torch.isnan(got[1]).all() and torch.isfinite(got[[0, 2]]).all()
    finally:
        ctx.set_image_sharing(False)
        ctx.status()
    assert live_classes(images, None) == 9
    on_vs_off(ctx, images, None, 9)


NV = 60


@pytest.fixture(scope='module')
def model(dev):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(NV)), None, True, True, True, True, 15)
    enc = encoders.PyramidConvEncoder('resnet50', width=16, pretrained=False)
    lm = lms.LanguageModel(idx, 16, 64)
    dec = decoders.Decoder(idx, enc, lm, embedding_size=16, hidden_size=64, length=10,
                           beam_size=4)
    sd = synthetic.milan_state_dict(NV + 4, 'resnet50', seed=11, width=16, hidden_size=64,
                                    embedding_size=16, lm_hidden_size=64, lm_embedding_size=16)
    dec.load_state_dict(sd, strict=True)
    return dec.to('cuda')


@pytest.mark.parametrize('strategy', ['greedy', 'rerank'])
def test_decoder_end_to_end(model, strategy):
    """8 neurons x k = 3 with images repeated across neurons: captions, tokens and scores do
    not depend on `share_images`, and DecoderOutput keeps its fields."""
    dec = model
    assert dec.share_images is False
    images, masks = synthetic.exemplars(8, k=3, size=64, seed=41, zero_every=0)
    images = images.clone()
    images[1, 0] = images[0, 0]; images[5, 2] = images[0, 0]; images[7, 1] = images[3, 1]
    samples = [(0, 0, images[i], masks[i]) for i in range(8)]
    off = dec.predict(samples, batch_size=4, display_progress_as=None, strategy=strategy)
    on = dec.predict(samples, batch_size=4, display_progress_as=None, strategy=strategy,
                     share_images=True)
    assert dec.share_images is False and on == off and len(on) == 8
    slots, trunk = dec._ctx.image_sharing_stats(clear=True)
    assert (slots, trunk) == (24, 21)
    a = dec(images, masks, strategy=strategy)
    dec.share_images = True
    try:
        b = dec(images, masks, strategy=strategy)
    finally:
        dec.share_images = False
    assert dec._ctx.image_sharing_stats(clear=True) == (24, 21)
    assert isinstance(b, milan_amd.DecoderOutput) and b._fields == a._fields
    assert b.captions == a.captions
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.scores, b.scores)
    assert 'share_images' not in dec.properties()


SUB_SCRIPT = r'''
import sys
sys.path[:0] = [{repo!r}, {pkg!r}]
import torch
from milan_amd import hip, synthetic
PREFIX = 'encoder.encoder.model.'
blocks = synthetic.RESNET_BLOCKS['resnet50']
sd = synthetic.resnet_state_dict('resnet50', seed=13, width=16, prefix=PREFIX)
c = hip.Context(hip.make_dims(sd, 10, blocks=blocks), sd, hip.require_device('cuda'))
images, masks = synthetic.exemplars(4, k=3, size=64, seed=17, zero_every=0)
images = images.reshape(12, 3, 64, 64).clone()
masks = masks.reshape(12, 1, 64, 64).clone()
# passes of 5: slots 0-4, 5-9, 10-11.  Inside a pass: 3 <- 0, 8 <- 6, 11 <- 10; across
# passes (NOT shared): 7 <- 0, 10 <- 5; slot 9 is empty
images[3] = images[0]; images[8] = images[6]; images[7] = images[0]
images[10] = images[5]; images[11] = images[10]
masks[9] = 0
c.set_precision('split_f16')
want = c.encode(images, masks).cpu()
c.set_image_sharing(True)
got = c.encode(images, masks).cpu()
print('EQUAL', bool(torch.equal(got, want)), 'STATS', *c.image_sharing_stats())
c.close()
'''


def test_sub_batches_share_within_a_pass_only(tmp_path):
    """MILAN_ENC_SUB is cached per process: one fresh child with passes of 5 images, with
    duplicates inside and across the passes.  Live classes per pass: 4 + 3 + 1."""
    script = tmp_path / 'sub.py'
    script.write_text(SUB_SCRIPT.format(repo=str(REPO), pkg=str(REPO / 'neuron-descriptions_amd')))
    env = dict(os.environ, MILAN_ENC_SUB='5')
    env.pop('MILAN_SHARE_IMAGES', None)
    out = subprocess.run(['timeout', '-k', '10', '120', sys.executable, str(script)], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'EQUAL True STATS 12 8' in out.stdout, out.stdout
