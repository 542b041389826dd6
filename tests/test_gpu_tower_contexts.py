"""What `hip.ClipContext`, `hip.BertContext` and `hip.VitContext` have in common (the weight
store of csrc/tower.hip and `hip._TowerContext`): the errors of a bad state dict name the tower
and the tensor, fail before any launch and leave the library usable; entries that are not
floating point are skipped; `close()` may be called twice; the workspace only grows.

Every comparison is bit for bit (`torch.equal`): the same context class on the same inputs.
Each tower runs at its smallest stand-in configuration.
"""
import pathlib
import re
import sys

import pytest
import torch

import vitref
from milan_amd import bertscore, hip, rerankers

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import bert_standin  # noqa: E402
import clip_standin  # noqa: E402

DEVICE = torch.device('cuda:0')


class Clip:
    name, context = 'clip', hip.ClipContext
    block_key = 'visual.transformer.resblocks.1.mlp.c_fc.weight'

    def __init__(self):
        clip_standin.configure(seed=0)
        d = clip_standin.DEFAULTS
        self.weights = {k: v for k, v in clip_standin.load()[0].state_dict().items()
                        if v.dtype.is_floating_point}
        self.dims = rerankers.infer_dims(self.weights, d['vision_heads'], d['text_heads'])
        g = torch.Generator().manual_seed(1)
        res = self.dims['resolution']
        self.images = torch.randn(3, 3, res, res, generator=g)
        self.masks = torch.rand(3, 1, res, res, generator=g)
        self.tokens = torch.randint(1, self.dims['vocab_size'],
                                    (3, self.dims['context_length']), generator=g)

    def make_dims(self):
        return hip.ClipDims(**self.dims)

    def run(self, ctx, n):
        return [ctx.encode_images(self.images[:n], self.masks[:n], 0b1, True),
                ctx.encode_texts(self.tokens[:n], self.dims['context_length'])]


class Bert:
    name, context = 'bert', hip.BertContext
    block_key = 'encoder.layer.0.attention.self.query.weight'
    lengths = (5, 9, 7)

    def __init__(self):
        cfg = dict(bert_standin.CONFIGS['bert'], layers=1, num_layers=1)
        sd = bert_standin.state_dict(cfg, 5)
        self.dims = bertscore.infer_dims(sd, heads=cfg['heads'])
        self.weights = {k: v for k, v in bertscore.strip_prefix(sd)[0].items()
                        if not k.startswith('pooler.')}
        g = torch.Generator().manual_seed(2)
        self.ids = torch.randint(0, self.dims['vocab_size'], (sum(self.lengths),), generator=g)

    def make_dims(self):
        return hip.BertDims(**self.dims)

    def run(self, ctx, n):
        bounds = [sum(self.lengths[:i]) for i in range(n + 1)]
        ids = self.ids[:bounds[-1]].to(DEVICE)
        offsets = torch.tensor(bounds, dtype=torch.int32, device=DEVICE)
        return [ctx.encode(ids, offsets, max(self.lengths[:n]))]


class Vit:
    name, context = 'vit', hip.VitContext
    block_key = 'blocks.1.mlp.fc1.weight'

    def __init__(self):
        self.d = vitref.make_dims(16, 8, 32, 2, 2, 64)
        self.weights = vitref.cast(vitref.weights(self.d, seed=3), torch.float32)
        self.images = vitref.images(self.d, 3, seed=4).float()

    def make_dims(self):
        d = self.d
        return hip.VitDims(resolution=d['res'], patch=d['patch'], width=d['width'],
                           layers=d['depth'], heads=d['heads'], hidden=d['hidden'],
                           eps=vitref.EPS)

    def run(self, ctx, n):
        taps, cls = ctx.run(self.images[:n], range(self.d['depth']), True)
        return [taps[t] for t in sorted(taps)] + [cls]


TOWERS = {'clip': Clip, 'bert': Bert, 'vit': Vit}


@pytest.fixture(params=list(TOWERS))
def tower(request):
    return TOWERS[request.param]()


def build(tower, weights=None):
    return tower.context(tower.make_dims(), tower.weights if weights is None else weights,
                         DEVICE)


def results(tower, weights=None, n=2):
    ctx = build(tower, weights)
    out = [t.clone() for t in tower.run(ctx, n)]
    ctx.close()
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_missing_weight_is_named_and_the_next_context_works(tower):
    before = results(tower)
    weights = {k: v for k, v in tower.weights.items() if k != tower.block_key}
    with pytest.raises(RuntimeError) as error:
        build(tower, weights)
    text = str(error.value)
    assert f'{tower.name}: weight {tower.block_key} was not uploaded' in text
    assert same(results(tower), before)


def test_a_wrong_element_count_is_named_and_the_next_context_works(tower):
    before = results(tower)
    need = tower.weights[tower.block_key].numel()
    weights = dict(tower.weights)
    weights[tower.block_key] = torch.zeros(need + 3)
    with pytest.raises(RuntimeError) as error:
        build(tower, weights)
    text = str(error.value)
    assert re.search(rf'{tower.name}: weight {re.escape(tower.block_key)} '
                     rf'has {need + 3} elements, the dims need {need}\b', text), text
    assert same(results(tower), before)


def test_an_integer_entry_is_ignored(tower):
    weights = dict(tower.weights)
    weights['position_ids'] = torch.arange(12, dtype=torch.int64)
    assert same(results(tower, weights), results(tower))


def test_close_twice_and_a_workspace_that_only_grows(tower):
    ctx = build(tower)
    small = [t.clone() for t in tower.run(ctx, 1)]
    bytes_small = ctx._ws.numel()
    large = [t.clone() for t in tower.run(ctx, 3)]
    pointer, bytes_large = ctx._ws.data_ptr(), ctx._ws.numel()
    assert bytes_large > bytes_small
    again = tower.run(ctx, 1)
    assert ctx._ws.data_ptr() == pointer and ctx._ws.numel() == bytes_large
    assert same(again, small)
    assert same(tower.run(ctx, 3), large)
    ctx.close()
    ctx.close()
    assert ctx._ws is None
