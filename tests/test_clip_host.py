"""Host side of the CLIP reranker: dims inference, error types, DecoderWithCLIP
arguments, properties and the serialise round trip (no GPU)."""
import io
import json
import pathlib
import sys

import pytest
import torch

from milan_amd import decoders, encoders, lang, rerankers, synthetic
import milan_amd

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import clip_standin  # noqa: E402

META = json.loads((GOLDEN / 'reference_goldens_clip.json').read_text())
TENSORS = torch.load(GOLDEN / 'reference_goldens_clip.pt', weights_only=True)
DIMS = {k: v for k, v in META['configs']['odd'].items() if k != 'seed'}
WEIGHTS = TENSORS['weights/odd']
HEADS = dict(vision_heads=DIMS['vision_heads'], text_heads=DIMS['text_heads'])


class IdentityEncoder(torch.nn.Module):

    def __init__(self, size):
        super().__init__()
        self.feature_shape = (size,)

    def properties(self):
        return {'feature_size': self.feature_shape[0]}


def corpus():
    rows = [[None, None, None, None, [f'a {w} thing', f'the {w}']]
            for w in ('dog', 'sky', 'tree')]
    return rows


def test_dims_are_inferred_from_the_state_dict():
    assert rerankers.infer_dims(WEIGHTS, **HEADS) == DIMS
    model = rerankers.CLIPWithMasks(weights=WEIGHTS, **HEADS)
    grid = DIMS['resolution'] // DIMS['patch']
    assert model.input_resolution == DIMS['resolution']
    assert model.num_patches == grid * grid and model.num_patches_xy == grid
    assert model.mask_layers == tuple(range(DIMS['vision_layers']))
    assert all(v.dtype == torch.float32 for v in model.weights.values())


def test_true_vit_b32_dims_from_shapes_alone():
    clip_standin.configure(resolution=224, patch=32, vision_width=128, vision_layers=1,
                           vision_heads=2, embed_dim=64, context_length=77, vocab_size=100,
                           text_width=64, text_layers=1, text_heads=1)
    sd = clip_standin.load()[0].half().state_dict()
    dims = rerankers.infer_dims(sd)
    assert (dims['resolution'], dims['patch'], dims['vision_heads'], dims['text_heads'],
            dims['context_length']) == (224, 32, 2, 1, 77)
    model = rerankers.CLIPWithMasks(weights=sd)  # fp16 state dicts are converted
    assert model.weights['visual.proj'].dtype == torch.float32


def test_state_dict_path_and_error_types(tmp_path):
    torch.save(dict(WEIGHTS), tmp_path / 'clip.pt')
    model = rerankers.CLIPWithMasks(weights=tmp_path / 'clip.pt', **HEADS)
    assert model.dims == DIMS
    with pytest.raises(ValueError, match='ResNet'):
        rerankers.CLIPWithMasks(weights={'visual.layer1.0.conv1.weight': torch.zeros(1)})
    with pytest.raises(ValueError):
        rerankers.CLIPWithMasks(weights=WEIGHTS, source_mean=(0., 0., 0.), **HEADS)
    with pytest.raises(ValueError, match='heads'):
        rerankers.infer_dims(WEIGHTS)  # width 30 // 64 = 0 heads
    with pytest.raises(ImportError, match='weights='):
        rerankers.CLIPWithMasks()  # no `clip` package here
    with pytest.raises(NotImplementedError, match='tokenize='):
        model.tokens(['a dog'])
    ids = model.tokens(torch.zeros(2, DIMS['context_length'], dtype=torch.long))
    assert ids.shape == (2, DIMS['context_length'])
    with pytest.raises(ValueError):
        model.tokens(torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(RuntimeError, match='must match'):
        model._check_images(torch.zeros(1, 3, 80, 80), True, True)
    model._check_images(torch.zeros(1, 3, DIMS['resolution'], DIMS['resolution']), True, True)


def test_reranker_factory_defaults_and_batch_errors():
    r = rerankers.reranker(weights=WEIGHTS, **HEADS)
    assert r.lam == 1. and isinstance(r, rerankers.CLIPWithMasksReranker)
    assert rerankers.CLIPWithMasksReranker(r.clip_with_masks).lam == .5
    res = DIMS['resolution']
    with pytest.raises(ValueError, match='masks batch'):
        r(torch.zeros(2, 1, 3, res, res), torch.zeros(1, 1, 1, res, res), [[], []])
    with pytest.raises(ValueError, match='texts batch'):
        r(torch.zeros(2, 1, 3, res, res), torch.zeros(2, 1, 1, res, res), [[]])
    assert rerankers.RerankerOutput._fields == ('texts', 'orders', 'scores')
    assert milan_amd.DecoderWithCLIP is decoders.DecoderWithCLIP


def tokenize(texts):
    if isinstance(texts, str):
        return tuple(texts.lower().split())
    return tuple(tuple(t.lower().split()) for t in texts)


def make(**kwargs):
    kw = dict(weights=WEIGHTS, **HEADS)
    return decoders.decoder(corpus(), IdentityEncoder(12), rerank_with_clip=True,
                            indexer_kwargs=dict(tokenize=tokenize), embedding_size=8,
                            hidden_size=16, reranker_kwargs=kw, **kwargs)


def test_decoder_factory_returns_a_decoder_with_clip():
    model = make()
    assert isinstance(model, decoders.DecoderWithCLIP)
    assert (model.strategy, model.beam_size, model.temperature) == ('beam', 1000, .5)
    props = model.properties()
    assert props['beam_size'] == 1000
    assert props['reranker_kwargs'] == dict(name='ViT-B/32', jit=False, device='cpu', **HEADS)
    with pytest.raises(ValueError, match='masks'):
        model(torch.zeros(1, 1, 3, 48, 48))
    with pytest.raises(ValueError, match='strategy'):
        model(torch.zeros(1, 1, 3, 48, 48), torch.zeros(1, 1, 1, 48, 48), strategy='greedy')


def test_serialize_round_trip_and_from_decoder():
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(12)), None, True, True, True, True, 15)
    enc = encoders.PyramidConvEncoder('resnet50', width=8, pretrained=False)
    model = decoders.DecoderWithCLIP(idx, enc, embedding_size=4, hidden_size=8, length=7,
                                     reranker_kwargs=dict(weights=WEIGHTS, **HEADS))
    buffer = io.BytesIO()
    model.save(buffer)
    buffer.seek(0)
    payload = torch.load(buffer, weights_only=False)
    # CLIP's tensors travel under the reference's names (wrapped visual attention)
    prefix = rerankers.REFERENCE_PREFIX
    assert prefix + 'visual.transformer.resblocks.0.attn.qkv.weight' in payload['state_dict']
    assert prefix + 'transformer.resblocks.0.attn.in_proj_weight' in payload['state_dict']
    buffer.seek(0)
    for cls in (decoders.Decoder, decoders.DecoderWithCLIP):
        buffer.seek(0)
        again = cls.load(buffer)
        assert isinstance(again, decoders.DecoderWithCLIP) and again.length == 7
        assert again.properties()['reranker_kwargs'] == model.properties()['reranker_kwargs']
        for key, value in model.reranker.clip_with_masks.weights.items():
            assert torch.equal(again.reranker.clip_with_masks.weights[key], value), key
        for key, value in model.state_dict().items():
            assert torch.equal(again.state_dict()[key], value), key
    base = decoders.Decoder(idx, enc, embedding_size=4, hidden_size=8)
    with pytest.raises(ImportError):
        decoders.DecoderWithCLIP.from_decoder(base)
    converted = decoders.DecoderWithCLIP.from_decoder(
        base, reranker_kwargs=dict(weights=WEIGHTS, **HEADS))
    assert isinstance(converted, decoders.DecoderWithCLIP)
    assert torch.equal(converted.state_dict()['lstm.weight_hh'], base.state_dict()['lstm.weight_hh'])
