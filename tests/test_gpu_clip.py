"""The CLIP reranker in HIP against the reference's goldens and, where no golden
exists, against tests/clipref.py in float64.

Tolerance (tests/golden/reference_goldens_clip.json): bound = 4 x the fp32
reference's own error against float64, 4 x 4.71e-7 = 1.89e-6 on similarities
and rerank scores (cosines, |x| <= k).  Measured on an MI355X: see
`hip_max_abs_error` in the json and DESIGN.md 4.14.  For the fuzz cases, which
have their own dims, the bound is 4 x the error of clipref in fp32 against
clipref in float64 on that same case.  Orders are compared only across adjacent
pairs whose float64 gap exceeds 2 x bound; `test_order_skips_stay_within_two_percent`
runs every case (cached) and asserts that at most 2 % of all adjacent pairs
were skipped that way.
"""
import functools
import json
import pathlib
import sys

import pytest
import torch

import clipref
from milan_amd import rerankers

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import clip_standin  # noqa: E402

META = json.loads((GOLDEN / 'reference_goldens_clip.json').read_text())
TENSORS = torch.load(GOLDEN / 'reference_goldens_clip.pt', weights_only=True)
BOUND = META['tolerance']['bound']


def check_order(order, scores64, bound):
    """`order` sorts the float64 scores descending, up to gaps <= 2 x bound.
    Returns (adjacent pairs, pairs skipped because their gap is within 2 x bound)."""
    s = scores64[list(order)]
    assert sorted(order) == list(range(len(order)))
    gaps = s[:-1] - s[1:]
    assert bool((gaps > -2 * bound).all())
    return len(gaps), int((gaps.abs() <= 2 * bound).sum())


def build(case_or_dims, weights, **kwargs):
    return rerankers.reranker(weights=weights, tokenize=clip_standin.tokenize,
                              vision_heads=case_or_dims['vision_heads'],
                              text_heads=case_or_dims['text_heads'], **kwargs)


@pytest.mark.parametrize('index', range(len(META['cases'])),
                         ids=[c['key'] for c in META['cases']])
def test_golden_case(index):
    run_golden(index)


@functools.lru_cache(maxsize=None)
def run_golden(index):
    case = META['cases'][index]
    pairs = skipped = 0
    dims = META['configs'][case['config']]
    clip_standin.configure(**{k: v for k, v in dims.items()})
    gold = TENSORS[case['key']]
    images, masks, texts = clipref.synthetic_inputs(dims, case['neurons'], case['k'],
                                                    case['candidates'], case['masks'],
                                                    case['seed'])
    r = build(dims, TENSORS['weights/' + case['config']], lam=.125,
              mask_layers=case['mask_layers'])
    sims = r.clip_with_masks(images[0].cuda(), texts[0], masks=masks[0].cuda()).cpu()
    err = (sims.double() - gold['sims64']).abs().max().item()
    out = r(images.cuda(), masks.cuda(), texts, lam=case['lam'])
    assert isinstance(out, rerankers.RerankerOutput)
    for n in range(case['neurons']):
        got = torch.empty(len(out.orders[n]), dtype=torch.float64)
        got[list(out.orders[n])] = torch.tensor(out.scores[n], dtype=torch.float64)
        err = max(err, (got - gold['scores64'][n]).abs().max().item())
        p, k = check_order(out.orders[n], gold['scores64'][n], BOUND)
        pairs, skipped = pairs + p, skipped + k
        assert out.texts[n] == tuple(texts[n][i] for i in out.orders[n])
        assert list(out.scores[n]) == sorted(out.scores[n], reverse=True)
    print(case['key'], 'hip max |err| vs float64', err, 'bound', BOUND)
    assert err <= BOUND
    assert (sims - gold['sims']).abs().max() <= 2 * BOUND  # fp32 reference itself
    # token ids in place of texts, and the same bits twice
    again = r(images.cuda(), masks.cuda(), gold['tokens'], lam=case['lam'])
    assert again.scores == out.scores and again.orders == out.orders
    return pairs, skipped


def random_tokens(g, rows, dims, longest=None):
    ctx, vocab = dims['context_length'], dims['vocab_size']
    t = torch.zeros(rows, ctx, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(1, (longest or ctx - 2) + 1, (1,), generator=g))
        t[r, 0] = vocab - 2
        t[r, 1:1 + n] = torch.randint(1, vocab - 2, (n,), generator=g)
        t[r, 1 + n] = vocab - 1
    return t


FUZZ = [
    dict(resolution=40, patch=8, vision_width=36, vision_layers=2, vision_heads=3,
         embed_dim=20, context_length=12, vocab_size=50, text_width=28, text_layers=1,
         text_heads=7),
    dict(resolution=42, patch=14, vision_width=66, vision_layers=3, vision_heads=2,
         embed_dim=33, context_length=30, vocab_size=70, text_width=34, text_layers=2,
         text_heads=2),
    dict(resolution=96, patch=32, vision_width=128, vision_layers=1, vision_heads=2,
         embed_dim=64, context_length=77, vocab_size=90, text_width=64, text_layers=2,
         text_heads=1),
    # a 9 x 9 grid (82 image tokens: more keys than one wave) and, on the text side, head
    # size 72 (more columns than one wave); both at once would not fit 64 KiB of LDS
    dict(resolution=72, patch=8, vision_width=80, vision_layers=2, vision_heads=2,
         embed_dim=48, context_length=40, vocab_size=90, text_width=144, text_layers=1,
         text_heads=2),
    # the true ViT-B/32
    dict(resolution=224, patch=32, vision_width=768, vision_layers=12, vision_heads=12,
         embed_dim=512, context_length=77, vocab_size=600, text_width=512, text_layers=12,
         text_heads=8),
]


@pytest.mark.parametrize('index', range(len(FUZZ)))
def test_fuzz_against_float64(index):
    run_fuzz(index)


@functools.lru_cache(maxsize=None)
def run_fuzz(index):
    dims = FUZZ[index]
    g = torch.Generator().manual_seed(100 + index)
    clip_standin.configure(seed=100 + index, **dims)
    sd = clip_standin.load()[0].state_dict()
    big = dims['vision_width'] == 768
    neurons, k = (1, 2) if big else (3, 1 + index)
    counts = [5] if big else [int(c) for c in torch.randint(1, 12, (neurons,), generator=g)]
    res = dims['resolution']
    images = torch.randn(neurons, k, 3, res, res, generator=g)
    masks = torch.rand(neurons, k, 1, res, res, generator=g)
    tokens = [random_tokens(g, c, dims, 17 if big else None) for c in counts]
    layers = None if index % 2 else tuple(range(0, dims['vision_layers'], 2))
    lam = (.5, 0., 1., .7, .3)[index]
    vh, th = dims['vision_heads'], dims['text_heads']
    want = clipref.rerank_scores(clipref.cast(sd, torch.float64), vh, th, images, masks,
                                 tokens, lam, layers)
    ref32 = clipref.rerank_scores(sd, vh, th, images, masks, tokens, lam, layers)
    ref_err = max((a.double() - b).abs().max().item() for a, b in zip(ref32, want))
    bound = 4 * ref_err
    r = build(dims, sd, mask_layers=layers)
    got = r.similarities(images.cuda(), masks.cuda(), tokens, lam=lam)
    err = max((a.cpu().double() - b).abs().max().item() for a, b in zip(got, want))
    print(dims, 'hip err', err, 'fp32 ref err', ref_err, 'bound', bound)
    assert err <= bound
    out = r(images.cuda(), masks.cuda(), tokens, lam=lam)
    pairs = skipped = 0
    for order, scores in zip(out.orders, want):
        p, k = check_order(order, scores, bound)
        pairs, skipped = pairs + p, skipped + k
    return pairs, skipped


def test_order_skips_stay_within_two_percent():
    """Over the whole test set, goldens and fuzz: at most 2 % of the adjacent pairs may be
    left uncompared because their float64 gap is within twice the bound."""
    counts = [run_golden(i) for i in range(len(META['cases']))]
    counts += [run_fuzz(i) for i in range(len(FUZZ))]
    pairs, skipped = (sum(c[i] for c in counts) for i in (0, 1))
    print('adjacent pairs', pairs, 'skipped', skipped)
    assert pairs > 100 and skipped <= .02 * pairs


def test_causal_truncation_changes_nothing_beyond_rounding():
    dims = FUZZ[2]
    g = torch.Generator().manual_seed(7)
    clip_standin.configure(seed=7, **dims)
    sd = clip_standin.load()[0].state_dict()
    tokens = random_tokens(g, 9, dims, longest=10)
    want = clipref.encode_texts(clipref.cast(sd, torch.float64), dims['text_heads'], tokens)
    ref_err = (clipref.encode_texts(sd, dims['text_heads'], tokens).double() - want).abs().max()
    bound = 4 * float(ref_err)
    model = build(dims, sd).clip_with_masks
    cut = model.encode_texts(tokens).cpu().double()
    model.truncate_text = False
    full = model.encode_texts(tokens).cpu().double()
    print('truncated err', (cut - want).abs().max().item(), 'full err',
          (full - want).abs().max().item(), 'bound', bound)
    assert (cut - want).abs().max() <= bound and (full - want).abs().max() <= bound


def test_errors_on_the_gpu():
    dims = META['configs']['small']
    model = build(dims, TENSORS['weights/small'])
    with pytest.raises(RuntimeError, match='must match'):
        model.clip_with_masks(torch.zeros(2, 3, 80, 80).cuda(), ['a dog'])
    with pytest.raises(ValueError):
        model(torch.zeros(2, 1, 3, 64, 64).cuda(), torch.zeros(1, 1, 1, 64, 64).cuda(), [[], []])


def golden_decoder():
    from milan_amd import decoders, encoders, lang, synthetic
    case = META['decoder']
    dims = META['configs'][case['config']]
    clip_standin.configure(**dims)

    class PoolEncoder(encoders.Encoder):

        def __init__(self):
            super().__init__()
            self.feature_shape = (clipref.POOL_FEATURES,)

        def forward(self, images, masks=None, **_):
            return clipref.pool_features(images, masks)

        def properties(self):
            return {}

    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(case['nvocab'])), None, True, True,
                       True, True, case['length'])
    model = decoders.DecoderWithCLIP(
        idx, PoolEncoder(), embedding_size=case['emb'], hidden_size=case['hidden'],
        length=case['length'], beam_size=case['beam'],
        reranker_kwargs=dict(weights=TENSORS['weights/' + case['config']],
                             tokenize=clip_standin.tokenize, lam=case['lam'],
                             vision_heads=dims['vision_heads'],
                             text_heads=dims['text_heads']))
    sd = synthetic.decoder_state_dict(len(idx), feature_size=clipref.POOL_FEATURES,
                                      hidden_size=case['hidden'], embedding_size=case['emb'],
                                      lm=False, seed=case['weight_seed'])
    result = model.load_state_dict(sd, strict=False)
    assert not result.unexpected_keys and not result.missing_keys, result
    model.precision = 'f32'  # the reference's arithmetic
    images, masks, _ = clipref.synthetic_inputs(dims, case['neurons'], case['k'],
                                                [1] * case['neurons'], 'random',
                                                case['input_seed'])
    return model.to('cuda'), images, masks, case


def test_decoder_with_clip_forward_matches_the_reference_end_to_end():
    """G19: DecoderOutput of the reference's DecoderWithCLIP.forward.  Tokens and captions
    are compared exactly, log-probability scores within the beam goldens' tolerance
    (rtol 1e-4, atol 2e-3: the smoke test's bound for fp32 beam scores)."""
    from milan_amd import decoders
    model, images, masks, case = golden_decoder()
    gold = TENSORS['decoder']
    with pytest.raises(ValueError, match='masks'):
        model(images.cuda())
    with pytest.raises(ValueError, match='strategy'):
        model(images.cuda(), masks.cuda(), strategy='beam')
    out = model(images.cuda(), masks.cuda())
    assert isinstance(out, decoders.DecoderOutput)
    assert list(out.captions) == case['captions']
    assert torch.equal(out.tokens.cpu(), gold['tokens'])
    torch.testing.assert_close(out.scores.cpu(), gold['scores'], rtol=1e-4, atol=2e-3)
    assert torch.equal(out.beam_tokens.cpu(), gold['beam_tokens'])
    torch.testing.assert_close(out.beam_scores.cpu(), gold['beam_scores'], rtol=1e-4,
                               atol=2e-3)
    assert [list(c) for c in out.beam_captions] == case['beam_captions']
    assert out.predictions is None and out.attentions is None
    for n, choice in enumerate(case['choice']):
        assert torch.equal(out.tokens[n], out.beam_tokens[n, choice])
        assert torch.equal(out.scores[n], out.beam_scores[n, choice])
    assert any(case['choice'])  # the reranker changed the beam search's own pick
    again = model(images.cuda(), masks.cuda())
    assert again.captions == out.captions and torch.equal(again.scores, out.scores)
    with pytest.raises(ValueError, match='beam_size='):
        model(images.cuda(), masks.cuda(), beam_size=1000)


def test_decoder_with_clip_predict_on_the_synthetic_dataset(tmp_path):
    """predict: the memory-mapped uint8 path (chunks of neurons, group_size), the generic
    sample path (floats in [0, 1]) and forward group by group give the same captions; the
    captions are those clipref ranks first among the beam."""
    import numpy
    from milan_amd import datasets, decoders, encoders, lang, synthetic
    dims = META['configs']['small']
    clip_standin.configure(**dims)
    weights = TENSORS['weights/small']
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(12)), None, True, True, True, True, 15)
    enc = encoders.PyramidConvEncoder('resnet50', width=8, pretrained=False)
    torch.manual_seed(3)
    model = decoders.DecoderWithCLIP(
        idx, enc, embedding_size=4, hidden_size=8, length=6, beam_size=5,
        reranker_kwargs=dict(weights=weights, tokenize=clip_standin.tokenize, lam=.5,
                             vision_heads=dims['vision_heads'],
                             text_heads=dims['text_heads']))
    model.reset_parameters()
    model.precision = 'f32'
    images, masks = synthetic.exemplars(7, k=2, size=64, seed=5)
    (tmp_path / 'conv5').mkdir()
    numpy.save(tmp_path / 'conv5' / 'images.npy', images.numpy())
    numpy.save(tmp_path / 'conv5' / 'masks.npy', masks.numpy())
    ds = datasets.TopImagesDataset(tmp_path)
    got = model.predict(ds, batch_size=3, display_progress_as=None, device='cuda')
    assert isinstance(got, tuple) and len(got) == 7
    samples = [ds[i] for i in range(len(ds))]
    assert samples[0][2].dtype == torch.float32 and float(samples[0][2].max()) <= 1.
    assert model.predict(samples, batch_size=3, display_progress_as=None) == got
    floats = images.float().mul(torch.tensor(1. / 255., dtype=torch.float64).float())
    w64 = clipref.cast(weights, torch.float64)
    for lo in range(0, 7, 3):
        im, mk = images[lo:lo + 3].cuda(), masks[lo:lo + 3].cuda()
        out = model(im, mk, group_size=3)
        assert out.captions == got[lo:lo + 3]
        plain = decoders.Decoder.forward(model, im, mk, strategy='beam', group_size=3)
        assert torch.equal(out.beam_tokens, plain.beam_tokens)
        texts = [list(c) for c in plain.beam_captions]
        tokens = [clip_standin.tokenize(t) for t in texts]
        want = clipref.rerank_scores(w64, dims['vision_heads'], dims['text_heads'],
                                     floats[lo:lo + 3], masks[lo:lo + 3].float(), tokens, .5)
        for n, scores in enumerate(want):
            best = texts[n].index(out.captions[n])
            assert scores[best] >= scores.max() - 2 * BOUND
