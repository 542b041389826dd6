"""Host-side pieces of Decoder training (no GPU): the restated corpus BLEU on
hand-worked cases, `decoders.decoder()` against the reference's seeded
initialisation (tests/golden/make_golden_decoder_fit.py), its errors, and the
host restatement of the decoder's dropout mask."""
import json
import math

import pytest
import torch

from conftest import GOLDEN_DIR
from milan_amd import decoders, encoders, lms, metrics
import milan_amd

META = json.loads((GOLDEN_DIR / 'reference_goldens_decoder_fit.json').read_text())


def tokenize(texts):
    if isinstance(texts, str):
        return tuple(texts.lower().split())
    return tuple(tuple(t.lower().split()) for t in texts)


class IdentityEncoder(encoders.Encoder):
    """(N, 1, 1, F) "images" -> (N, F) features (the goldens' stand-in)."""

    def __init__(self, feature_size):
        super().__init__()
        self.feature_shape = (feature_size,)

    def forward(self, images, masks=None, **_):
        return images.reshape(len(images), -1)

    def properties(self):
        return {'feature_size': self.feature_shape[0]}


def corpus_dataset():
    return [('layer', i, None, None, ann) for i, ann in enumerate(META['corpus'])]


# ---- BLEU ------------------------------------------------------------------------
def test_bleu_exact_match_is_100():
    out = metrics.corpus_bleu(['the red dog runs fast'], [['the red dog runs fast']])
    assert out.score == pytest.approx(100.)
    assert out.counts == [5, 4, 3, 2] and out.totals == [5, 4, 3, 2]
    assert out.bp == 1. and out.sys_len == 5 and out.ref_len == 5


def test_bleu_zero_4gram_matches_use_exp_smoothing():
    out = metrics.corpus_bleu(['a b c d'], [['a b c e']])
    assert out.counts == [3, 2, 1, 0] and out.totals == [4, 3, 2, 1]
    # the first order without a match scores 100 / (2 * total)
    assert out.precisions == pytest.approx([75., 200. / 3, 50., 50.])
    assert out.score == pytest.approx((75. * 200. / 3 * 50. * 50.)**.25)


def test_bleu_two_unmatched_orders_halve_again():
    # refs: "the cat" (2 tokens) and "the the dog on mat" (5): closest to 4 is 5
    out = metrics.corpus_bleu(['the the the the'],
                              [['the cat'], ['the the dog on mat']])
    # 'the' x4 clipped to its largest count in one reference (2), 'the the'
    # x3 clipped to 1; 3- and 4-grams unmatched: 100 / (2 * 2), 100 / (4 * 1)
    assert out.counts == [2, 1, 0, 0] and out.totals == [4, 3, 2, 1]
    assert out.precisions == pytest.approx([50., 100. / 3, 25., 25.])
    assert out.ref_len == 5 and out.bp == pytest.approx(math.exp(1 - 5 / 4))
    assert out.score == pytest.approx(
        math.exp(1 - 5 / 4) * (50. * 100. / 3 * 25. * 25.)**.25)


def test_bleu_brevity_penalty():
    out = metrics.corpus_bleu(['a b c d'], [['a b c d e f']])
    assert out.precisions == pytest.approx([100.] * 4)
    assert out.bp == pytest.approx(math.exp(-.5))
    assert out.score == pytest.approx(100. * math.exp(-.5))


def test_bleu_closest_reference_length_ties_to_shorter():
    # 4 tokens, references of 3 and 5: the tie goes to 3, so no brevity penalty
    out = metrics.corpus_bleu(['a b c d'], [['a b c'], ['a b c d e']])
    assert out.ref_len == 3 and out.bp == 1.
    assert out.score == pytest.approx(100.)


def test_bleu_13a_splits_punctuation():
    assert metrics.tokenize_13a('a dog, running. 3.5 x-ray 1-2 "hi"') == \
        'a dog , running . 3.5 x-ray 1 - 2 " hi "'
    assert metrics.tokenize_13a('a&amp;b') == 'a & b'
    out = metrics.corpus_bleu(['dogs, cats and birds'], [['dogs , cats and birds']])
    assert out.score == pytest.approx(100.)


def test_bleu_empty_hypothesis_scores_zero():
    out = metrics.corpus_bleu([''], [['a b c d']])
    assert out.score == 0. and out.bp == 0. and out.sys_len == 0
    assert out.totals == [0, 0, 0, 0]


def test_bleu_preprocesses_and_truncates_references_like_zip():
    dataset = [(0, None, None, None, ['A B C D.', 'x y z w']),
               (1, None, None, None, 'e f g h')]
    got = metrics.bleu(dataset, ['X Y Z W.', ' e f g h'])
    # references transposed with zip: the second annotation of sample 0 is dropped
    want = metrics.corpus_bleu(['x y z w', 'e f g h'], [['a b c d', 'e f g h']])
    assert got == want
    assert got.score < 100.
    both = metrics.corpus_bleu(['x y z w', 'e f g h'],
                               [['a b c d', 'e f g h'], ['x y z w', 'e f g h']])
    assert both.score == pytest.approx(100.)


def test_decoder_bleu_uses_given_predictions():
    dataset = [(0, None, None, None, 'The red dog runs.')]
    out = decoders.Decoder.bleu(None, dataset, predictions=['the red dog runs'])
    assert out.score == pytest.approx(100.)


# ---- decoder() ---------------------------------------------------------------------
def test_decoder_factory_matches_reference_init():
    golden = torch.load(GOLDEN_DIR / 'reference_goldens_decoder_fit.pt')
    dims = {k: v for k, v in META['dims'].items() if k not in ('k', 'F')}
    torch.manual_seed(7)
    model = milan_amd.decoder(corpus_dataset(), IdentityEncoder(META['dims']['F']),
                              indexer_kwargs=dict(tokenize=tokenize), **dims)
    assert isinstance(model, decoders.Decoder)
    assert list(model.indexer.vocab.tokens) == META['tokens']
    assert not model.training
    sd = model.state_dict()
    assert set(golden['init']) == set(decoders.TRAIN_PARAMS)
    for name, want in golden['init'].items():
        assert torch.equal(sd[name], want), name


def test_decoder_factory_needs_tokenizer_and_no_clip():
    with pytest.raises(NotImplementedError):
        decoders.decoder(corpus_dataset(), IdentityEncoder(64))
    with pytest.raises(NotImplementedError):
        decoders.decoder(corpus_dataset(), IdentityEncoder(64), rerank_with_clip=True,
                         indexer_kwargs=dict(tokenize=tokenize))


def test_golden_features_redraw_from_their_seed():
    """The fit goldens store a seed and a fingerprint instead of the features:
    the GPU tests draw them again from a seeded CPU generator."""
    meta = META['features']
    g = torch.Generator().manual_seed(meta['seed'])
    flat = torch.randn(*meta['shape'], generator=g).reshape(-1)
    assert flat[:len(meta['head'])].tolist() == meta['head']
    assert float(flat.double().sum()) == pytest.approx(meta['sum'], rel=1e-12)
    assert float((flat.double()**2).sum()) == pytest.approx(meta['sum_squares'],
                                                           rel=1e-12)


# ---- dropout mask ------------------------------------------------------------------
def test_decoder_dropout_mask_rate_and_determinism():
    m = lms.decoder_dropout_mask(12345, 64, 16, 512, .5)
    assert m.shape == (64, 16, 512) and m.dtype == torch.bool
    assert abs(float(m.float().mean()) - .5) < .01
    assert torch.equal(m, lms.decoder_dropout_mask(12345, 64, 16, 512, .5))
    assert not torch.equal(m, lms.decoder_dropout_mask(12346, 64, 16, 512, .5))
    # its own tag: never the LM's layer-0 mask for the same seed
    assert not torch.equal(m, lms.dropout_mask(12345, 0, 64, 16, 512, .5))
    low = lms.decoder_dropout_mask(7, 32, 8, 256, .1)
    assert abs(float(low.float().mean()) - .9) < .02
    assert lms.decoder_dropout_mask(7, 4, 4, 4, 0.).all()
