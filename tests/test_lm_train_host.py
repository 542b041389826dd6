"""LanguageModel training, host side: vocabulary / indexer / `lm()` against the
reference goldens (tests/golden/make_golden_lm_fit.py), the training
utilities, and the host restatement of the kernels' dropout mask."""
import json

import pytest
import torch

from conftest import GOLDEN_DIR
from milan_amd import lang, lms, training

META = json.loads((GOLDEN_DIR / 'reference_goldens_lm_fit.json').read_text())


def tokenize(texts):
    """The goldens' stand-in for the spaCy tokenizer."""
    if isinstance(texts, str):
        return tuple(texts.lower().split())
    return tuple(tuple(t.lower().split()) for t in texts)


def dataset():
    return [(i, None, None, None, ann) for i, ann in enumerate(META['corpus'])]


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN_DIR / 'reference_goldens_lm_fit.pt')


@pytest.mark.parametrize('case', sorted(META['vocab']))
def test_vocab_and_indexer_match_reference(case):
    want = META['vocab'][case]
    texts = [lang.join(ann) for ann in META['corpus']]
    assert list(lang.vocab(texts, tokenize, **want['kwargs']).tokens) == \
        want['vocab']
    idx = lang.indexer(texts, tokenize, start=True, **want['kwargs'])
    assert list(idx.vocab.tokens) == want['indexer']
    assert idx.start and not idx.stop and idx.tokenize is tokenize


def test_vocab_without_tokenizer_raises_like_indexer():
    with pytest.raises(NotImplementedError, match='needs a tokenizer'):
        lang.vocab(['a b'])
    with pytest.raises(NotImplementedError, match='needs a tokenizer'):
        lms.lm(dataset())


def test_lm_factory_matches_reference(golden):
    torch.manual_seed(7)
    model = lms.lm(dataset(), indexer_kwargs=dict(tokenize=tokenize),
                   **META['dims'])
    assert list(model.indexer.vocab.tokens) == META['lm_tokens']
    assert [model.indexer.start, model.indexer.stop, model.indexer.pad,
            model.indexer.unk] == META['lm_flags']
    state = model.state_dict()
    assert list(state) == list(golden['init'])
    for name, want in golden['init'].items():
        assert torch.equal(state[name], want), name
    assert not state['embedding.weight'][model.indexer.pad_index].any()


def test_sequence_dataset_flattens_lists():
    seqs = lms._SequenceDataset(dataset())
    assert len(seqs) == 200
    assert seqs[0] == META['corpus'][0][0] and seqs[1] == META['corpus'][0][1]
    assert seqs[2] == META['corpus'][1]


def test_early_stopping():
    stop = training.EarlyStopping(patience=2)
    assert not stop(3.) and stop.improved and stop.best == 3.
    assert not stop(3.) and not stop.improved  # equal is not better
    assert not stop(2.5) and stop.improved
    assert not stop(4.) and not stop(5.)
    assert stop(6.) and stop.num_bad == 3 and stop.best == 2.5
    up = training.EarlyStopping(patience=0, decreasing=False)
    assert not up(1.) and up.improved
    assert up(0.5)


def test_random_split_draws_like_torch():
    data = list(range(50))
    torch.manual_seed(3)
    train, val = training.random_split(data, hold_out=.1)
    torch.manual_seed(3)
    want_train, want_val = torch.utils.data.random_split(data, (45, 5))
    assert list(train.indices) == list(want_train.indices)
    assert list(val.indices) == list(want_val.indices)
    for bad in (0., 1., -.5, 1.5):
        with pytest.raises(ValueError, match='hold_out must be in'):
            training.random_split(data, hold_out=bad)
    with pytest.raises(ValueError, match='causes val set size to be zero'):
        training.random_split(list(range(5)), hold_out=.1)


def test_fixed_split():
    data = list(range(6))
    train, val = training.fixed_split(data, [4, 1])
    assert list(train.indices) == [0, 2, 3, 5] and list(val.indices) == [4, 1]
    with pytest.raises(IndexError, match='dataset index out of bounds: 6'):
        training.fixed_split(data, [6])
    with pytest.raises(IndexError, match='out of bounds: -1'):
        training.fixed_split(data, [-1])
    with pytest.raises(ValueError, match='nothing to split'):
        training.fixed_split(data, range(6))


def test_dropout_mask_is_a_pure_function_with_the_right_rate():
    a = lms.dropout_mask(1234, 0, 64, 16, 512, 0.5)
    assert a.shape == (64, 16, 512) and a.dtype == torch.bool
    assert torch.equal(a, lms.dropout_mask(1234, 0, 64, 16, 512, 0.5))
    # a prefix of a larger batch is the same mask: (row, t, unit) addressing
    assert torch.equal(a[:10, :5, :7], lms.dropout_mask(1234, 0, 10, 5, 7, .5))
    assert abs(a.float().mean().item() - 0.5) < 0.005
    assert not torch.equal(a, lms.dropout_mask(1235, 0, 64, 16, 512, 0.5))
    assert not torch.equal(a, lms.dropout_mask(1234, 1, 64, 16, 512, 0.5))
    for p in (0.1, 0.3, 0.8):
        keep = lms.dropout_mask(99, 1, 64, 16, 256, p).float().mean().item()
        assert abs(keep - (1 - p)) < 0.006, (p, keep)
    assert lms.dropout_mask(5, 0, 4, 4, 4, 0.).all()
