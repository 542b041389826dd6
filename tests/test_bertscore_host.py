"""Host side of BERTScore: idf, weights, the multi-reference maximum, the empty
sentence rule, the baseline, state-dict handling, `load`, and the plumbing of
`metrics.bert_score` / `Decoder.bert_score`, on hand-worked cases.  No GPU.
"""
import math
import pathlib
import sys
import warnings

import pytest
import torch

import bertref
from milan_amd import bertscore, decoders, metrics

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import bert_standin  # noqa: E402


def scorer(kind='roberta', **kwargs):
    cfg = bert_standin.CONFIGS[kind]
    return bertscore.BERTScorer(bert_standin.state_dict(cfg, 1), bert_standin.tokenizer(cfg),
                                num_layers=cfg['num_layers'], heads=cfg['heads'],
                                **bert_standin.ids_of(cfg), **kwargs), cfg


def test_idf_counts_sets_of_ids_and_specials_weigh_nothing():
    s, cfg = scorer(idf=True)
    v = bert_standin.vocab(cfg)
    with pytest.raises(ValueError, match='compute_idf'):
        s.token_weight(v['dog'])
    # 'dog' in 2 of 3 sentences (twice in one: a set), 'sky' in 1, 'red' in none
    s.compute_idf(['dog dog sky', 'a dog', 'the'])
    assert s.token_weight(v['dog']) == pytest.approx(math.log(4 / 3))
    assert s.token_weight(v['sky']) == pytest.approx(math.log(4 / 2))
    assert s.token_weight(v['red']) == pytest.approx(math.log(4))
    assert s.token_weight(v[cfg['cls']]) == 0. and s.token_weight(v[cfg['sep']]) == 0.
    with pytest.warns(UserWarning, match='Overwriting'):
        s.compute_idf(['dog'])
    assert s.token_weight(v['dog']) == pytest.approx(math.log(2 / 2))
    # the restatement the GPU tests trust agrees
    w = bertref.idf_weights([[0, 6, 6, 7, 2], [0, 4, 6, 2], [0, 5, 2]], 0, 2)
    assert w(6) == pytest.approx(math.log(4 / 3)) and w(0) == 0. and w(9) == pytest.approx(
        math.log(4))


def test_without_idf_every_token_weighs_one_except_the_specials():
    s, cfg = scorer(idf=False)
    v = bert_standin.vocab(cfg)
    assert [s.token_weight(t) for t in s.tokens('a dog')] == [0., 1., 1., 0.]
    w = bertref.idf_weights([], v[cfg['cls']], v[cfg['sep']], idf=False)
    assert [w(t) for t in s.tokens('a dog')] == [0., 1., 1., 0.]


def test_tokens_strip_and_the_empty_sentence_is_cls_sep():
    s, cfg = scorer('bert')
    v = bert_standin.vocab(cfg)
    assert s.tokens('  a dog ') == [v['[CLS]'], v['a'], v['dog'], v['[SEP]']]
    assert s.tokens('   ') == [v['[CLS]'], v['[SEP]']]
    assert s.max_length == cfg['max_positions']
    long = ' '.join(['dog'] * 60)
    assert len(s.tokens(long)) == s.max_length and s.tokens(long)[-1] == v['[SEP]']


def test_maximum_over_references_is_taken_per_field_then_the_baseline():
    s, _ = scorer()
    prf = torch.tensor([[.9, .2, .3], [.1, .8, .2], [.5, .5, .5], [.4, .6, .7]])
    p, r, f = s._combine(prf, owner=[0, 0, 1, 0], count=2)
    assert p.tolist() == pytest.approx([.9, .5]) and r.tolist() == pytest.approx([.8, .5])
    assert f.tolist() == pytest.approx([.7, .5])
    s2, _ = scorer(rescale_with_baseline=True, baseline=(.5, .6, .75))
    assert s2.baseline_vals.tolist() == pytest.approx([.5, .6, .75])
    p, r, f = s2._combine(prf, owner=[0, 0, 1, 0], count=2)
    assert p.tolist() == pytest.approx([.8, 0.]) and r.tolist() == pytest.approx([.5, -.25])
    assert f.tolist() == pytest.approx([-.2, -1.])
    with pytest.raises(ValueError, match='baseline'):
        scorer(rescale_with_baseline=True)


def test_baseline_file_is_read_at_the_row_of_num_layers(tmp_path):
    path = tmp_path / 'standin.tsv'
    path.write_text('LAYER,P,R,F\n0,.1,.2,.3\n1,.4,.5,.6\n2,.7,.8,.9\n')
    assert bertscore.read_baseline(path, 2) == (.7, .8, .9)
    s, _ = scorer(rescale_with_baseline=True, baseline=path)  # roberta stand-in: 2 layers run
    assert s.baseline_vals.tolist() == pytest.approx([.7, .8, .9])
    with pytest.raises(ValueError, match='no row'):
        bertscore.read_baseline(path, 17)


def test_empty_sentences_warn_and_score_zero_in_the_restatement():
    s, _ = scorer()
    with pytest.warns(UserWarning, match='Empty candidate'):
        sentences, ids, cand_of, ref_of, owner = s._prepare(['', 'a dog'],
                                                            [['dog'], ['a', 'a dog']])
    # deduplicated: 'a dog' is both a candidate and a reference
    assert sentences == ['', 'dog', 'a dog', 'a'] and cand_of == [0, 2, 2]
    assert ref_of == [1, 3, 2] and owner == [0, 1, 1] and ids[0] == [0, 2]
    with pytest.warns(UserWarning, match='Empty reference'):
        s._prepare(['a'], [' '])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        every = s._prepare(['a dog', 'a dog'], ['dog', 'dog'], dedup=False)[0]
    assert every == ['a dog', 'dog', 'a dog', 'dog']
    c, r = torch.randn(2, 8, dtype=torch.float64), torch.randn(5, 8, dtype=torch.float64)
    p, rr, f, low = bertref.pair(c, r, torch.tensor([0., 0.]), torch.ones(5))
    assert p == 0 and rr == 0 and f == 0 and low is None
    with pytest.raises(ValueError, match='candidates'):
        s._prepare(['a'], [])
    with pytest.raises(ValueError, match='at least one reference'):
        s._prepare(['a'], [[]])


def test_a_sentence_beyond_the_supported_length_names_itself():
    cfg = dict(bert_standin.CONFIGS['bert'], max_positions=100)
    s = bertscore.BERTScorer(bert_standin.state_dict(cfg, 1), bert_standin.tokenizer(cfg),
                             num_layers=2, heads=3, **bert_standin.ids_of(cfg))
    long = ' '.join(['dog'] * (bertscore.MAX_TOKENS - 1))  # + cls + sep = MAX_TOKENS + 1
    with pytest.raises(ValueError, match='65 tokens.*dog dog'):
        s._prepare([long], ['dog'])
    s._prepare([long[4:]], ['dog'])


def test_hand_worked_pair():
    """Two candidate tokens and three reference tokens on the unit circle."""
    def unit(deg):
        return [math.cos(math.radians(deg)), math.sin(math.radians(deg))]
    c = 2. * torch.tensor([unit(0), unit(90), unit(10)], dtype=torch.float64)
    r = torch.tensor([unit(0), unit(30), unit(60), unit(20)], dtype=torch.float64)
    p, rr, f, low = bertref.pair(c, r, torch.tensor([0., 1., 3.]), torch.tensor([0., 1., 1., 0.]))
    cos = lambda d: math.cos(math.radians(d))
    want_p = .25 * cos(30) + .75 * cos(10)  # 90 -> 60 deg; 10 -> 0 or 20
    want_r = .5 * cos(20) + .5 * cos(30)  # 30 -> 10; 60 -> 90
    assert float(p) == pytest.approx(want_p) and float(rr) == pytest.approx(want_r)
    assert float(f) == pytest.approx(2 * want_p * want_r / (want_p + want_r))
    assert low == pytest.approx(cos(30))


def test_prefix_stripping_and_dims_inference():
    cfg = bert_standin.CONFIGS['bert']
    sd = bert_standin.state_dict(cfg, 2)
    stripped, kind = bertscore.strip_prefix(sd)
    assert kind == 'bert' and 'embeddings.word_embeddings.weight' in stripped
    assert bertscore.strip_prefix(stripped)[1] is None
    dims = bertscore.infer_dims(sd, num_layers=3, heads=3)
    assert dims == dict(vocab_size=30, width=48, layers=3, heads=3, intermediate=64,
                        max_positions=40, type_vocab=2, position_offset=0, eps=1e-12)
    assert bertscore.infer_dims(sd, heads=3)['layers'] == 4
    with pytest.raises(ValueError, match='model_type'):
        bertscore.infer_dims(stripped)
    with pytest.raises(ValueError, match='multiple'):
        bertscore.infer_dims(sd, heads=5)
    with pytest.raises(ValueError, match='num_layers'):
        bertscore.infer_dims(sd, num_layers=5, heads=3)
    rob = bert_standin.state_dict(bert_standin.CONFIGS['roberta'], 2)
    with pytest.raises(ValueError, match='pad_id'):
        bertscore.infer_dims(rob, heads=4)
    with pytest.raises(ValueError, match='pass heads='):
        bertscore.infer_dims(rob, pad_id=1)  # width 48: no width // 64 default
    dims = bertscore.infer_dims(rob, pad_id=1, heads=4)
    assert dims['position_offset'] == 2 and dims['eps'] == 1e-5
    s, _ = scorer('bert')
    assert not any(k.startswith('pooler') or k.startswith('bert.') for k in s.weights)


def test_load_says_what_to_put_where(tmp_path, monkeypatch):
    monkeypatch.setenv('MILAN_MODELS_DIR', str(tmp_path))
    with pytest.raises(FileNotFoundError) as info:
        bertscore.load()
    assert str(tmp_path / 'roberta-large') in str(info.value)
    assert 'tokenizer.json' in str(info.value) and 'roberta-large.tsv' in str(info.value)
    # bert_scorer=None means bertscore.load()
    with pytest.raises(FileNotFoundError, match='MILAN_MODELS_DIR'):
        metrics.bert_score([], [], bert_scorer=None, annotation_index=0)
    (tmp_path / 'roberta-large').mkdir()
    with pytest.raises(FileNotFoundError, match='config.json'):
        bertscore.load()


def test_load_builds_the_scorer_from_a_model_directory(tmp_path):
    import json
    cfg = bert_standin.CONFIGS['roberta']
    root = tmp_path / 'standin'
    root.mkdir()
    special = bert_standin.ids_of(cfg)
    (root / 'config.json').write_text(json.dumps(dict(
        model_type='roberta', num_attention_heads=cfg['heads'], layer_norm_eps=cfg['eps'],
        pad_token_id=special['pad_id'])))
    torch.save(bert_standin.state_dict(cfg, 4), root / 'pytorch_model.bin')
    bert_standin.tokenizer(cfg).save(str(root / 'tokenizer.json'))
    (root / 'baseline.tsv').write_text('LAYER,P,R,F\n0,0,0,0\n1,0,0,0\n2,.25,.5,.75\n')
    with pytest.raises(ValueError, match='num_layers'):
        bertscore.load(root)
    s = bertscore.load(root, num_layers=2)
    assert s.idf and s.rescale_with_baseline and s.num_layers == 2
    assert s.baseline_vals.tolist() == [.25, .5, .75]
    assert (s.cls_id, s.sep_id, s.pad_id) == (0, 2, 1) and s.dims['position_offset'] == 2
    assert s.tokens('a dog') == [0, 4, 6, 2]


class StubScorer:
    idf = True

    def __init__(self):
        self.calls = []

    def compute_idf(self, sents):
        warnings.warn('Overwriting the previous importance weights.')
        self.calls.append(('idf', list(sents)))

    def score(self, cands, refs, batch_size=64):
        self.calls.append(('score', list(cands), [list(r) for r in refs], batch_size))
        n = len(cands)
        return (torch.arange(n).float(), torch.ones(n), torch.full((n,), .5))


def test_metrics_bert_score_normalises_flattens_and_names_its_keys():
    dataset = [(0, 0, 0, 0, ('A Dog. ', 'Blue SKY')), (0, 0, 0, 0, 'Grass.'),
               (0, 0, 0, 0, ['. tree', 'Red', 'a '])]
    stub = StubScorer()
    with warnings.catch_warnings():
        warnings.simplefilter('error')  # the overwrite warning is filtered, as in the reference
        out = metrics.bert_score(dataset, ['The dog.', ' Sky ', 'TREE. .'], batch_size=5,
                                 bert_scorer=stub)
    assert out == {'p': 1., 'r': 1., 'f': .5}
    refs = [['a dog', 'blue sky'], ['grass'], ['tree', 'red', 'a']]
    assert stub.calls == [('idf', ['a dog', 'blue sky', 'grass', 'tree', 'red', 'a']),
                          ('score', ['the dog', 'sky', 'tree'], refs, 5)]
    stub.idf = False
    stub.calls.clear()
    metrics.bert_score([(('x',),)], ['y'], annotation_index=0, bert_scorer=stub)
    assert stub.calls == [('score', ['y'], [['x']], 16)]


def test_decoder_bert_score_forwards_to_metrics(monkeypatch):
    seen = {}

    class Fake:
        def predict(self, dataset, **kwargs):
            seen['predict'] = kwargs
            return ('a dog',) * len(dataset)

    dataset = [(0, 0, 0, 0, 'a dog')] * 2
    stub = StubScorer()
    out = decoders.Decoder.bert_score(Fake(), dataset, bert_scorer=stub,
                                      bert_scorer_batch_size=3, predictions=['x', 'y'])
    assert set(out) == {'p', 'r', 'f'} and 'predict' not in seen
    assert stub.calls[-1] == ('score', ['x', 'y'], [['a dog'], ['a dog']], 3)
    decoders.Decoder.bert_score(Fake(), dataset, bert_scorer=stub, beam_size=7)
    assert seen['predict'] == {'beam_size': 7}
    assert stub.calls[-1] == ('score', ['a dog', 'a dog'], [['a dog'], ['a dog']], 16)
    assert decoders.DecoderWithCLIP.bert_score is decoders.Decoder.bert_score
