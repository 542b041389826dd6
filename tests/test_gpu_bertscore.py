"""BERTScore in HIP (csrc/bert.hip, milan_amd/bertscore.py) against float64.

Tolerance (tests/golden/reference_goldens_bertscore.json): bound = 4 x the error
of tests/bertref.py in float32 against bertref in float64 on the same case, no
floor -- the rule of DESIGN.md 4.14.  The goldens carry their bounds; a fuzz
case computes its own.  Every test prints the HIP error beside its bound;
DESIGN.md 4.15 records them.

Every case has positive best-match cosines in float64 (asserted by the golden
generator, checked per fuzz case), so bert_score's padding-mask quirk, which this
project does not reproduce, cannot matter.
"""
import functools
import json
import os
import pathlib
import sys

import pytest
import torch

import bertref
from milan_amd import bertscore, hip

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import bert_standin  # noqa: E402

META = json.loads((GOLDEN / 'reference_goldens_bertscore.json').read_text())
TENSORS = torch.load(GOLDEN / 'reference_goldens_bertscore.pt', weights_only=True)
VARIANTS = {'plain': (False, False), 'idf': (True, False), 'baseline': (False, True),
            'idf_baseline': (True, True)}


def build(cfg, sd, words=bert_standin.WORDS, **kwargs):
    return bertscore.BERTScorer(sd, bert_standin.tokenizer(cfg, words),
                                num_layers=cfg['num_layers'], heads=cfg['heads'],
                                device='cuda', **bert_standin.ids_of(cfg, words), **kwargs)


@pytest.mark.parametrize('kind', list(META['models']))
def test_golden_embeddings(kind):
    m = META['models'][kind]
    s = build(m['config'], TENSORS['weights/' + kind])
    got = torch.cat(list(s.embed(m['unique']))).cpu().double()
    want = TENSORS[kind + '/emb64']
    err = (got - want).abs().max().item()
    print(kind, 'embeddings: hip max |err| vs float64', err, 'bound', m['bound']['emb'])
    assert got.shape == want.shape and err <= m['bound']['emb']
    # normalised rows have unit length
    unit = torch.cat(list(s.embed(m['unique'], normalize=True)))
    assert (unit.norm(dim=-1) - 1).abs().max() < 1e-6


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', list(META['models']))
def test_golden_scores(kind, variant):
    m = META['models'][kind]
    idf, rescale = VARIANTS[variant]
    flat = [r for rs in m['references'] for r in rs]
    s = build(m['config'], TENSORS['weights/' + kind], idf=idf, idf_sents=flat if idf else None,
              rescale_with_baseline=rescale, baseline=META['baseline'])
    with pytest.warns(UserWarning, match='Empty candidate'):
        prf = s.score(m['candidates'], m['references'])
    got = torch.stack(prf, 1)
    assert got.dtype == torch.float32 and not got.is_cuda
    want = TENSORS[f'{kind}/prf64/{variant}']
    err = (got.double() - want).abs().max().item()
    bound = m['bound']['prf/' + variant]
    print(kind, variant, 'P/R/F: hip max |err| vs float64', err, 'bound', bound)
    assert err <= bound
    empty = m['candidates'].index('')
    raw = torch.zeros(3) if not rescale else -torch.tensor(META['baseline']) / (
        1 - torch.tensor(META['baseline']))
    assert torch.allclose(got[empty], raw.float(), atol=1e-6)


# ---- fuzz -------------------------------------------------------------------------------------
# MILAN_FUZZ_SEEDS=<n> widens the campaign
N_SEEDS = int(os.environ.get('MILAN_FUZZ_SEEDS', '10'))
HEAD_SIZES = (20, 64, 12, 16, 24, 40, 8, 72, 32, 48)


def fuzz_case(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    pick = lambda n: int(torch.randint(0, n, (1,), generator=g))
    kind = ('bert', 'roberta')[seed % 2]
    hd = HEAD_SIZES[seed % len(HEAD_SIZES)]  # seed 0: not a power of two
    heads = 1 + pick(3)
    layers = 2 + pick(2)
    cfg = dict(bert_standin.CONFIGS[kind], width=hd * heads, heads=heads, layers=layers,
               num_layers=layers - pick(2), intermediate=32 * (1 + pick(4)) + 8 * pick(2),
               max_positions=70, type_vocab=1 + pick(2))
    longest = 62 if seed % 10 == 1 else 4 + pick(20)  # seed 1: 64 tokens with the specials
    cands = bert_standin.sentences(g, 3 + pick(5), longest)
    refs = [bert_standin.sentences(g, 1 + pick(3), longest) for _ in cands]
    if seed % 10 == 1:
        cands[0] = ' '.join(bert_standin.sentences(g, 1, 62, shortest=62))
    return kind, cfg, cands, refs, bool(pick(2)), bool(pick(2))


def fuzz_reference(seed):
    """The case, its float64 P/R/F, the bound from the float32 restatement, and the smallest
    best-match cosine float64 met (runs on the CPU)."""
    kind, cfg, cands, refs, idf, rescale = fuzz_case(seed)
    sd = bert_standin.state_dict(cfg, 2000 + seed)
    tok = bert_standin.tokenizer(cfg)
    special = bert_standin.ids_of(cfg)
    rc = bert_standin.ref_cfg(cfg)
    ids = lambda s: tok.encode(s).ids
    flat = [r for rs in refs for r in rs]
    weight_of = bertref.idf_weights([ids(r) for r in flat], special['cls_id'],
                                    special['sep_id'], idf=idf)
    baseline = (.8, .7, .75) if rescale else None
    args = ([ids(c) for c in cands], [[ids(r) for r in rs] for rs in refs], weight_of, baseline)
    sd32 = bert_standin.strip(sd)
    *want, lowest = bertref.bert_score(bertref.cast(sd32, torch.float64), *args, **rc)
    *ref32, _ = bertref.bert_score(sd32, *args, **rc)
    want, ref32 = torch.stack(want, 1), torch.stack(ref32, 1)
    bound = 4 * (ref32.double() - want).abs().max().item()
    longest = max(len(ids(c)) for c in cands + flat)
    return (kind, cfg, cands, refs, idf, rescale, sd, flat, baseline), want, bound, lowest, longest


@functools.lru_cache(maxsize=None)
def run_fuzz(seed):
    """-> True when the case was compared, False when float64 found a non-positive
    best-match cosine (the one input on which bert_score itself is batch dependent)."""
    case, want, bound, lowest, longest = fuzz_reference(seed)
    kind, cfg, cands, refs, idf, rescale, sd, flat, baseline = case
    if lowest is None or lowest <= 0:
        return False
    s = build(cfg, sd, idf=idf, idf_sents=flat if idf else None, rescale_with_baseline=rescale,
              baseline=baseline)
    got = torch.stack(s.score(cands, refs, batch_size=5), 1)
    err = (got.double() - want).abs().max().item()
    print('seed', seed, kind, 'width', cfg['width'], 'heads', cfg['heads'], 'longest', longest,
          'hip err', err, 'bound', bound, 'smallest best-match cosine', lowest)
    assert err <= bound
    return True


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_fuzz_against_float64(seed):
    run_fuzz(seed)


def test_fuzz_covers_its_corners_and_skips_at_most_a_tenth():
    assert fuzz_case(0)[1]['width'] // fuzz_case(0)[1]['heads'] == 20
    kind, cfg, cands, _, _, _ = fuzz_case(1)
    assert len(cands[0].split()) + 2 == hip.BERT_MAX_TOKENS
    compared = [run_fuzz(seed) for seed in range(N_SEEDS)]
    print('fuzz cases', len(compared), 'skipped', compared.count(False))
    assert compared.count(False) <= .1 * len(compared)


# ---- properties -------------------------------------------------------------------------------
def golden_scorer(kind='roberta', **kwargs):
    m = META['models'][kind]
    flat = [r for rs in m['references'] for r in rs]
    return build(m['config'], TENSORS['weights/' + kind], idf=True, idf_sents=flat,
                 **kwargs), m


def test_batches_do_not_change_a_bit():
    """Rows are ragged and the GEMMs' split count depends on K alone: nothing a sentence
    is scored with depends on what else is in its batch."""
    s, m = golden_scorer()
    with pytest.warns(UserWarning):
        one = s.score(m['candidates'], m['references'], batch_size=1)
        seven = s.score(m['candidates'], m['references'], batch_size=7)
        whole = s.score(m['candidates'], m['references'], batch_size=10000)
    for a, b, c in zip(one, seven, whole):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_wide_model_is_batch_invariant_too():
    """Width 512 / intermediate 2048: K is large enough for split-K (2 and 4 splits)."""
    cfg = dict(bert_standin.CONFIGS['bert'], width=512, heads=8, layers=1, num_layers=1,
               intermediate=2048)
    s = build(cfg, bert_standin.state_dict(cfg, 3, std=.05))
    g = torch.Generator().manual_seed(4)
    cands = bert_standin.sentences(g, 6, 12)
    refs = [bert_standin.sentences(g, 2, 12) for _ in cands]
    one = s.score(cands, refs, batch_size=1)
    whole = s.score(cands, refs, batch_size=64)
    for a, b in zip(one, whole):
        assert torch.equal(a, b)
    sd32 = bert_standin.strip(bert_standin.state_dict(cfg, 3, std=.05))
    tok = bert_standin.tokenizer(cfg)
    ids = lambda t: tok.encode(t).ids
    special = bert_standin.ids_of(cfg)
    weight_of = bertref.idf_weights([], special['cls_id'], special['sep_id'], idf=False)
    args = ([ids(c) for c in cands], [[ids(r) for r in rs] for rs in refs], weight_of)
    *want, _ = bertref.bert_score(bertref.cast(sd32, torch.float64), *args,
                                  **bert_standin.ref_cfg(cfg))
    *ref32, _ = bertref.bert_score(sd32, *args, **bert_standin.ref_cfg(cfg))
    want, ref32 = torch.stack(want, 1), torch.stack(ref32, 1)
    bound = 4 * (ref32.double() - want).abs().max().item()
    err = (torch.stack(whole, 1).double() - want).abs().max().item()
    print('width 512: hip max |err| vs float64', err, 'bound', bound)
    assert err <= bound


def test_two_calls_give_the_same_bits_and_deduplication_changes_none():
    s, m = golden_scorer(rescale_with_baseline=True, baseline=META['baseline'])
    with pytest.warns(UserWarning):
        a = s.score(m['candidates'], m['references'])
        b = s.score(m['candidates'], m['references'])
        c = s.score(m['candidates'], m['references'], _dedup=False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # one reference per candidate may be given as a plain string
    single = s.score(m['candidates'][:2], [r[0] for r in m['references'][:2]])
    listed = s.score(m['candidates'][:2], [r[:1] for r in m['references'][:2]])
    assert all(torch.equal(x, y) for x, y in zip(single, listed))


def test_errors_fault_nothing():
    cfg = dict(bert_standin.CONFIGS['bert'], max_positions=100)
    s = build(cfg, bert_standin.state_dict(cfg, 1))
    long = ' '.join(['dog'] * 63)
    with pytest.raises(ValueError, match='65 tokens'):
        s.score([long], ['dog'])
    # the C entry point refuses the length on its own
    ctx = s._context()
    ids = torch.zeros(65, dtype=torch.long, device='cuda')
    offsets = torch.tensor([0, 65], dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='exceeds the supported 64'):
        ctx.encode(ids, offsets, 65)
    assert torch.isfinite(torch.stack(s.score(['a dog'], ['the dog']))).all()
    # head size 128: Q, K, V of 64 tokens do not fit a workgroup's LDS
    wide = dict(bert_standin.CONFIGS['bert'], width=256, heads=2, layers=1, num_layers=1)
    with pytest.raises(ValueError, match='head size 128.*LDS'):
        build(wide, bert_standin.state_dict(wide, 1))._context()
    with pytest.raises(IndexError):
        s2 = build(cfg, bert_standin.state_dict(cfg, 1, vocab_size=10))
        s2.score(['plants'], ['dog'])


def test_encode_and_score_pairs_capture_into_one_graph():
    s, m = golden_scorer()
    ctx = s._context()
    sentences, ids, cand_of, ref_of, _ = s._prepare(
        [c for c in m['candidates'] if c], [r for c, r in zip(m['candidates'],
                                                             m['references']) if c])
    lens = [len(i) for i in ids]
    dev = ctx.device
    flat = torch.tensor([t for i in ids for t in i], dtype=torch.long, device=dev)
    offsets = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(dev)
    weight = torch.tensor([s.token_weight(t) for i in ids for t in i], device=dev)
    cand = torch.tensor(cand_of, dtype=torch.int32, device=dev)
    ref = torch.tensor(ref_of, dtype=torch.int32, device=dev)
    emb = torch.empty(len(flat), s.dims['width'], device=dev)

    def call():
        ctx.encode(flat, offsets, max(lens), normalize=True, out=emb)
        return ctx.score_pairs(emb, offsets, weight, cand, ref)

    want = call().clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()
        with torch.cuda.graph(graph, stream=side):
            out = call()
    torch.cuda.current_stream().wait_stream(side)
    for replay in range(2):
        out.fill_(7)
        emb.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), replay


# ---- end to end -------------------------------------------------------------------------------
def test_decoder_bert_score_end_to_end():
    from milan_amd import decoders, encoders, lang, synthetic
    words = bert_standin.WORDS
    kind = 'roberta'
    m = META['models'][kind]
    cfg = m['config']
    idx = lang.Indexer(lang.Vocab(words), None, True, True, True, True, 15)
    enc = encoders.PyramidConvEncoder('resnet50', width=8, pretrained=False)
    torch.manual_seed(3)
    model = decoders.Decoder(idx, enc, embedding_size=4, hidden_size=8, length=6, beam_size=4)
    model.reset_parameters()
    model.precision = 'f32'
    model.to('cuda')
    dataset = synthetic.annotated_samples(6, words, annotations=3, seed=5)
    baseline = tuple(META['baseline'])
    s = build(cfg, TENSORS['weights/' + kind], idf=True, rescale_with_baseline=True,
              baseline=baseline)
    predictions = ['The dog and the sky.', 'blue things', 'Grass', 'a tree of stripes ',
                   'round water face', 'edge of the red dog']

    def reference(preds):
        tok = bert_standin.tokenizer(cfg)
        special = bert_standin.ids_of(cfg)
        ids = lambda t: tok.encode(t).ids
        preds = [p.lower().strip('. ') for p in preds]
        refs = [[a.lower().strip('. ') for a in sample[4]] for sample in dataset]
        weight_of = bertref.idf_weights([ids(r) for rs in refs for r in rs], special['cls_id'],
                                        special['sep_id'])
        args = ([ids(p) for p in preds], [[ids(r) for r in rs] for rs in refs], weight_of,
                baseline)
        sd32 = bert_standin.strip(TENSORS['weights/' + kind])
        *want, low = bertref.bert_score(bertref.cast(sd32, torch.float64), *args,
                                        **bert_standin.ref_cfg(cfg))
        *ref32, _ = bertref.bert_score(sd32, *args, **bert_standin.ref_cfg(cfg))
        assert low is None or low > 0
        # a mean is no further off than its worst element
        bound = 4 * max((a.double() - b).abs().max().item() for a, b in zip(ref32, want))
        return dict(zip('prf', (w.mean().item() for w in want))), bound

    got = model.bert_score(dataset, predictions=predictions, bert_scorer=s,
                           bert_scorer_batch_size=4)
    want, bound = reference(predictions)
    print('end to end', got, 'float64', want, 'bound', bound)
    assert set(got) == {'p', 'r', 'f'}
    assert all(abs(got[k] - want[k]) <= bound for k in 'prf')
    # without predictions= the decoder captions the dataset first
    captions = model.predict(dataset, display_progress_as=None)
    got = model.bert_score(dataset, bert_scorer=s, display_progress_as=None)
    want, bound = reference(captions)
    print('with predict', captions, got, 'float64', want, 'bound', bound)
    assert all(abs(got[k] - want[k]) <= bound for k in 'prf')
