"""Goldens G18-G19 of the CLIP reranker: the reference's unmodified
`CLIPWithMasks` and `CLIPWithMasksReranker` run on the CPU over clip_standin.py
(installed as `clip`), in fp32 -- the goldens -- and in float64 -- the yardstick
the fp32 reference's own error is measured against.

    python tests/golden/make_golden_clip.py

writes tests/golden/reference_goldens_clip.pt (tensors: weights, token ids,
outputs; data only -- images and masks are redrawn from the case's seed by
clipref.synthetic_inputs and checked against a stored fingerprint) and reference_goldens_clip.json (dims, cases, the measured
fp32-reference error and the bound derived from it).

Tolerance: bound = 4 x the largest |fp32 reference - float64 reference| over
all golden similarities and scores (both sides are fp32 with different summation
orders; the factor covers order and depth).  Orders are compared only across
adjacent pairs whose float64 score gap exceeds 2 x bound; the generator asserts
that at most 2 % of adjacent pairs fall below that gap, and that the fp32
reference itself passes the same check.
"""
import json
import pathlib
import sys

import torch

HERE = pathlib.Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent), str(HERE.parent.parent),
                str(HERE.parent.parent / 'neuron-descriptions_amd')]

import allennlp_standin  # noqa: E402
import clip_standin  # noqa: E402
import clipref  # noqa: E402
import make_golden  # noqa: E402

CONFIGS = {
    'small': dict(seed=3),
    'odd': dict(seed=5, resolution=48, patch=12, vision_width=30,
                vision_layers=3, vision_heads=5, embed_dim=24,
                context_length=24, vocab_size=80, text_width=30, text_layers=3,
                text_heads=5),
}
# (config, neurons, k, candidates per neuron, lam, mask_layers, mask kind, seed)
CASES = [
    ('small', 2, 3, (6, 9), .5, None, 'random', 11),
    ('small', 1, 1, (7,), 0., (1,), 'random', 12),
    ('small', 2, 2, (5, 5), 1., (), 'random', 13),
    ('small', 1, 4, (8,), .5, None, 'zeros', 14),
    ('small', 1, 4, (8,), 0., None, 'ones', 15),
    ('odd', 3, 5, (12, 3, 10), .5, (0, 2), 'random', 16),
    ('odd', 2, 2, (9, 9), .25, None, 'random', 17),
]


def decoder_case(tensors, meta, bound):
    """G19: the reference's DecoderWithCLIP.forward end to end on a synthetic decoder
    (beam search on the allennlp stand-in, then its own reranker over clip_standin)."""
    from src.milan import decoders, encoders
    from src.utils import lang
    from milan_amd import synthetic
    case = dict(clipref.DECODER_CASE)
    config = dict(CONFIGS[case['config']])
    seed = config.pop('seed')
    clip_standin.configure(seed=seed, **config)
    dims = dict(clip_standin.DEFAULTS, **config)

    class PoolEncoder(encoders.Encoder):

        def __init__(self):
            super().__init__()
            self.feature_shape = (clipref.POOL_FEATURES,)

        def forward(self, images, masks=None, **_):
            return clipref.pool_features(images, masks)

        def properties(self):
            return {}

    vocab = lang.Vocab(synthetic.vocab_tokens(case['nvocab']))
    indexer = lang.Indexer(vocab, lang.Tokenizer(nlp=object()), start=True, stop=True,
                           pad=True, unk=True, length=case['length'])
    dec = decoders.DecoderWithCLIP(indexer, PoolEncoder(), embedding_size=case['emb'],
                                   hidden_size=case['hidden'], length=case['length'],
                                   beam_size=case['beam'],
                                   reranker_kwargs=dict(lam=case['lam']))
    assert (dec.strategy, dec.temperature) == ('beam', .5)
    sd = synthetic.decoder_state_dict(len(indexer), feature_size=clipref.POOL_FEATURES,
                                      hidden_size=case['hidden'], embedding_size=case['emb'],
                                      lm=False, seed=case['weight_seed'])
    result = dec.load_state_dict(sd, strict=False)
    assert not result.unexpected_keys
    assert all(k.startswith('reranker.') for k in result.missing_keys), result.missing_keys
    dec.eval()
    images, masks, _ = clipref.synthetic_inputs(dims, case['neurons'], case['k'],
                                                [1] * case['neurons'], 'random',
                                                case['input_seed'])
    with torch.no_grad():
        out = dec(images, masks)
    # the float64 rerank scores of the beam: the winner must be clear of 2 x bound
    weights = clipref.cast(tensors['weights/' + case['config']], torch.float64)
    texts = [list(c) for c in out.beam_captions]
    tokens = [clip_standin.tokenize(t) for t in texts]
    scores64 = clipref.rerank_scores(weights, dims['vision_heads'], dims['text_heads'], images,
                                     masks, tokens, case['lam'])
    choice = []
    for n, s in enumerate(scores64):
        # (equal captions score equal: the margin is to the best DIFFERENT caption)
        best = int(s.argmax())
        others = [float(s[i]) for i, t in enumerate(texts[n]) if t != texts[n][best]]
        assert float(s[best]) - max(others) > 2 * bound, (n, float(s[best]), max(others))
        assert out.captions[n] == texts[n][best]
        choice.append(texts[n].index(out.captions[n]))
        assert torch.equal(out.tokens[n], out.beam_tokens[n, choice[-1]])
        assert torch.equal(out.scores[n], out.beam_scores[n, choice[-1]])
    assert out.predictions is None and out.attentions is None
    tensors['decoder'] = dict(tokens=out.tokens.clone(), scores=out.scores.clone(),
                              beam_tokens=out.beam_tokens.clone(),
                              beam_scores=out.beam_scores.clone(), scores64=scores64)
    meta['decoder'] = dict(case, captions=list(out.captions), beam_captions=texts,
                           choice=choice)


def main():
    make_golden.import_reference(allennlp_standin)
    from src.milan import rerankers
    rerankers.clip = clip_standin

    tensors, meta = {}, {'configs': {}, 'cases': []}
    worst, pairs, close = 0., 0, 0
    gaps = []
    for name, config in CONFIGS.items():
        config = dict(config)
        seed = config.pop('seed')
        clip_standin.configure(seed=seed, **config)
        dims = dict(clip_standin.DEFAULTS, **config)
        meta['configs'][name] = dict(dims, seed=seed)
        tensors[f'weights/{name}'] = {
            k: v.clone() for k, v in clip_standin.load()[0].state_dict().items()
        }
        for index, case in enumerate(CASES):
            cfg, neurons, k, counts, lam, layers, kind, case_seed = case
            if cfg != name:
                continue
            images, masks, texts = clipref.synthetic_inputs(dims, neurons, k, counts, kind, case_seed)
            tokens = [clip_standin.tokenize(t) for t in texts]
            out = {}
            for dtype in (torch.float32, torch.float64):
                r = rerankers.reranker(lam=.125, mask_layers=layers)
                r = r.to(dtype)
                with torch.no_grad():
                    ranked = r(images.to(dtype), masks.to(dtype), texts, lam=lam)
                    sims = r.clip_with_masks(images[0].to(dtype), texts[0],
                                             masks=masks[0].to(dtype))
                scores = []
                for order, score in zip(ranked.orders, ranked.scores):
                    unsorted = torch.empty(len(order), dtype=torch.float64)
                    unsorted[list(order)] = torch.tensor(score, dtype=torch.float64)
                    scores.append(unsorted)
                out[dtype] = (ranked, sims.double(), scores)
            (r32, s32, u32), (r64, s64, u64) = out[torch.float32], out[torch.float64]
            worst = max(worst, (s32 - s64).abs().max().item(),
                        max((a - b).abs().max().item() for a, b in zip(u32, u64)))
            key = f'case{index}'
            tensors[key] = dict(tokens=tokens, fingerprint=images.double().sum() + masks.double().sum(),
                                sims=s32.float(), sims64=s64,
                                scores=[u.float() for u in u32], scores64=u64)
            for u in u64:
                gaps.append(u.sort(descending=True).values.diff().abs())
            meta['cases'].append(dict(key=key, config=cfg, neurons=neurons, k=k,
                                      candidates=list(counts), lam=lam,
                                      mask_layers=None if layers is None else list(layers),
                                      masks=kind, seed=case_seed, texts=texts,
                                      orders=[list(o) for o in r32.orders],
                                      orders64=[list(o) for o in r64.orders],
                                      reranked=[list(t) for t in r32.texts]))
    bound = 4 * worst
    decoder_case(tensors, meta, bound)
    gaps = torch.cat(gaps)
    close = int((gaps <= 2 * bound).sum())
    assert close <= .02 * len(gaps), (close, len(gaps))
    # the fp32 reference itself passes the order check
    for case in meta['cases']:
        for n, (o32, u64) in enumerate(zip(case['orders'], tensors[case['key']]['scores64'])):
            s = u64[o32]
            assert bool((s[:-1] - s[1:] > -2 * bound).all()), (case['key'], n)
    meta['tolerance'] = dict(
        fp32_reference_max_abs_error=worst, factor=4, bound=bound,
        adjacent_pairs=len(gaps), pairs_within_twice_bound=close,
        note='bound = 4 x max |fp32 reference - float64 reference| over all golden '
             'similarities and scores; hip_max_abs_error = the largest HIP error against float64 '
             'over the golden cases, measured on an MI355X (recorded, never used for the bound)')
    old = HERE / 'reference_goldens_clip.json'
    if old.exists():  # keep the recorded GPU measurement
        previous = json.loads(old.read_text()).get('tolerance', {})
        if 'hip_max_abs_error' in previous:
            meta['tolerance']['hip_max_abs_error'] = previous['hip_max_abs_error']
    torch.save(tensors, HERE / 'reference_goldens_clip.pt')
    old.write_text(json.dumps(meta, indent=1) + '\n')
    print(json.dumps(meta['tolerance'], indent=1))


if __name__ == '__main__':
    main()
