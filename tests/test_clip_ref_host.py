"""tests/clipref.py (the float64-capable restatement the GPU tests measure
against) reproduces the reference's own outputs, stored in
tests/golden/reference_goldens_clip.pt, on the CPU."""
import json
import pathlib

import pytest
import torch

import clipref

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
META = json.loads((GOLDEN / 'reference_goldens_clip.json').read_text())
TENSORS = torch.load(GOLDEN / 'reference_goldens_clip.pt', weights_only=True)
BOUND = META['tolerance']['bound']


def test_bound_is_four_times_the_fp32_reference_error():
    tol = META['tolerance']
    assert tol['bound'] == 4 * tol['fp32_reference_max_abs_error']
    assert tol['pairs_within_twice_bound'] <= .02 * tol['adjacent_pairs']


@pytest.mark.parametrize('case', META['cases'], ids=lambda c: c['key'])
def test_clipref_matches_reference(case):
    dims = META['configs'][case['config']]
    sd = TENSORS['weights/' + case['config']]
    gold = TENSORS[case['key']]
    images, masks, texts = clipref.synthetic_inputs(dims, case['neurons'], case['k'],
                                                    case['candidates'], case['masks'],
                                                    case['seed'])
    assert texts == case['texts']
    assert float(images.double().sum() + masks.double().sum()) == pytest.approx(
        float(gold['fingerprint']), rel=1e-12)
    for dtype, sims, scores in ((torch.float32, gold['sims'], gold['scores']),
                                (torch.float64, gold['sims64'], gold['scores64'])):
        w = clipref.cast(sd, dtype)
        got = clipref.similarities(w, dims['vision_heads'], dims['text_heads'], images[0],
                                   gold['tokens'][0], masks[0], case['mask_layers'])
        print(case['key'], dtype, 'sims err', (got.double() - sims.double()).abs().max().item())
        assert (got.double() - sims.double()).abs().max() <= BOUND
        got = clipref.rerank_scores(w, dims['vision_heads'], dims['text_heads'], images, masks,
                                    gold['tokens'], case['lam'], case['mask_layers'])
        for a, b in zip(got, scores):
            assert (a.double() - b.double()).abs().max() <= BOUND


def test_causal_truncation_is_exact_in_float64():
    dims = META['configs']['small']
    sd = clipref.cast(TENSORS['weights/small'], torch.float64)
    tokens = TENSORS['case0']['tokens'][0]
    positions = int(tokens.argmax(dim=-1).max()) + 1
    assert positions < dims['context_length']
    full = clipref.encode_texts(sd, dims['text_heads'], tokens)
    cut = clipref.encode_texts(sd, dims['text_heads'], tokens, positions)
    assert (full - cut).abs().max() < 1e-14
