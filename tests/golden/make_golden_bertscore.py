"""Writes tests/golden/reference_goldens_bertscore.{pt,json}: two stand-in encoders
(bert_standin.py), sentences of varied lengths with one empty candidate and 1 to 3 references
per candidate, and -- from tests/bertref.py in float64 -- the token embeddings and P/R/F with
and without idf and with and without the baseline.  For every quantity the json records the
error of the float32 restatement against float64; the GPU test's bound is 4 x that error, no
floor (the rule of DESIGN.md 4.14).

The generator asserts that every token's best-match cosine is positive in float64, so the
padding-mask quirk of bert_score that this project does not reproduce cannot matter.

    python tests/golden/make_golden_bertscore.py
"""
import json
import pathlib
import sys

import torch

HERE = pathlib.Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent)]
import bert_standin  # noqa: E402
import bertref  # noqa: E402

BASELINE = (.83, .81, .82)
VARIANTS = {'plain': (False, False), 'idf': (True, False), 'baseline': (False, True),
            'idf_baseline': (True, True)}
SEEDS = {'bert': 21, 'roberta': 22}


def cases(kind):
    g = torch.Generator().manual_seed(SEEDS[kind] + 100)
    cands = bert_standin.sentences(g, 9, 12)
    cands[4] = ''  # the empty candidate
    cands[7] = cands[1]  # a repeated candidate
    refs = []
    for n in range(len(cands)):
        refs.append(bert_standin.sentences(g, 1 + n % 3, 14))
    refs[2][0] = cands[2]  # a candidate equal to its reference
    refs[5][0] = refs[3][0]  # a reference shared by two candidates
    return cands, refs


def main():
    tensors, meta = {}, {'baseline': BASELINE, 'tolerance_factor': 4, 'models': {}}
    for kind, cfg in bert_standin.CONFIGS.items():
        sd = bert_standin.state_dict(cfg, SEEDS[kind])
        tensors['weights/' + kind] = sd
        tok = bert_standin.tokenizer(cfg)
        special = bert_standin.ids_of(cfg)
        rc = bert_standin.ref_cfg(cfg)
        cands, refs = cases(kind)

        def ids(s):
            return tok.encode(s.strip()).ids if s.strip() else [special['cls_id'],
                                                               special['sep_id']]

        unique = list(dict.fromkeys(cands + [r for rs in refs for r in rs]))
        sd32 = bert_standin.strip(sd)
        sd64 = bertref.cast(sd32, torch.float64)
        emb64 = torch.cat(bertref.encode(sd64, [ids(s) for s in unique], **rc))
        emb32 = torch.cat(bertref.encode(sd32, [ids(s) for s in unique], **rc))
        tensors[kind + '/emb64'] = emb64
        errors = {'emb': (emb32.double() - emb64).abs().max().item()}
        flat_refs = [r for rs in refs for r in rs]
        lowest = None
        for name, (idf, rescale) in VARIANTS.items():
            weight_of = bertref.idf_weights([ids(r) for r in flat_refs], special['cls_id'],
                                            special['sep_id'], idf=idf)
            args = ([ids(c) for c in cands], [[ids(r) for r in rs] for rs in refs], weight_of,
                    BASELINE if rescale else None)
            *prf64, low = bertref.bert_score(sd64, *args, **rc)
            *prf32, _ = bertref.bert_score(sd32, *args, **rc)
            prf64, prf32 = torch.stack(prf64, 1), torch.stack(prf32, 1)
            assert not torch.isnan(prf64).any()
            tensors[f'{kind}/prf64/{name}'] = prf64
            errors['prf/' + name] = (prf32.double() - prf64).abs().max().item()
            lowest = low if lowest is None else min(lowest, low)
        # the positivity condition: no token's best match is negative
        assert lowest is not None and lowest > 0, lowest
        meta['models'][kind] = {
            'seed': SEEDS[kind],
            'config': {k: v for k, v in cfg.items()},
            'candidates': cands,
            'references': refs,
            'unique': unique,
            'ref32_max_abs_error': errors,
            'bound': {k: 4 * v for k, v in errors.items()},
            'smallest_best_match_cosine': lowest,
            'hip_max_abs_error': {},  # measured on an MI355X: DESIGN.md 4.15
        }
        print(kind, 'fp32 restatement errors', errors, 'smallest best-match cosine', lowest)
    torch.save(tensors, HERE / 'reference_goldens_bertscore.pt')
    (HERE / 'reference_goldens_bertscore.json').write_text(json.dumps(meta, indent=1) + '\n')


if __name__ == '__main__':
    main()
