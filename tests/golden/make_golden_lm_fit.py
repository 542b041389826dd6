"""Goldens for LanguageModel training: the reference's `lang.vocab` /
`lang.indexer`, `lms.lm` and `LanguageModel.fit` on a tiny seeded corpus.

Run in the build container (the reference is not available on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lm_fit.py

Imports the reference with the stub modules of make_golden.py and a plain
whitespace tokenizer standing in for spaCy, then records

  vocab    token order of `vocab` / `indexer` on the corpus, with and without
           `ignore_rarer_than` / `ignore_in`;
  init     the state dict `lms.lm(dataset, ...)` builds after a seed;
  fit_*    `lm.fit(...)` with dropout 0, batch 16, AdamW (lr 1e-3): the torch
           RNG state right before the call, the initial and final state dicts,
           every per-batch loss (train / val; captured by wrapping
           torch.nn.NLLLoss, the reference code is not touched), the per-epoch
           means and the number of epochs run.  `fit_split` holds out 10 %
           at random, `fit_fixed` a fixed index list, `fit_stop` uses a large
           learning rate and patience 0 so that early stopping triggers.

Outputs: reference_goldens_lm_fit.pt / .json (data only).
"""
import json
import pathlib
import random
import sys

import torch
from torch import nn

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'neuron-descriptions_amd'))
sys.path.insert(0, str(HERE))

import make_golden  # noqa: E402  (stubs + import_reference)

WORDS = ('a the of and with in on dog dogs cat cats red blue green white black '
         'small large striped furry wooden metal car cars wheel wheels tree '
         'trees leaves grass sky water boat boats person people face faces '
         'text letters building windows door road sign bird birds fish '
         'flowers pattern stripes circles edges shapes animal animals '
         'object objects').split()


def tokenize(texts):
    """Lower-case whitespace split (stands in for the spaCy tokenizer)."""
    if isinstance(texts, str):
        return tuple(texts.lower().split())
    return tuple(tuple(t.lower().split()) for t in texts)


def corpus(seed=0, samples=150):
    """Dataset of (.., .., .., .., annotation) samples; every third sample has
    a list of two captions, so there are 200 sequences.  Zipf-ish word
    frequencies, a few words rare enough for `ignore_rarer_than`."""
    rng = random.Random(seed)
    weights = [1.0 / (i + 1)**0.9 for i in range(len(WORDS))]

    def caption():
        n = rng.randint(2, 9)
        return ' '.join(rng.choices(WORDS, weights)[0] for _ in range(n))

    data = []
    for i in range(samples):
        ann = [caption(), caption()] if i % 3 == 0 else caption()
        data.append((i, None, None, None, ann))
    return data


class RecordingNLL(nn.NLLLoss):
    log = []

    def forward(self, input, target):
        loss = super().forward(input, target)
        RecordingNLL.log.append(
            ('train' if torch.is_grad_enabled() else 'val', loss.item()))
        return loss


def state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def main():
    torch.set_num_threads(8)
    _, _, lms, lang, _, _ = make_golden.import_reference()
    nn.NLLLoss = RecordingNLL  # what lms.fit instantiates (torch.nn.NLLLoss)
    out, meta = {}, {}
    data = corpus()
    texts = [lang.join(sample[4]) for sample in data]

    meta['vocab'] = {}
    for name, kw in (('plain', {}), ('rare', dict(ignore_rarer_than=9)),
                     ('ignore', dict(ignore_in=['a', 'the', 'of'])),
                     ('both', dict(ignore_rarer_than=12,
                                   ignore_in=('dog', 'cats')))):
        meta['vocab'][name] = {
            'kwargs': {k: list(v) if isinstance(v, tuple) else v
                       for k, v in kw.items()},
            'vocab': list(lang.vocab(texts, tokenize=tokenize, **kw).tokens),
            'indexer': list(lang.indexer(texts, tokenize=tokenize,
                                         **kw).vocab.tokens),
        }

    dims = dict(embedding_size=16, hidden_size=32, layers=2, dropout=0.)
    meta['dims'] = dims
    torch.manual_seed(7)
    model = lms.lm(data, indexer_kwargs=dict(tokenize=tokenize), **dims)
    meta['lm_tokens'] = list(model.indexer.vocab.tokens)
    meta['lm_flags'] = [model.indexer.start, model.indexer.stop,
                        model.indexer.pad, model.indexer.unk]
    out['init'] = state(model)
    meta['corpus'] = [sample[4] for sample in data]

    cases = {
        'fit_split': dict(seed=11, kwargs=dict(hold_out=.1, max_epochs=3)),
        'fit_fixed': dict(seed=12, kwargs=dict(
            hold_out=list(range(0, 200, 9)), max_epochs=2)),
        'fit_stop': dict(seed=13, kwargs=dict(
            hold_out=.1, max_epochs=8, patience=0,
            optimizer_kwargs=dict(lr=0.05))),
    }
    for name, case in cases.items():
        torch.manual_seed(7)
        model = lms.lm(data, indexer_kwargs=dict(tokenize=tokenize), **dims)
        torch.manual_seed(case['seed'])
        out[f'{name}_rng'] = torch.get_rng_state()
        out[f'{name}_init'] = state(model)
        RecordingNLL.log = []
        model.fit(data, batch_size=16, display_progress_as=None,
                  **case['kwargs'])
        out[f'{name}_final'] = state(model)
        train, val, epochs = [], [], []
        for mode, value in RecordingNLL.log:
            (train if mode == 'train' else val).append(value)
            if mode == 'val' and (not epochs or epochs[-1][0] == 'train'):
                epochs.append(['val', len(train), len(val) - 1])
            if mode == 'train' and (not epochs or epochs[-1][0] == 'val'):
                epochs.append(['train', len(train) - 1])
        n_epochs = sum(1 for e in epochs if e[0] == 'val')
        n_train = len(train) // n_epochs
        n_val = len(val) // n_epochs
        meta[name] = {
            'kwargs': case['kwargs'],
            'epochs': n_epochs,
            'train_batches': n_train,
            'val_batches': n_val,
            'batch_train_loss': train,
            'batch_val_loss': val,
            'train_loss': [sum(train[e * n_train:(e + 1) * n_train]) / n_train
                           for e in range(n_epochs)],
            'val_loss': [sum(val[e * n_val:(e + 1) * n_val]) / n_val
                         for e in range(n_epochs)],
        }
        print(name, 'epochs', n_epochs, 'val', meta[name]['val_loss'])

    torch.save(out, HERE / 'reference_goldens_lm_fit.pt')
    with open(HERE / 'reference_goldens_lm_fit.json', 'w') as f:
        json.dump(meta, f, indent=1)


if __name__ == '__main__':
    main()
