"""Corpus BLEU and BERTScore (reference `src/utils/metrics.py:16-43, 94-150`).

The reference scores with `sacrebleu.corpus_bleu` (sacrebleu 1.5.1, its
defaults: 13a tokenizer, 'exp' smoothing, no lowercasing, 4-grams).  sacrebleu
is not part of this build, so `corpus_bleu` below restates that computation in
pure Python.  It was written from knowledge of sacrebleu 1.5.1's algorithm, not
read from its source, and there is no oracle for it here: it is pinned by
hand-worked cases (tests/test_decoder_train_host.py) rather than checked
against sacrebleu itself.  `bert_score` keeps the reference's preprocessing and
hands the scoring to `milan_amd.bertscore` (HIP).  `rouge` alone is not built.
"""
import collections
import math
import re
import warnings
from typing import Any, List, Mapping, NamedTuple, Optional, Sequence

from torch.utils import data

NGRAM_ORDER = 4


class BLEUScore(NamedTuple):
    """The fields of sacrebleu's BLEUScore that the reference reads."""

    score: float
    counts: List[int]
    totals: List[int]
    precisions: List[float]
    bp: float
    sys_len: int
    ref_len: int


# mteval-v13a's regular expressions, in order (sacrebleu's TokenizerRegexp)
_13A = (
    (re.compile(r'([\{-\~\[-\` -\&\(-\+\:-\@\/])'), r' \1 '),
    (re.compile(r'([^0-9])([\.,])'), r'\1 \2 '),  # . , unless preceded by a digit
    (re.compile(r'([\.,])([^0-9])'), r' \1 \2'),  # . , unless followed by a digit
    (re.compile(r'([0-9])(-)'), r'\1 \2 '),  # - preceded by a digit
)


def tokenize_13a(line: str) -> str:
    """The '13a' tokenizer: a few entity / line-break substitutions, then the
    regular expressions above; tokens come back joined by single spaces."""
    line = line.replace('<skipped>', '')
    line = line.replace('-\n', '')
    line = line.replace('\n', ' ')
    line = line.replace('&quot;', '"')
    line = line.replace('&amp;', '&')
    line = line.replace('&lt;', '<')
    line = line.replace('&gt;', '>')
    line = f' {line} '
    for pattern, replacement in _13A:
        line = pattern.sub(replacement, line)
    return ' '.join(line.split())


def _ngrams(line: str) -> collections.Counter:
    tokens = line.split()
    counts: collections.Counter = collections.Counter()
    for n in range(1, NGRAM_ORDER + 1):
        for i in range(len(tokens) - n + 1):
            counts[' '.join(tokens[i:i + n])] += 1
    return counts


def corpus_bleu(hypotheses: Sequence[str],
                references: Sequence[Sequence[str]]) -> BLEUScore:
    """sacrebleu 1.5.1 `corpus_bleu(hypotheses, references)` with its defaults.

    `references` is a list of reference streams, each with one line per
    hypothesis.  Per sentence: n-gram counts (n <= 4) clipped by the largest
    count of that n-gram in any reference; the reference length is the one
    closest to the hypothesis length, ties to the shorter.  Corpus score:
    brevity penalty exp(1 - ref_len / sys_len) when sys_len < ref_len (0 when
    sys_len == 0) times the geometric mean of the n-gram precisions, where the
    j-th order with no match scores 100 / (2^j * total) ('exp' smoothing) and
    an order with no n-grams at all makes the score 0.  On a 0-100 scale."""
    streams = [list(hypotheses)] + [list(r) for r in references]
    if any(len(s) != len(streams[0]) for s in streams):
        raise EOFError('Source and reference streams have different lengths!')
    correct = [0] * NGRAM_ORDER
    total = [0] * NGRAM_ORDER
    sys_len = ref_len = 0
    for lines in zip(*streams):
        output, *refs = [tokenize_13a(x.rstrip()) for x in lines]
        hyp_len = len(output.split())
        ref_counts: collections.Counter = collections.Counter()
        closest_diff, closest_len = None, None
        for ref in refs:
            length = len(ref.split())
            diff = abs(hyp_len - length)
            if (closest_diff is None or diff < closest_diff or
                    (diff == closest_diff and length < closest_len)):
                closest_diff, closest_len = diff, length
            for ngram, count in _ngrams(ref).items():
                ref_counts[ngram] = max(ref_counts[ngram], count)
        sys_len += hyp_len
        ref_len += closest_len or 0
        for ngram, count in _ngrams(output).items():
            n = len(ngram.split())
            correct[n - 1] += min(count, ref_counts.get(ngram, 0))
            total[n - 1] += count

    precisions = [0.] * NGRAM_ORDER
    smooth = 1.
    for n in range(NGRAM_ORDER):
        if total[n] == 0:
            break
        if correct[n] == 0:
            smooth *= 2
            precisions[n] = 100. / (smooth * total[n])
        else:
            precisions[n] = 100. * correct[n] / total[n]
    if sys_len < ref_len:
        bp = math.exp(1 - ref_len / sys_len) if sys_len > 0 else 0.
    else:
        bp = 1.
    logs = [math.log(p) if p > 0 else -9999999999 for p in precisions]
    score = bp * math.exp(sum(logs) / NGRAM_ORDER)
    return BLEUScore(score, correct, total, precisions, bp, sys_len, ref_len)


def bleu(dataset: data.Dataset,
         predictions: Sequence[str],
         annotation_index: int = 4) -> BLEUScore:
    """Corpus BLEU of `predictions` against the annotations of `dataset`
    (reference metrics.py:16-43).  Predictions and references are lowercased
    and stripped of '. '.  As in the reference, the references are transposed
    with `zip`, so every sample contributes only as many references as the
    sample with the fewest annotations has."""
    predictions = [pred.lower().strip('. ') for pred in predictions]
    references = []
    for index in range(len(predictions)):
        annotations = dataset[index][annotation_index]
        if isinstance(annotations, str):
            annotations = [annotations]
        references.append([anno.lower().strip('. ') for anno in annotations])
    return corpus_bleu(predictions, list(zip(*references)))


def bert_score(dataset: data.Dataset,
               predictions: Sequence[str],
               annotation_index: int = 4,
               batch_size: int = 16,
               device: Optional[Any] = None,
               bert_scorer: Optional[Any] = None) -> Mapping[str, float]:
    """Average BERTScore P/R/F of `predictions` against the annotations of
    `dataset` (reference metrics.py:94-150), under the keys 'p', 'r', 'f'.
    Predictions and annotations are lowercased and stripped of '. '; with an
    idf scorer the idf is computed over all annotations, flattened.
    `bert_scorer` defaults to `bertscore.load(device=device)`: roberta-large
    cut to 17 layers, idf, rescaled with the baseline, read from
    `MILAN_MODELS_DIR`."""
    if bert_scorer is None:
        from milan_amd import bertscore
        bert_scorer = bertscore.load(idf=True, rescale_with_baseline=True,
                                     device=device)

    predictions = [pred.lower().strip('. ') for pred in predictions]

    references = []
    for index in range(len(predictions)):
        annotations = dataset[index][annotation_index]
        if isinstance(annotations, str):
            annotations = [annotations]
        references.append([anno.lower().strip('. ') for anno in annotations])

    if bert_scorer.idf:
        with warnings.catch_warnings():
            warnings.filterwarnings('ignore', message=r'.*Overwriting.*')
            bert_scorer.compute_idf([r for rs in references for r in rs])

    prf = bert_scorer.score(predictions, references, batch_size=batch_size)
    return {
        key: scores.mean().item() for key, scores in zip(('p', 'r', 'f'), prf)
    }
