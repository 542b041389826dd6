"""BERTScore on the GPU (reference `src/utils/metrics.py:94-150`), in HIP.

The reference scores captions with `bert_score.BERTScorer(idf=True, lang='en',
rescale_with_baseline=True)` (bert_score 0.3.11): `roberta-large` cut to its
first 17 layers embeds every token of every caption and annotation, and each
(candidate, reference) pair is scored by greedy cosine matching of the tokens,
weighted by idf.  Here the encoder and the matching are HIP kernels
(csrc/bert.hip) in exact fp32: the sentences of a call run through every layer
as ragged rows, with no padding, and every distinct sentence is encoded once.

Neither the `bert_score` package nor any checkpoint ships with this project,
and nothing here touches the network.  `BERTScorer(weights=..., tokenizer=...)`
takes a HuggingFace state dict and a tokenizer from the user; `load()` reads
both from a directory under `MILAN_MODELS_DIR`.  The algorithm below was
written from knowledge of bert_score 0.3.11, not read from its source (the
package is not installed here); the encoder is checked against `transformers`
(tests/test_bertscore_ref_vs_transformers.py).

One deliberate deviation: the library pads every batch and multiplies the
similarity matrix by the padding mask, so a token whose best real match has a
negative cosine scores 0 if, and only if, its batch happened to hold a longer
sentence.  Here the maximum runs over the other sentence's real tokens only,
whatever else is scored in the same call.
"""
import collections
import json
import math
import os
import pathlib
import warnings
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple, Union

import torch

from milan_amd import hip

StrSequence = Sequence[str]

PREFIXES = {'roberta.': 'roberta', 'bert.': 'bert'}
LAYER_NORM_EPS = {'roberta': 1e-5, 'bert': 1e-12}
# bert_score's model2layers, for the models `load` knows by name
NUM_LAYERS = {'roberta-large': 17, 'roberta-base': 10, 'bert-base-uncased': 9,
              'bert-large-uncased': 18}
MAX_TOKENS = hip.BERT_MAX_TOKENS


def strip_prefix(
    state_dict: Mapping[str, torch.Tensor]
) -> Tuple[Dict[str, torch.Tensor], Optional[str]]:
    """The state dict without its leading `roberta.` / `bert.` and the model
    type that prefix names (None when there is none)."""
    for prefix, kind in PREFIXES.items():
        if any(key.startswith(prefix + 'embeddings.') for key in state_dict):
            return ({key[len(prefix):]: value
                     for key, value in state_dict.items()
                     if key.startswith(prefix)}, kind)
    return dict(state_dict), None


def infer_dims(state_dict: Mapping[str, torch.Tensor],
               num_layers: Optional[int] = None,
               heads: Optional[int] = None,
               model_type: Optional[str] = None,
               pad_id: Optional[int] = None,
               layer_norm_eps: Optional[float] = None) -> Dict[str, Any]:
    """Dims of a BERT-family encoder from its state dict (prefix stripped or
    not).  What a state dict cannot tell comes from the arguments: `heads`
    (width // 64 unless given), the model type (from the prefix unless given:
    it decides the position offset -- `pad_id + 1` for RoBERTa, 0 for BERT --
    and the default LayerNorm eps), and how many layers to run."""
    state_dict, kind = strip_prefix(state_dict)
    model_type = model_type or kind
    if model_type not in LAYER_NORM_EPS:
        raise ValueError('cannot tell BERT from RoBERTa: the state dict has no '
                         '"bert." / "roberta." prefix; pass model_type=')
    try:
        word = state_dict['embeddings.word_embeddings.weight']
        total_layers = len({
            key.split('.')[2] for key in state_dict
            if key.startswith('encoder.layer.')
        })
        dims = {
            'vocab_size': word.shape[0],
            'width': word.shape[1],
            'layers': total_layers if num_layers is None else num_layers,
            'heads': heads or word.shape[1] // 64,
            'intermediate':
                state_dict['encoder.layer.0.intermediate.dense.weight'].shape[0],
            'max_positions':
                state_dict['embeddings.position_embeddings.weight'].shape[0],
            'type_vocab':
                state_dict['embeddings.token_type_embeddings.weight'].shape[0],
        }
    except KeyError as error:
        raise ValueError(f'BERT state dict lacks {error}') from error
    if not 1 <= dims['layers'] <= total_layers:
        raise ValueError(f'num_layers {dims["layers"]} is not in 1 .. '
                         f'{total_layers}, the layers of the state dict')
    if dims['heads'] < 1 or dims['width'] % dims['heads']:
        raise ValueError(f'width {dims["width"]} is not a multiple of '
                         f'{dims["heads"]} heads; pass heads=')
    if model_type == 'roberta':
        if pad_id is None:
            raise ValueError('RoBERTa numbers positions from pad_id + 1: '
                             'pass pad_id=')
        dims['position_offset'] = pad_id + 1
    else:
        dims['position_offset'] = 0
    dims = {key: int(value) for key, value in dims.items()}
    dims['eps'] = float(layer_norm_eps or LAYER_NORM_EPS[model_type])
    return dims


def read_baseline(path: Union[str, os.PathLike],
                  num_layers: int) -> Tuple[float, float, float]:
    """(P, R, F) of row `num_layers` of bert_score's rescale_baseline file
    (`LAYER,P,R,F`, one row per layer count from 0)."""
    rows = pathlib.Path(path).read_text().split('\n')[1:]
    for row in rows:
        fields = row.replace('\t', ',').split(',')
        if len(fields) >= 4 and int(fields[0]) == num_layers:
            return (float(fields[1]), float(fields[2]), float(fields[3]))
    raise ValueError(f'{path} has no row for {num_layers} layers')


class BERTScorer:
    """`bert_score.BERTScorer` as far as the reference uses it: `idf`,
    `compute_idf`, `score`, `baseline_vals`, `rescale_with_baseline`."""

    def __init__(self,
                 weights: Union[str, os.PathLike, Mapping[str, torch.Tensor]],
                 tokenizer: Any,
                 cls_id: int,
                 sep_id: int,
                 pad_id: Optional[int] = None,
                 num_layers: Optional[int] = None,
                 heads: Optional[int] = None,
                 model_type: Optional[str] = None,
                 layer_norm_eps: Optional[float] = None,
                 idf: bool = False,
                 idf_sents: Optional[StrSequence] = None,
                 rescale_with_baseline: bool = False,
                 baseline: Union[None, str, os.PathLike,
                                 Sequence[float]] = None,
                 device: Any = None):
        """`weights`: a HuggingFace state dict of a BERT or RoBERTa model (or a
        path to one saved with torch.save); a leading `roberta.` / `bert.` is
        stripped, keys the encoder does not read (pooler, LM head) are ignored.
        `tokenizer`: anything with `encode(str)` returning the ids with the
        special tokens in place -- a list, or an object with `.ids` as a
        `tokenizers.Tokenizer` returns.  `baseline`: (P, R, F), or the library's
        baseline file, read at row `num_layers`."""
        if not isinstance(weights, Mapping):
            weights = torch.load(weights, map_location='cpu', weights_only=True)
        self.dims = infer_dims(weights, num_layers, heads, model_type, pad_id,
                               layer_norm_eps)
        stripped, _ = strip_prefix(weights)
        self.weights = {
            key: value.detach().to('cpu', torch.float32)
            for key, value in stripped.items()
            if isinstance(value, torch.Tensor) and value.dtype.is_floating_point
            and (key.startswith('embeddings.') or key.startswith('encoder.'))
        }
        self.num_layers = self.dims['layers']
        self.tokenizer = tokenizer
        self.cls_id, self.sep_id, self.pad_id = cls_id, sep_id, pad_id
        # tokenizer.model_max_length of the library's models
        self.max_length = self.dims['max_positions'] - self.dims['position_offset']
        self.idf = idf
        self._idf_dict: Optional[Dict[int, float]] = None
        self.rescale_with_baseline = rescale_with_baseline
        self._baseline: Optional[torch.Tensor] = None
        if baseline is not None:
            if isinstance(baseline, (str, os.PathLike)):
                baseline = read_baseline(baseline, self.num_layers)
            if len(baseline) != 3:
                raise ValueError('baseline must be (P, R, F)')
            self._baseline = torch.tensor([float(b) for b in baseline])
        if rescale_with_baseline and self._baseline is None:
            raise ValueError('rescale_with_baseline needs baseline=(P, R, F) or '
                             'the path of a baseline file')
        self._device = None if device is None else torch.device(device)
        self._ctx: Optional[hip.BertContext] = None
        if idf_sents is not None:
            self.compute_idf(idf_sents)

    @property
    def baseline_vals(self) -> Optional[torch.Tensor]:
        return self._baseline

    def _context(self) -> hip.BertContext:
        device = hip.require_device(self._device or torch.device('cuda'))
        if self._ctx is None or self._ctx.device != device:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.BertContext(hip.BertDims(**self.dims), self.weights,
                                        device)
        return self._ctx

    # -- host side ------------------------------------------------------------------
    def tokens(self, sentence: str) -> Sequence[int]:
        """`tokenizer.encode(sentence.strip(), add_special_tokens=True,
        truncation=True, max_length=model_max_length)`; `[cls, sep]` for an
        empty sentence."""
        sentence = sentence.strip()
        if not sentence:
            return [self.cls_id, self.sep_id]
        ids = self.tokenizer.encode(sentence)
        ids = [int(i) for i in getattr(ids, 'ids', ids)]
        if len(ids) > self.max_length:
            ids = ids[:self.max_length - 1] + [self.sep_id]
        return ids

    def compute_idf(self, sents: StrSequence) -> None:
        """idf[t] = log((N + 1) / (df[t] + 1)) over the N sentences `sents`, df
        counting the sentences whose id set (specials included) holds t; ids
        never seen weigh log(N + 1)."""
        if self._idf_dict is not None:
            warnings.warn('Overwriting the previous importance weights.')
        counts: collections.Counter = collections.Counter()
        for sent in sents:
            counts.update(set(self.tokens(sent)))
        n = len(sents)
        table: Dict[int, float] = collections.defaultdict(
            lambda: math.log((n + 1) / 1))
        table.update({t: math.log((n + 1) / (c + 1)) for t, c in counts.items()})
        self._idf_dict = table

    def token_weight(self, token: int) -> float:
        if self.idf:
            if self._idf_dict is None:
                raise ValueError('idf=True: call compute_idf(sentences) before '
                                 'score (or pass idf_sents=)')
            return self._idf_dict[token]
        return 0. if token in (self.cls_id, self.sep_id) else 1.

    # -- the score --------------------------------------------------------------------
    def score(self,
              cands: StrSequence,
              refs: Sequence[Union[str, StrSequence]],
              batch_size: int = 64,
              _dedup: bool = True) -> Tuple[torch.Tensor, torch.Tensor,
                                            torch.Tensor]:
        """(P, R, F), each a float32 CPU tensor of len(cands).  `refs` holds one
        reference or a list of them per candidate; with several, P, R and F are
        each the largest over the references.  Every distinct sentence is
        encoded once, at most `batch_size` sentences per pass of the encoder."""
        if batch_size < 1:
            raise ValueError('batch_size must be at least 1')
        if len(cands) == 0:
            return (torch.zeros(0),) * 3
        sentences, ids, cand_of, ref_of, owner = self._prepare(cands, refs,
                                                               _dedup)
        lens = [len(i) for i in ids]
        ctx = self._context()
        device = ctx.device
        offsets = [0]
        for length in lens:
            offsets.append(offsets[-1] + length)
        total = offsets[-1]
        flat = torch.tensor([t for i in ids for t in i], dtype=torch.long)
        weight = torch.tensor([self.token_weight(t) for i in ids for t in i],
                              dtype=torch.float32)
        # batch-local offsets of every encoder pass, uploaded once
        spans, local = [], []
        for lo in range(0, len(sentences), batch_size):
            hi = min(len(sentences), lo + batch_size)
            spans.append((lo, hi, len(local)))
            local += [o - offsets[lo] for o in offsets[lo:hi + 1]]
        flat = flat.to(device)
        local_dev = torch.tensor(local, dtype=torch.int32).to(device)
        emb = torch.empty((total, self.dims['width']), device=device)
        for lo, hi, at in spans:
            ctx.encode(flat[offsets[lo]:offsets[hi]],
                       local_dev[at:at + hi - lo + 1], max(lens[lo:hi]),
                       normalize=True, out=emb[offsets[lo]:offsets[hi]])
        prf = ctx.score_pairs(emb, torch.tensor(offsets, dtype=torch.int32),
                              weight, torch.tensor(cand_of, dtype=torch.int32),
                              torch.tensor(ref_of, dtype=torch.int32))
        return self._combine(prf.cpu(), owner, len(cands))

    def _prepare(self, cands: StrSequence,
                 refs: Sequence[Union[str, StrSequence]], dedup: bool = True):
        """The host half of `score`: the distinct sentences (every occurrence
        when not `dedup`), their token ids, and per (candidate, reference)
        pair the two sentence numbers and the candidate it belongs to."""
        if len(cands) != len(refs):
            raise ValueError(f'{len(cands)} candidates, {len(refs)} references')
        refs = [[r] if isinstance(r, str) else list(r) for r in refs]
        if any(len(r) == 0 for r in refs):
            raise ValueError('every candidate needs at least one reference')
        sentences, index = [], {}

        def number(sentence: str) -> int:
            if dedup and sentence in index:
                return index[sentence]
            index[sentence] = len(sentences)
            sentences.append(sentence)
            return index[sentence]

        cand_of, ref_of, owner = [], [], []
        for i, (cand, cand_refs) in enumerate(zip(cands, refs)):
            for ref in cand_refs:
                cand_of.append(number(cand))
                ref_of.append(number(ref))
                owner.append(i)
        ids = [self.tokens(s) for s in sentences]
        for sentence, sentence_ids in zip(sentences, ids):
            if len(sentence_ids) > MAX_TOKENS:
                raise ValueError(
                    f'a sentence of {len(sentence_ids)} tokens exceeds the '
                    f'{MAX_TOKENS} this build supports (attention runs in LDS): '
                    f'{sentence!r}')
            if not (0 <= min(sentence_ids) and
                    max(sentence_ids) < self.dims['vocab_size']):
                raise IndexError('index out of range in self')  # nn.Embedding
        empty = {n for n, i in enumerate(ids) if len(i) <= 2}
        if empty & set(cand_of):
            warnings.warn('Warning: Empty candidate sentence detected; '
                          'setting raw BERTscores to 0.')
        if empty & set(ref_of):
            warnings.warn('Warning: Empty reference sentence detected; '
                          'setting raw BERTScores to 0.')
        return sentences, ids, cand_of, ref_of, owner

    def _combine(self, prf: torch.Tensor, owner: Sequence[int], count: int):
        """(pairs, 3) raw P, R, F -> per candidate and per field the largest
        over its references, then the baseline."""
        slot, seen = [], collections.Counter()
        for i in owner:
            slot.append(seen[i])
            seen[i] += 1
        best = torch.full((count, max(seen.values()), 3), -math.inf)
        best[torch.tensor(owner), torch.tensor(slot)] = prf.float()
        out = best.max(dim=1).values
        if self.rescale_with_baseline:
            out = (out - self._baseline) / (1 - self._baseline)
        return out[:, 0], out[:, 1], out[:, 2]

    def embed(self, sentences: StrSequence,
              normalize: bool = False) -> Sequence[torch.Tensor]:
        """Per sentence the (tokens, width) embeddings the score is built on
        (the last hidden state of the cut model), on the GPU."""
        ids = [self.tokens(s) for s in sentences]
        for sentence, sentence_ids in zip(sentences, ids):
            if len(sentence_ids) > MAX_TOKENS:
                raise ValueError(
                    f'a sentence of {len(sentence_ids)} tokens exceeds the '
                    f'{MAX_TOKENS} this build supports: {sentence!r}')
        if not ids:
            return ()
        ctx = self._context()
        lens = [len(i) for i in ids]
        offsets = torch.tensor([0] + lens).cumsum(0).to(torch.int32)
        flat = torch.tensor([t for i in ids for t in i], dtype=torch.long)
        out = ctx.encode(flat.to(ctx.device), offsets.to(ctx.device), max(lens),
                         normalize=normalize)
        return out.split(lens)


def models_dir() -> pathlib.Path:
    return pathlib.Path(os.environ.get('MILAN_MODELS_DIR') or
                        pathlib.Path.home() / '.cache' / 'milan_amd' / 'models')


def load(name_or_dir: Union[str, os.PathLike] = 'roberta-large',
         num_layers: Optional[int] = None,
         idf: bool = True,
         rescale_with_baseline: bool = True,
         device: Any = None,
         **kwargs: Any) -> BERTScorer:
    """The scorer the reference builds by default, from files on this machine:
    a HuggingFace-format directory (`name_or_dir` itself, or that name under
    `MILAN_MODELS_DIR`) holding `config.json`, the weights (`model.safetensors`
    or `pytorch_model.bin`), `tokenizer.json` and, for
    `rescale_with_baseline`, bert_score's baseline file as `<name>.tsv` or
    `baseline.tsv`.  Nothing is downloaded."""
    root = pathlib.Path(name_or_dir)
    if not root.is_dir():
        root = models_dir() / str(name_or_dir)
    wanted = ('config.json, model.safetensors or pytorch_model.bin, '
              'tokenizer.json' +
              (f', {root.name}.tsv (bert_score\'s rescale_baseline/en file)'
               if rescale_with_baseline else ''))
    if not root.is_dir():
        raise FileNotFoundError(
            f'no BERTScore model at {root}: put a HuggingFace-format directory '
            f'there ({wanted}), or set MILAN_MODELS_DIR to where it is. '
            'Nothing is downloaded.')

    def need(*names: str) -> pathlib.Path:
        for name in names:
            if (root / name).is_file():
                return root / name
        raise FileNotFoundError(
            f'{root} lacks {" or ".join(names)}; it must hold {wanted}')

    config = json.loads(need('config.json').read_text())
    path = need('model.safetensors', 'pytorch_model.bin')
    if path.suffix == '.safetensors':
        from safetensors.torch import load_file
        weights = load_file(str(path))
    else:
        weights = torch.load(path, map_location='cpu', weights_only=True)
    import tokenizers
    tokenizer = tokenizers.Tokenizer.from_file(str(need('tokenizer.json')))
    model_type = config.get('model_type')
    if model_type == 'roberta':
        cls, sep = '<s>', '</s>'
    else:
        cls, sep = '[CLS]', '[SEP]'
    if num_layers is None:
        num_layers = NUM_LAYERS.get(root.name)
        if num_layers is None:
            raise ValueError(f'pass num_layers= for {root.name}: only '
                             f'{sorted(NUM_LAYERS)} have a default')
    baseline = None
    if rescale_with_baseline:
        baseline = need(f'{root.name}.tsv', 'baseline.tsv')
    return BERTScorer(weights, tokenizer,
                      cls_id=tokenizer.token_to_id(cls),
                      sep_id=tokenizer.token_to_id(sep),
                      pad_id=config.get('pad_token_id'),
                      num_layers=num_layers,
                      heads=config.get('num_attention_heads'),
                      model_type=model_type,
                      layer_norm_eps=config.get('layer_norm_eps'),
                      idf=idf, rescale_with_baseline=rescale_with_baseline,
                      baseline=baseline, device=device, **kwargs)
