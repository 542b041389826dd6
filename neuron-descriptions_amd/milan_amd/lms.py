"""The LSTM language model used for PMI decoding / reranking, and its training.

Mirror of the reference's `src/milan/lms.py`: Embedding(V,E,padding_idx) ->
LSTM(layers, dropout) -> Linear(V) + LogSoftmax.
  * `forward(inputs, reduce=True)` = masked sequence log-probability with the
    reference's stop-mask off-by-one (lms.py:93-96); `logp(texts)` indexes
    text with start/stop/pad/unk first (lms.py:103-132).  Works attached to a
    Decoder (sharing its HIP context) or standalone.
  * `fit(dataset, ...)` (lms.py:134-265): NLLLoss(ignore_index=pad) training
    with the reference's split, shuffling, optimizer and early stopping.  The
    loss and every gradient come from libmilan_hip (`milan_lm_train_step`:
    exact fp32 MFMA, deterministic; include/milan_hip.h); the torch optimizer
    then steps the parameters.
  * `forward` in training mode is differentiable once the parameters ask
    for it: after `lm.requires_grad_(True); lm.train()` the call runs
    `TrainingForward` (`milan_lm_forward_train` and, on `backward()`,
    `milan_lm_backward`) with inter-layer dropout on, so the
    log-probs (`reduce=False`) and the sequence scores (`reduce=True`) carry
    `grad_fn` and a user's own loss or optimizer loop trains the LM.  The one
    difference from the reference, whose parameters are trainable by
    default: the parameters here are created with `requires_grad=False`, and
    while none of them requires grad every call runs the inference kernels
    (no dropout, no graph), in training mode too.
  * `lm(dataset, ...)` (lms.py:283-322) builds the indexer from the dataset's
    annotations and a model initialised as the reference's would be (same
    draws from torch's global generator).
Text needs a tokenizer: the reference's is spaCy, which is not in this build,
so `indexer.tokenize` (or `indexer_kwargs['tokenize']`) is any callable
str | [str] -> tokens | [tokens]; without one, NotImplementedError.
"""
from typing import (Any, List, Mapping, Optional, Sequence, Sized, Type,
                    Union, cast)

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn, optim
from torch.autograd.function import once_differentiable
from torch.utils import data

from milan_amd import hip, lang, params, training


def tagged_dropout_mask(seed: int, tag: int, rows: int, length: int,
                        units: int, p: float) -> torch.Tensor:
    """Host restatement of the training kernels' dropout mask (`keep` in
    csrc/train_common.h): (rows, length, units) bool, True = kept (kept values
    are scaled by 1 / (1 - p)).  A pure function of (seed, tag, row, t, unit);
    the tag tells the LM's layers and the decoder apart."""
    m64 = np.uint64(0xFFFFFFFFFFFFFFFF)

    def mix64(z):
        with np.errstate(over='ignore'):
            z = (z + np.uint64(0x9E3779B97F4A7C15)) & m64
            z = ((z ^ (z >> np.uint64(30))) *
                 np.uint64(0xBF58476D1CE4E5B9)) & m64
            z = ((z ^ (z >> np.uint64(27))) *
                 np.uint64(0x94D049BB133111EB)) & m64
            return z ^ (z >> np.uint64(31))

    b = np.arange(rows, dtype=np.uint64)[:, None, None]
    t = np.arange(length, dtype=np.uint64)[None, :, None]
    j = np.arange(units, dtype=np.uint64)[None, None, :]
    key = ((np.uint64(tag) << np.uint64(56)) | (b << np.uint64(32)) |
           (t << np.uint64(16)) | j)
    z = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64(key))
    threshold = int(float(np.float32(p)) * 16777216.0)
    return torch.from_numpy((z >> np.uint64(40)) >= np.uint64(threshold))


DECODER_DROPOUT_TAG = 0xDC  # the decoder's mask, never one of the LM's layers


def dropout_mask(seed: int, layer: int, rows: int, length: int, units: int,
                 p: float) -> torch.Tensor:
    """The mask on the output of LSTM layer `layer` of the LM (tag = layer);
    see milan_lm_train_step in include/milan_hip.h."""
    return tagged_dropout_mask(seed, layer, rows, length, units, p)


def decoder_dropout_mask(seed: int, rows: int, length: int, units: int,
                         p: float) -> torch.Tensor:
    """The mask on the decoder's h before the output Linear (tag 0xDC); see
    milan_decoder_train_step in include/milan_hip.h."""
    return tagged_dropout_mask(seed, DECODER_DROPOUT_TAG, rows, length, units,
                               p)


class _SequenceDataset(data.Dataset):
    """The annotations of a dataset, one sample per sequence (a sample's
    annotation may be a str or a list of str; reference lms.py:176-200)."""

    def __init__(self, dataset: data.Dataset, annotation_index: int = 4):
        self.sequences: List[str] = []
        for index in range(len(cast(Sized, dataset))):
            annotation = dataset[index][annotation_index]
            if isinstance(annotation, str):
                self.sequences.append(annotation)
            else:
                self.sequences += annotation

    def __getitem__(self, index: int) -> str:
        return self.sequences[index]

    def __len__(self) -> int:
        return len(self.sequences)


class TrainingForward(torch.autograd.Function):
    """The LM with inter-layer dropout as one autograd node:
    `milan_lm_forward_train` / `milan_lm_backward` (include/milan_hip.h).
    Inputs: the dims-only hip.Context, inputs (rows, L), targets (rows, L) or
    None, dropout, seed and the 4 * layers + 3 parameters in state-dict order.
    Output: without targets the log-probs (rows, L, V); with targets only
    picked[r, t] = logprobs[r, t, targets[r, t]], (rows, L) -- no (rows, L, V)
    tensor then exists in either direction.  The forward's workspace holds
    every activation and the backward overwrites them in place, so the graph
    supports one backward."""

    @staticmethod
    def forward(ctx, hctx, inputs, targets, dropout, seed, *params):
        logprobs, picked, ws = hctx.lm_forward_train(
            params, inputs, dropout, seed, targets=targets,
            want_logprobs=targets is None)
        ctx.hctx, ctx.dropout, ctx.seed, ctx.ws = hctx, dropout, seed, ws
        ctx.inputs, ctx.targets = inputs, targets
        ctx.save_for_backward(*params)
        ctx.set_materialize_grads(False)
        return logprobs if targets is None else picked

    @staticmethod
    @once_differentiable
    def backward(ctx, upstream):
        if upstream is None:
            return (None,) * (5 + len(ctx.saved_tensors))
        ws, ctx.ws = ctx.ws, None
        if ws is None:
            raise RuntimeError(
                'the training-mode LM graph was already backpropagated once: '
                'its activations are consumed by the first backward; run the '
                'forward again')
        params = ctx.saved_tensors
        grads = [torch.empty_like(p) for p in params]
        upstream = upstream.contiguous()
        picked = ctx.targets is not None
        ctx.hctx.lm_backward(params, grads, ctx.inputs, ctx.dropout, ctx.seed,
                             None if picked else upstream,
                             upstream if picked else None, ctx.targets, ws)
        # (the kernels compute them all; torch accumulates the ones asked for)
        pgrads = [g if need else None
                  for g, need in zip(grads, ctx.needs_input_grad[5:])]
        return (None, None, None, None, None, *pgrads)


class LanguageModel(nn.Module):
    """Parameter owner + HIP entry point for the LM."""

    def __init__(self,
                 indexer: lang.Indexer,
                 embedding_size: int = 128,
                 hidden_size: int = 512,
                 layers: int = 2,
                 dropout: float = .5):
        super().__init__()
        self.indexer = indexer
        self.embedding_size = embedding_size
        self.hidden_size = hidden_size
        self.layers = layers
        self.dropout = dropout
        f = torch.float32
        v, e, h = len(indexer), embedding_size, hidden_size
        spec = {'embedding.weight': ((v, e), f)}
        for layer in range(layers):
            spec[f'lstm.weight_ih_l{layer}'] = ((4 * h, e if layer == 0 else h),
                                                f)
            spec[f'lstm.weight_hh_l{layer}'] = ((4 * h, h), f)
            spec[f'lstm.bias_ih_l{layer}'] = ((4 * h,), f)
            spec[f'lstm.bias_hh_l{layer}'] = ((4 * h,), f)
        spec['output.0.weight'] = ((v, h), f)
        spec['output.0.bias'] = ((v,), f)
        params.build(spec, root=self)
        # inside a Decoder the LM scores through the decoder's HIP context (one
        # packed copy of the weights); on its own it builds an LM-only context
        self._owner = None
        self._ctx: Optional[hip.Context] = None
        self._ctx_key = None
        self._train_ctx: Optional[hip.Context] = None  # training-mode forward
        self._train_ctx_key = None

    def _context(self) -> hip.Context:
        if self._owner is not None and self._owner() is not None:
            return self._owner()._context()
        device = hip.require_device(self.embedding.weight.device)
        key = (device, tuple(p._version for p in self.parameters()))
        if self._ctx is None or self._ctx_key != key:
            sd = {f'lm.{k}': v for k, v in self.state_dict().items()}
            dims = hip.make_dims(sd, len(self.indexer.vocab))
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.Context(dims, sd, device)
            self._ctx_key = key
        return self._ctx

    def forward(self,
                inputs: torch.Tensor,
                reduce: bool = False,
                masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Log-probabilities under the LM (reference lms.py:58-101).

        `reduce=False`: (batch, length, vocab) next-token log-probs at every
        position.  `reduce=True`: (batch,) sequence log-probs, the first token
        taken as given; `masks` (batch, length-1) weights the token terms, by
        default everything after the first stop token is dropped -- with the
        reference's off-by-one: the term predicting the token AFTER the stop
        still counts (lms.py:93-95).

        In training mode with at least one parameter requiring grad (they do
        not by default: `lm.requires_grad_(True)`) the result carries
        `grad_fn` and inter-layer dropout is on; see `_forward_train`.
        """
        if self.training and any(p.requires_grad for p in self.parameters()):
            return self._forward_train(inputs, reduce, masks)
        ctx = self._context()
        if reduce and masks is None:
            return ctx.lm_score(inputs)  # fused: never materialises (B,L,V)
        lps = ctx.lm_logprobs(inputs)
        if not reduce:
            return lps
        targets = inputs[:, 1:].to(lps.device)
        picked = lps[:, :-1].gather(2, targets.unsqueeze(-1)).squeeze(-1)
        return picked.mul(masks.to(lps.device)).sum(dim=-1)

    def _train_context(self, device: torch.device) -> hip.Context:
        """A context that only carries the LM's dims, never finalized, cached
        on the LM (attached to a Decoder or not): the training calls read the
        live parameters, so optimizer steps do not rebuild it."""
        key = (device, tuple(p.shape for p in self.parameters()))
        if self._train_ctx is None or self._train_ctx_key != key:
            sd = {f'lm.{k}': v for k, v in self.state_dict().items()}
            # (the old one closes when the last graph that holds it goes)
            self._train_ctx = hip.Context(
                hip.make_dims(sd, len(self.indexer.vocab)), {}, device,
                finalize=False)
            self._train_ctx_key = key
        return self._train_ctx

    def _forward_train(self, inputs: torch.Tensor, reduce: bool,
                       masks: Optional[torch.Tensor]) -> torch.Tensor:
        """`forward` through `TrainingForward` (reference lms.py:85-101 with
        nn.LSTM's dropout on): dropout `self.dropout` on the output of every
        layer but the last, its seed drawn from the device's generator when
        there is a mask to draw (dropout > 0 and more than one layer).
        `reduce=True` asks the kernels for the log-probs of the next tokens
        alone; the mask and the sum over positions are torch's, and `masks` is
        a constant.  Under `torch.no_grad()` this is still the training
        forward, and nothing is kept."""
        if masks is not None and masks.requires_grad:
            raise ValueError('masks is a constant of the training-mode forward: '
                             'no gradient flows into it (detach it)')
        if inputs.dim() != 2:
            raise ValueError(f'inputs must be 2D, got {inputs.dim()}')
        device = hip.require_device(self.embedding.weight.device)
        named = dict(self.named_parameters())
        weights = [named[name] for name in self._param_names()]
        seed = 0
        if self.dropout > 0 and self.layers > 1:  # as fit draws it
            seed = int(torch.randint(
                2**62, (), device=device,
                generator=torch.cuda.default_generators[device.index]))
        hctx = self._train_context(device)
        inputs = inputs.to(device, torch.long).contiguous()
        if not reduce:
            return TrainingForward.apply(hctx, inputs, None,
                                         float(self.dropout), seed, *weights)
        # position t predicts inputs[:, t + 1]; the last one predicts nothing
        # (any id does there: its term is cut off below)
        targets = F.pad(inputs[:, 1:], (0, 1))
        picked = TrainingForward.apply(hctx, inputs, targets,
                                       float(self.dropout), seed, *weights)
        if masks is None:
            # ones up to AND INCLUDING the term after the first stop token
            stopped = inputs.eq(self.indexer.stop_index).cumsum(dim=1).gt(0)
            masks = torch.ones_like(picked[:, :-1])
            masks[:, 1:] = (~stopped[:, :-2]).to(masks.dtype)
        return picked[:, :-1].mul(masks.to(device)).sum(dim=-1)

    def reset_parameters(self) -> None:
        """Initialise the parameters as the reference's torch modules do
        (the constructor leaves them zero): nn.Embedding, nn.LSTM and
        nn.Linear are built in the reference's order, so the draws from
        torch's global generator are the same."""
        v, e, h = len(self.indexer), self.embedding_size, self.hidden_size
        embedding = nn.Embedding(v, e, padding_idx=self.indexer.pad_index)
        lstm = nn.LSTM(input_size=e,
                       hidden_size=h,
                       num_layers=self.layers,
                       dropout=self.dropout,
                       batch_first=True)
        output = nn.Linear(h, v)
        state = {'embedding.weight': embedding.weight}
        state.update({f'lstm.{k}': t for k, t in lstm.state_dict().items()})
        state.update({'output.0.weight': output.weight,
                      'output.0.bias': output.bias})
        with torch.no_grad():
            self.load_state_dict(state)

    def logp(self,
             sequences: Sequence[str],
             device: Optional[Any] = None) -> torch.Tensor:
        """Log probability of each text (reference lms.py:103-132): indexed
        with start / stop / pad / unk, then `forward(reduce=True)`."""
        if device is not None:
            self.to(device)
        self.eval()
        inputs = torch.tensor(self.indexer(sequences,
                                           start=True,
                                           stop=True,
                                           pad=True,
                                           unk=True))
        with torch.no_grad():
            return self(inputs, reduce=True)

    # -- training (reference lms.py:134-265) -----------------------------------
    def _param_names(self) -> List[str]:
        names = ['embedding.weight']
        for layer in range(self.layers):
            names += [f'lstm.{kind}_l{layer}' for kind in
                      ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
        return names + ['output.0.weight', 'output.0.bias']

    def fit(self,
            dataset: data.Dataset,
            annotation_index: int = 4,
            batch_size: int = 128,
            max_epochs: int = 100,
            patience: int = 4,
            hold_out: Union[float, Sequence[int]] = .1,
            optimizer_t: Type[optim.Optimizer] = optim.AdamW,
            optimizer_kwargs: Optional[Mapping[str, Any]] = None,
            device: Optional[Any] = None,
            display_progress_as: Optional[str] = 'train lm') -> None:
        """Train on the annotations of `dataset` (reference lms.py:134-265).

        Same loop as the reference: hold-out split (`random_split` on torch's
        global generator, or `fixed_split(hold_out)`), shuffled training
        batches, `optimizer_t(self.parameters(), **optimizer_kwargs)`,
        NLLLoss(ignore_index=pad), early stopping on the validation loss.
        The loss and gradients of a batch come from `milan_lm_train_step`
        (train mode, dropout masks seeded from the device's torch generator)
        and are written into `p.grad`; the torch optimizer then steps.
        Validation uses `milan_lm_nll` (eval mode).  As in the reference,
        the "best" state kept for the restore on stop is `state_dict()`,
        whose tensors share storage with the parameters: the model ends with
        the parameters of the last epoch run.
        """
        if optimizer_kwargs is None:
            optimizer_kwargs = {}
        if device is not None:
            self.to(device)
        device = hip.require_device(self.embedding.weight.device)

        sequences = _SequenceDataset(dataset,
                                     annotation_index=annotation_index)
        if isinstance(hold_out, float):
            train, val = training.random_split(sequences, hold_out=hold_out)
        else:
            train, val = training.fixed_split(sequences, hold_out)
        train_loader = data.DataLoader(train,
                                       batch_size=batch_size,
                                       shuffle=True)
        val_loader = data.DataLoader(val, batch_size=batch_size)

        optimizer = optimizer_t(self.parameters(), **optimizer_kwargs)
        stopper = training.EarlyStopping(patience=patience)

        # an LM-dims context that is never finalized: the training calls read
        # the live parameters, so optimizer steps never rebuild it
        sd = {f'lm.{k}': v for k, v in self.state_dict().items()}
        ctx = hip.Context(hip.make_dims(sd, len(self.indexer.vocab)), {},
                          device, finalize=False)
        named = dict(self.named_parameters())
        weights = [named[name] for name in self._param_names()]
        grads = [torch.empty_like(p) for p in weights]
        cuda_generator = torch.cuda.default_generators[device.index]

        def batch(texts):
            inputs = torch.tensor(self.indexer(texts,
                                               start=True,
                                               stop=False,
                                               pad=True,
                                               unk=True))
            targets = torch.tensor(self.indexer(texts,
                                                start=False,
                                                stop=True,
                                                pad=True,
                                                unk=True))
            return inputs, targets

        def mean(loss: torch.Tensor) -> float:
            return (loss[0] / loss[1]).item()

        progress = range(max_epochs)
        if display_progress_as is not None:
            try:
                from tqdm.auto import tqdm
                progress = tqdm(progress, desc=display_progress_as)
            except ImportError:
                pass

        best = self.state_dict()
        for _ in progress:
            self.train()
            train_loss = 0.
            for texts in train_loader:
                inputs, targets = batch(texts)
                seed = 0
                if self.training and self.dropout > 0:
                    seed = int(torch.randint(2**62, (), device=device,
                                             generator=cuda_generator))
                dropout = self.dropout if self.training else 0.
                loss = ctx.lm_train_step(weights, grads, inputs, targets,
                                         dropout, seed)
                for p, g in zip(weights, grads):
                    p.grad = g
                optimizer.step()
                optimizer.zero_grad()
                train_loss += mean(loss)
            train_loss /= len(train_loader)

            self.eval()
            val_loss = 0.
            for texts in val_loader:
                inputs, targets = batch(texts)
                val_loss += mean(ctx.lm_nll(weights, inputs, targets))
            val_loss /= len(val_loader)

            if not isinstance(progress, range):
                progress.set_description(f'{display_progress_as} '
                                         f'[train_loss={train_loss:.3f}, '
                                         f'val_loss={val_loss:.3f}]')

            if stopper(val_loss):
                self.load_state_dict(best)
                break

            if stopper.improved:
                best = self.state_dict()
        ctx.close()

    def properties(self) -> Mapping[str, Any]:
        return {
            'indexer': self.indexer,
            'embedding_size': self.embedding_size,
            'hidden_size': self.hidden_size,
            'layers': self.layers,
            'dropout': self.dropout,
        }


def lm(dataset: data.Dataset,
       annotation_index: int = 4,
       indexer_kwargs: Optional[Mapping[str, Any]] = None,
       **kwargs: Any) -> LanguageModel:
    """A LanguageModel for the annotations of `dataset` (reference
    lms.py:283-322): each sample's annotations are joined with `lang.join`,
    the indexer is built from them (`start`, `stop`, `pad`, `unk` default to
    True; `tokenize` must be given, see the module docstring) and **kwargs go
    to the constructor.  The parameters are initialised as the reference's
    torch modules initialise theirs, with the same draws from torch's global
    generator."""
    indexer_kwargs = dict(indexer_kwargs or {})
    annotations = [
        lang.join(dataset[index][annotation_index])
        for index in range(len(cast(Sized, dataset)))
    ]
    for key in ('start', 'stop', 'pad', 'unk'):
        indexer_kwargs.setdefault(key, True)
    indexer = lang.indexer(annotations, **indexer_kwargs)
    model = LanguageModel(indexer, **kwargs)
    model.reset_parameters()
    return model
