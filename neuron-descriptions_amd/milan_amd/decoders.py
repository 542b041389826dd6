"""`src.milan.Decoder` on MI355X: same Python surface, HIP arithmetic.

Reference: `src/milan/decoders.py` -- `Decoder` (:224), `forward` (:335-523),
`encode` (:525-546), `init_state` (:548-574), `step` (:576-634), `predict`
(:809-871), `DecoderState/Step/Output` (:84-150), `STRATEGY_*` (:217-221),
serialisation (:1072-1109).  A script written against the reference (e.g.
`scripts/compute_milan_descriptions.py:52-63`) runs unchanged after
`from milan_amd import ...`.

What differs by design:
  * every tensor op is a call into libmilan_hip (see `hip.py`); there is no
    torch / CPU fallback -- without a GPU or the .so the calls raise;
  * inputs may be the reference's float tensors or raw uint8 exemplars
    (kept uint8 all the way to the GPU: 4x less host memory and PCIe traffic);
  * `predict` processes `chunk_size` neurons per launch instead of 16, but
    evaluates allennlp's early-exit length T' per group of `batch_size`
    neurons, so captions / rerank choices equal the reference's batch-16 run;
  * `score` and `strategy='sample'` are built on the same kernels (the
    tokenizer of `score` is any callable: spaCy is not in this image);
  * `fit` (:873-1070) trains the decoder with the reference's loop; the loss
    and gradients of a batch come from `milan_decoder_train_step` (exact fp32,
    deterministic; include/milan_hip.h), the torch optimizer steps.
    `decoder()` (:1214-1259) builds a seeded, reference-initialised model;
    `bleu` scores with `metrics.bleu`, a pure-Python restatement of
    sacrebleu 1.5.1's corpus BLEU;
  * `forward` in training mode with a tensor strategy (teacher forcing) is
    differentiable: `TeacherForced` runs `milan_decoder_forward_train` and,
    on `backward()`, `milan_decoder_backward`, so
    predictions, attentions and scores carry `grad_fn` and a user's own loss,
    optimizer loop or torch `Encoder` trains through it.  The decoder's 19
    own tensors require grad, as the reference's modules do;
  * out of scope: training-mode greedy / sample /
    beam decoding (raises NotImplementedError), `rouge` (needs rouge);
  * `bert_score` scores with `metrics.bert_score`: the encoder and the token
    matching run in HIP (milan_amd.bertscore);
  * `DecoderWithCLIP` reranks the beam with CLIP (milan_amd.rerankers: both
    towers in HIP);
  * `beam_size` goes up to min(vocabulary, 1024) -- `DecoderWithCLIP`'s default
    of 1000 runs as it stands; beyond that the library raises ValueError naming
    `beam_size=`.  Nothing is clamped here.
"""
import os
import weakref
from typing import (Any, Dict, Mapping, NamedTuple, Optional, Sequence, Sized,
                    Tuple, Type, Union, cast)

import torch
from torch import nn, optim
from torch.autograd.function import once_differentiable
from torch.utils import data

from milan_amd import (encoders, hip, lang, lms, metrics, params, rerankers,
                       serialize, training)

Strategy = Union[torch.Tensor, str]

STRATEGY_GREEDY = 'greedy'
STRATEGY_SAMPLE = 'sample'
STRATEGY_BEAM = 'beam'
STRATEGY_RERANK = 'rerank'
STRATEGIES = (STRATEGY_GREEDY, STRATEGY_SAMPLE, STRATEGY_BEAM, STRATEGY_RERANK)
# the decoder's own state dict in the reference's order: what Decoder.fit
# trains (milan_decoder_train_step's parameter list)
TRAIN_PARAMS = (
    'init_h.0.weight', 'init_h.0.bias', 'init_c.0.weight', 'init_c.0.bias',
    'embedding.weight', 'attend.query_to_hidden.weight',
    'attend.query_to_hidden.bias', 'attend.key_to_hidden.weight',
    'attend.key_to_hidden.bias', 'attend.output.0.weight',
    'attend.output.0.bias', 'feature_gate.0.weight', 'feature_gate.0.bias',
    'lstm.weight_ih', 'lstm.weight_hh', 'lstm.bias_ih', 'lstm.bias_hh',
    'output.1.weight', 'output.1.bias')
_HIP_STRATEGY = {
    STRATEGY_GREEDY: hip.GREEDY,
    STRATEGY_BEAM: hip.BEAM,
    STRATEGY_RERANK: hip.RERANK
}


class DecoderState(NamedTuple):
    """reference decoders.py:84-99."""
    h: torch.Tensor
    c: torch.Tensor
    h_lm: Optional[torch.Tensor]
    c_lm: Optional[torch.Tensor]


class DecoderStep(NamedTuple):
    """reference decoders.py:102-117."""
    predictions: torch.Tensor
    attentions: torch.Tensor
    state: DecoderState


class DecoderOutput(NamedTuple):
    """reference decoders.py:120-150 (field order matters: captions, scores,
    tokens; DecoderWithCLIP splats outputs[3:])."""
    captions: Sequence[str]
    scores: torch.Tensor
    tokens: torch.Tensor
    predictions: Optional[torch.Tensor]
    attentions: Optional[torch.Tensor]
    beam_captions: Optional[Sequence[Sequence[str]]]
    beam_scores: Optional[torch.Tensor]
    beam_tokens: Optional[torch.Tensor]


class Attention(params.ParamTree):
    """Weights of reference `Attention` (decoders.py:29-81)."""

    def __init__(self,
                 query_size: int,
                 key_size: int,
                 hidden_size: Optional[int] = None):
        super().__init__()
        self.query_size = query_size
        self.key_size = key_size
        self.hidden_size = hidden_size or min(query_size, key_size)
        f = torch.float32
        a = self.hidden_size
        params.build(
            {
                'query_to_hidden.weight': ((a, query_size), f),
                'query_to_hidden.bias': ((a,), f),
                'key_to_hidden.weight': ((a, key_size), f),
                'key_to_hidden.bias': ((a,), f),
                'output.0.weight': ((1, a), f),
                'output.0.bias': ((1,), f),
            },
            root=self)


class TeacherForced(torch.autograd.Function):
    """Teacher-forced decoder with dropout as one autograd node:
    `milan_decoder_forward_train` / `milan_decoder_backward`
    (include/milan_hip.h).  Inputs: the dims-only hip.Context, targets (rows,
    L), dropout, seed, features (rows, k, F) and the 19 TRAIN_PARAMS tensors;
    outputs: log-probs (rows, L, V) and attentions (rows, L, k).  The
    forward's workspace holds every activation and the backward overwrites
    them in place, so the graph supports one backward."""

    @staticmethod
    def forward(ctx, hctx, targets, dropout, seed, features, *params):
        logprobs, attentions, ws = hctx.decoder_forward_train(
            params, features, targets, dropout, seed)
        ctx.hctx, ctx.dropout, ctx.seed, ctx.ws = hctx, dropout, seed, ws
        ctx.save_for_backward(targets, features, *params)
        ctx.set_materialize_grads(False)
        return logprobs, attentions

    @staticmethod
    @once_differentiable
    def backward(ctx, dlogprobs, dattentions):
        ws, ctx.ws = ctx.ws, None
        if ws is None:
            raise RuntimeError(
                'the teacher-forced decoder graph was already backpropagated '
                'once: its activations are consumed by the first backward; run '
                'the forward again')
        targets, features, *params = ctx.saved_tensors
        dfeatures = (torch.empty_like(features)
                     if ctx.needs_input_grad[4] else None)
        grads = [torch.empty_like(p) for p in params]
        contig = [None if g is None else g.contiguous()
                  for g in (dlogprobs, dattentions)]
        ctx.hctx.decoder_backward(params, grads, features, targets,
                                  ctx.dropout, ctx.seed, *contig, dfeatures, ws)
        # (the kernels compute all 19; torch accumulates the ones asked for)
        pgrads = [g if need else None
                  for g, need in zip(grads, ctx.needs_input_grad[5:])]
        return (None, None, None, None, dfeatures, *pgrads)


class Decoder(nn.Module):
    """Neuron caption decoder (reference decoders.py:224)."""

    def __init__(self,
                 indexer: lang.Indexer,
                 encoder: encoders.Encoder,
                 lm: Optional[lms.LanguageModel] = None,
                 embedding_size: int = 128,
                 hidden_size: int = 512,
                 attention_hidden_size: Optional[int] = None,
                 dropout: float = .5,
                 length: int = 15,
                 strategy: Optional[str] = None,
                 temperature: float = .2,
                 beam_size: int = 50,
                 share_images: bool = False):
        super().__init__()
        if lm is not None:
            mine, theirs = indexer.vocab.unique, lm.indexer.vocab.unique
            if mine != theirs:
                raise ValueError('lm and decoder have different vocabs;'
                                 f'lm missing {mine - theirs} and '
                                 f'decoder missing {theirs - mine}')
        if strategy is None:
            strategy = STRATEGY_BEAM if lm is None else STRATEGY_RERANK
        self.indexer = indexer
        self.encoder = encoder
        self.lm = lm
        self.embedding_size = embedding_size
        self.hidden_size = hidden_size
        self.attention_hidden_size = attention_hidden_size
        self.dropout = dropout
        self.length = length
        self.strategy = strategy
        self.temperature = temperature
        self.beam_size = beam_size
        # neurons per HIP launch in predict(): 640 x beam 50 = 32 000 decoder
        # rows fill whole rounds of GEMM tiles (+2.6 % over 256, measured) and
        # take 154 GB of activation workspace; lower it on a shared GPU
        self.chunk_size = 640
        # 'f32' (exact fp32 MFMA, the reference's arithmetic), 'split_f16'
        # (3 x f16 MFMA on (hi,lo) operand pairs: fp32-class error, ~2.9x
        # faster; raises FloatingPointError if an activation leaves its range) or
        # 'auto' (split_f16, and a call that saturates is rerun in f32 with a
        # RuntimeWarning); see DESIGN.md section 4.2.  The default since round 6
        # is 'auto' -- the mode the published throughput belongs to, with the
        # loud fallback -- and MILAN_PRECISION overrides it.  Every guarded call
        # reads the device status word back (one stream synchronisation per
        # forward / encode; MILAN_ON_SATURATION=ignore skips it).
        import os
        self.precision = os.environ.get('MILAN_PRECISION', 'auto')
        # replay each distinct decode pass from a captured hipGraph (helps
        # only launch-bound small batches; see hip.Context.enable_graphs)
        self.use_graphs = os.environ.get('MILAN_GRAPHS', '0') == '1'
        # exemplar slots of one encoder pass that hold the same uint8 image share one
        # trunk pass (hip.Context.set_image_sharing; same bits, opt-in: how often real
        # exemplar sets repeat an image inside a chunk is not measured).  Not a
        # property of the model: `properties()` and checkpoints do not carry it.
        self.share_images = bool(share_images)

        f = torch.float32
        fs, hs, es, v = (self.feature_size, hidden_size, embedding_size,
                         self.vocab_size)
        params.build(
            {
                'init_h.0.weight': ((hs, fs), f),
                'init_h.0.bias': ((hs,), f),
                'init_c.0.weight': ((hs, fs), f),
                'init_c.0.bias': ((hs,), f),
                'embedding.weight': ((v, es), f),
                'feature_gate.0.weight': ((fs, hs), f),
                'feature_gate.0.bias': ((fs,), f),
                'lstm.weight_ih': ((4 * hs, es + fs), f),
                'lstm.weight_hh': ((4 * hs, hs), f),
                'lstm.bias_ih': ((4 * hs,), f),
                'lstm.bias_hh': ((4 * hs,), f),
                'output.1.weight': ((v, hs), f),
                'output.1.bias': ((v,), f),
            },
            root=self)
        self.attend = Attention(hidden_size,
                                fs,
                                hidden_size=attention_hidden_size)
        # the decoder's own tensors are trainable, as the reference's torch
        # modules are (the training-mode forward differentiates them; every
        # other path computes in HIP without autograd)
        for p in self._train_params():
            p.requires_grad_(True)
        if lm is not None:
            lm._owner = weakref.ref(self)
        self._ctx: Optional[hip.Context] = None
        self._ctx_key = None
        self._train_ctx: Optional[hip.Context] = None  # training-mode forward
        self._train_ctx_key = None
        self.eval()  # hubs.py:130 hands out models in eval mode

    # -- reference properties -------------------------------------------------
    @property
    def feature_size(self) -> int:
        return self.encoder.feature_shape[-1]

    @property
    def vocab_size(self) -> int:
        return len(self.indexer)

    @property
    def device(self) -> torch.device:
        return self.embedding.weight.device

    # -- HIP context -------------------------------------------------------------
    def _has_hip_encoder(self) -> bool:
        return isinstance(self.encoder, encoders.PyramidConvEncoder)

    def _context(self) -> hip.Context:
        """(Re)build the packed-weight context when device or weights change."""
        device = hip.require_device(self.device)
        key = (device, tuple(p._version for p in self.parameters()),
               tuple(b._version for b in self.buffers()))
        if self._ctx is None or self._ctx_key != key:
            sd = dict(self.state_dict())
            blocks = (3, 4, 23, 3)
            if self._has_hip_encoder():
                blocks = self.encoder.blocks
            else:  # foreign Encoder subclass: only decoder weights go native
                sd = {k: v for k, v in sd.items() if not k.startswith('encoder.')}
            dims = hip.make_dims(sd, len(self.indexer.vocab), blocks=blocks)
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.Context(dims, sd, device)
            self._ctx_key = key
        # 'auto' = split_f16 that falls back to f32 for a call whose activations left
        # the split format's range (hip.Context._guarded); otherwise saturation raises
        want = 'split_f16' if self.precision == 'auto' else self.precision
        if self._ctx.precision != want:
            self._ctx.set_precision(want)
        # (MILAN_ON_SATURATION, when set, wins: 'ignore' = no status read-back per call)
        import os
        self._ctx.on_saturation = os.environ.get(
            'MILAN_ON_SATURATION', 'f32' if self.precision == 'auto' else 'raise')
        if bool(getattr(self._ctx, '_graphs', False)) != bool(self.use_graphs):
            self._ctx.enable_graphs(self.use_graphs)
        self._apply_share_images(self._ctx)
        return self._ctx

    def _apply_share_images(self, ctx) -> None:
        """`self.share_images` -> the context's flag (MILAN_SHARE_IMAGES, read when the
        context was created, stays on when the attribute is left at its default)."""
        import os
        want = bool(self.share_images) or bool(
            int(os.environ.get('MILAN_SHARE_IMAGES') or 0))
        if bool(ctx.image_sharing) != want:
            ctx.set_image_sharing(want)

    def calibrate(self, images: torch.Tensor, headroom: float = 8.0) -> int:
        """Choose the split-f16 trunk's activation scale from a sample of exemplar
        images ((M,3,H,W) or (N,k,3,H,W), uint8 or float): the trunk runs once in the
        exact-fp32 mode, the largest |activation| of any tensor it stores is observed,
        and the scale becomes the largest power of two that leaves `headroom` x that
        maximum below the f16 range.  The decoder's feature and embedding scales follow by
        the same rule, from the largest feature of the sample and the largest entry of the
        embedding tables (`hip.Context.calibrate`).  Returns log2 of the activation scale.
        Not in the reference (its fp32 needs none); with the default scale 2^5 activations beyond 2047 raise
        FloatingPointError instead of being clamped silently."""
        if not self._has_hip_encoder():
            raise ValueError('calibrate() needs the native pyramid encoder')
        if images.dim() == 5:
            images = images.reshape(-1, *images.shape[2:])
        return self._context().calibrate(images, headroom)

    # -- forward -------------------------------------------------------------------
    def forward(self,
                images_or_features: torch.Tensor,
                masks: Optional[torch.Tensor] = None,
                encode: Optional[bool] = None,
                length: Optional[int] = None,
                strategy: Optional[Strategy] = None,
                mi: Optional[bool] = None,
                temperature: Optional[float] = None,
                beam_size: Optional[int] = None,
                group_size: Optional[int] = None) -> DecoderOutput:
        """Decode captions for top images + masks (reference :335-523).

        `group_size` (extension, default = the whole batch like the
        reference): neurons per allennlp early-exit group, see `predict`.
        """
        if encode is None:
            encode = masks is not None
        if length is None:
            length = self.length
        if strategy is None:
            strategy = self.strategy
        if mi is None:
            mi = self.lm is not None and not self.training
            mi &= not isinstance(strategy, str) or strategy != STRATEGY_RERANK
        if temperature is None:
            temperature = self.temperature
        if beam_size is None:
            beam_size = self.beam_size
        batch_size = len(images_or_features)

        # Validate arguments (reference :395-409).
        if mi and isinstance(strategy, str) and strategy == STRATEGY_RERANK:
            raise ValueError('cannot set `mi=` decoding when reranking')
        rerank = isinstance(strategy, str) and strategy == STRATEGY_RERANK
        if (mi or rerank) and self.lm is None:
            raise ValueError('cannot use MI/rerank decoding without an LM')
        if (mi or rerank) and self.training:
            raise ValueError('cannot use MI/rerank decoding while training')
        if isinstance(strategy, str) and strategy not in STRATEGIES:
            raise ValueError(f'unknown strategy: {strategy}')
        if isinstance(strategy, torch.Tensor):
            if strategy.dim() != 2:
                raise ValueError(f'strategy must be 2D, got {strategy.dim()}')
            if strategy.shape[-1] != length:
                raise ValueError(f'strategy must have length {length}, '
                                 f'got {strategy.shape[-1]}')
            if strategy.shape[0] != batch_size:
                raise ValueError('strategy must have one row per sample, got '
                                 f'{strategy.shape[0]} for batch {batch_size}')
            if strategy.numel() and (int(strategy.min()) < 0 or
                                     int(strategy.max()) >= self.vocab_size):
                raise IndexError('index out of range in self')  # nn.Embedding
        if self.training:
            if not isinstance(strategy, torch.Tensor):
                raise NotImplementedError(
                    'training-mode forward (dropout active) is built for '
                    'teacher forcing (a tensor strategy) only; call .eval() '
                    'to decode -- milan.pretrained() returns eval-mode models')
            return self._forward_train(images_or_features, masks, encode,
                                       strategy)

        if isinstance(strategy, str) and strategy == STRATEGY_SAMPLE:
            return self._sample(images_or_features, masks, encode, length, mi,
                                temperature)

        ctx = self._context()
        forced = None
        if isinstance(strategy, torch.Tensor):  # teacher forcing (:444-445)
            hip_strategy, forced = hip.FORCED, strategy
        else:
            hip_strategy = _HIP_STRATEGY[strategy]
        full = hip_strategy in (hip.GREEDY, hip.FORCED)
        gs = group_size or 0
        if encode and self._has_hip_encoder():
            images = images_or_features
            if images.dim() == 4:  # (B,3,H,W): one exemplar per sample
                images = images.unsqueeze(1)
                masks = None if masks is None else masks.unsqueeze(1)
            out = ctx.describe(images, masks, hip_strategy, length, beam_size,
                               mi, temperature, group_size=gs, want_full=full,
                               forced=forced)
        else:
            if encode:
                features = self.encode(images_or_features, masks=masks)
            else:
                features = images_or_features
            out = ctx.decode(features, hip_strategy, length, beam_size, mi,
                             temperature, group_size=gs, want_full=full,
                             forced=forced)

        tokens, scores = out['tokens'], out['scores']
        beam_captions = beam_scores = beam_tokens = None
        if not full:
            # allennlp returns T' <= length columns; with several groups the
            # tensors keep the longest group's T' (shorter groups are padded
            # with <stop>, which reconstruct() ignores).
            tprime = int(out['out_len'].max().item())
            tokens = tokens[:, :tprime]
            beam_tokens = out['beam_tokens'][:, :, :tprime]
            beam_scores = out['beam_scores']
            beam_captions = lang.LazyCaptions(self.indexer, beam_tokens)
        assert len(tokens) == batch_size
        return DecoderOutput(
            captions=self.indexer.reconstruct(tokens.tolist()),
            scores=scores,
            tokens=tokens,
            predictions=out['predictions'],
            attentions=out['attentions'],
            beam_captions=beam_captions,
            beam_scores=beam_scores,
            beam_tokens=beam_tokens,
        )

    def _train_context(self) -> hip.Context:
        """A context that only carries the decoder's dims, never finalized,
        cached on the decoder: the training calls read the live parameters, so
        optimizer steps do not rebuild it."""
        device = hip.require_device(self.device)
        key = (device, tuple(p.shape for p in self._train_params()))
        if self._train_ctx is None or self._train_ctx_key != key:
            sd = {k: v for k, v in self.state_dict().items()
                  if not k.startswith(('encoder.', 'lm.'))}
            # (the old one closes when the last graph that holds it goes)
            self._train_ctx = hip.Context(
                hip.make_dims(sd, len(self.indexer.vocab)), {}, device,
                finalize=False)
            self._train_ctx_key = key
        return self._train_ctx

    def _forward_train(self, images_or_features, masks, encode,
                       targets: torch.Tensor) -> DecoderOutput:
        """Training-mode teacher forcing (reference :431-463 with dropout on):
        predictions and attentions carry `grad_fn` through `TeacherForced`, and
        so does `scores`.  Features from the native encoder come under no_grad
        (its trunk has no backward); a foreign torch Encoder runs with
        autograd and receives the feature gradient."""
        device = hip.require_device(self.device)
        if encode:
            if self._has_hip_encoder():
                with torch.no_grad():
                    features = self.encode(images_or_features, masks=masks)
            else:
                features = self.encode(images_or_features, masks=masks)
        else:
            features = images_or_features
        features = features.to(device, torch.float32).contiguous()
        targets = targets.to(device, torch.long).contiguous()
        seed = 0
        if self.dropout > 0:  # as Decoder.fit draws it
            seed = int(torch.randint(
                2**62, (), device=device,
                generator=torch.cuda.default_generators[device.index]))
        predictions, attentions = TeacherForced.apply(
            self._train_context(), targets, float(self.dropout), seed,
            features, *self._train_params())
        # scores[:] += predictions[idx_b, currents] per step (reference :460-463)
        scores = predictions.gather(2, targets.unsqueeze(-1)).squeeze(-1).sum(1)
        return DecoderOutput(
            captions=self.indexer.reconstruct(targets.tolist()),
            scores=scores, tokens=targets, predictions=predictions,
            attentions=attentions, beam_captions=None, beam_scores=None,
            beam_tokens=None)

    def _sample(self, images_or_features, masks, encode, length, mi,
                temperature) -> DecoderOutput:
        """`strategy='sample'` (reference :448-453): one token per row drawn
        from exp(log-probs) with torch's global generator, row by row like the
        reference, so a seeded run consumes the RNG in the same order.  The
        steps run through `milan_step`; only the draw itself is torch's."""
        features = (self.encode(images_or_features, masks=masks)
                    if encode else images_or_features)
        features = features.to(self.device)
        batch_size = len(features)
        state = self.init_state(features, lm=mi)
        currents = torch.full((batch_size,), self.indexer.start_index,
                              dtype=torch.long, device=self.device)
        tokens = currents.new_zeros(batch_size, length)
        scores = features.new_zeros(batch_size)
        predictions = features.new_zeros(batch_size, length, self.vocab_size)
        attentions = features.new_zeros(batch_size, length, features.shape[1])
        rows = torch.arange(batch_size, device=self.device)
        for time in range(length):
            step = self.step(features, currents, state,
                             temperature=temperature)
            currents = currents.clone()
            for row, logprobs in enumerate(step.predictions):
                probs = torch.exp(logprobs)
                currents[row] = torch.distributions.Categorical(
                    probs=probs).sample()
            predictions[:, time] = step.predictions
            attentions[:, time] = step.attentions
            tokens[:, time] = currents
            state = step.state
            scores = scores + step.predictions[rows, currents]
        return DecoderOutput(
            captions=self.indexer.reconstruct(tokens.tolist()),
            scores=scores, tokens=tokens, predictions=predictions,
            attentions=attentions, beam_captions=None, beam_scores=None,
            beam_tokens=None)

    def encode(self,
               images: torch.Tensor,
               masks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Images+masks -> (B, k, F) features (reference :525-546)."""
        batch_size = len(images)
        images = images.reshape(-1, *images.shape[-3:])
        if masks is not None:
            masks = masks.reshape(-1, *masks.shape[-3:])
        if self._has_hip_encoder():
            features = self._context().encode(images, masks)
        else:
            features = self.encoder(images, masks=masks)
        return features.view(batch_size, -1, self.feature_size)

    def init_state(self, features: torch.Tensor, lm: bool = True) -> DecoderState:
        """reference :548-574."""
        h, c = self._context().init_state(features)
        h_lm = c_lm = None
        if self.lm is not None and lm:
            batch_size = len(features)
            h_lm = h.new_zeros(self.lm.layers, batch_size, self.lm.hidden_size)
            c_lm = c.new_zeros(self.lm.layers, batch_size, self.lm.hidden_size)
        return DecoderState(h, c, h_lm, c_lm)

    def step(self,
             features: torch.Tensor,
             tokens: torch.Tensor,
             state: DecoderState,
             temperature: Optional[float] = None) -> DecoderStep:
        """One decoding step (reference :576-634)."""
        h, c, h_lm, c_lm = state
        if (h_lm is None) != (c_lm is None):
            raise ValueError('state must have both h_lm and c_lm or neither')
        if h_lm is not None and self.lm is None:
            raise ValueError('state has h_lm or c_lm, but decoder has no lm')
        temperature = self.temperature if temperature is None else temperature
        pred, att, h2, c2, h_lm, c_lm = self._context().step(
            features, tokens, h, c, h_lm, c_lm, temperature)
        return DecoderStep(predictions=pred,
                           attentions=att,
                           state=DecoderState(h=h2, c=c2, h_lm=h_lm, c_lm=c_lm))

    # -- dataset driver ---------------------------------------------------------------
    def score(self,
              captions,
              images_or_features: torch.Tensor,
              masks: Optional[torch.Tensor] = None,
              device=None,
              **kwargs: Any) -> torch.Tensor:
        """Force decode the captions, returning their total scores
        (reference :636-711): log-probabilities (`mi=False`) or mutual
        informations (`mi=True`).

        `captions` are strings (needs `indexer.tokenize`, i.e. the spaCy
        tokenizer the checkpoint was trained with, or any callable) or --
        extension -- already tokenized sequences of token strings, which are
        indexed with `Indexer.index` directly.
        """
        for forbidden in ('strategy', 'length'):
            if forbidden in kwargs:
                raise ValueError(f'option disallowed: {forbidden}')
        if masks is not None and len(masks) != len(images_or_features):
            raise ValueError('images_or_features and masks must have the '
                             f'same batch size; got {len(images_or_features)} '
                             f'and {len(masks)}')
        if len(images_or_features) == 1:
            images_or_features = images_or_features.expand(
                len(captions), *images_or_features.shape[1:])
            if masks is not None:
                masks = masks.expand(len(captions), *masks.shape[1:])
        elif len(images_or_features) != len(captions):
            raise ValueError('images_or_features must have batch size 1 or '
                             f'{len(captions)}; got {len(images_or_features)}')
        if device is not None:
            self.to(device)
        pretokenized = len(captions) > 0 and not isinstance(captions[0], str)
        index = self.indexer.index if pretokenized else self.indexer
        targets = torch.tensor(index(captions))[:, 1:]
        _, length = targets.shape
        outputs = self(images_or_features, masks=masks, strategy=targets,
                       length=length, **kwargs)
        indexed = index(captions, start=False, stop=True, pad=False, unk=True)
        # total_i = sum_t predictions[i, t, indexed_i[t]] over the caption's own
        # length (the reference's per-caption Python gather, one device gather)
        lens = torch.tensor([len(ix) for ix in indexed])
        padded = torch.zeros(len(indexed), length, dtype=torch.long)
        for i, ix in enumerate(indexed):
            padded[i, :len(ix)] = torch.tensor(ix, dtype=torch.long)
        pred = outputs.predictions
        picked = pred.gather(2, padded.to(pred.device).unsqueeze(-1)).squeeze(-1)
        keep = torch.arange(length)[None, :] < lens[:, None]
        totals = (picked * keep.to(pred.device, pred.dtype)).sum(dim=1)
        return totals if device is None else totals.to(device)

    def predict(self,
                dataset: data.Dataset,
                mask: bool = True,
                image_index: int = 2,
                mask_index: int = 3,
                batch_size: int = 16,
                features: Optional[data.TensorDataset] = None,
                num_workers: int = 0,
                device: Optional[Union[str, torch.device]] = None,
                display_progress_as: Optional[str] = 'predict captions',
                share_images: Optional[bool] = None,
                **kwargs: Any) -> Tuple[str, ...]:
        """Feed an entire dataset through the decoder (reference :809-871).

        Same arguments and return value.  `batch_size` keeps its meaning for
        the result (allennlp's early exit is evaluated per `batch_size`
        neurons) but the GPU is fed `self.chunk_size` neurons at a time.
        `share_images` overrides `self.share_images` for this call (identical
        images inside one chunk go through the trunk once; same captions).
        """
        if share_images is not None:
            saved, self.share_images = self.share_images, bool(share_images)
            try:
                return self.predict(dataset, mask=mask, image_index=image_index,
                                    mask_index=mask_index, batch_size=batch_size,
                                    features=features, num_workers=num_workers,
                                    device=device,
                                    display_progress_as=display_progress_as,
                                    **kwargs)
            finally:
                self.share_images = saved
        if device is not None:
            self.to(device)
        chunk = max(batch_size, (self.chunk_size // batch_size) * batch_size)
        source = dataset if features is None else features
        n = len(source)

        def progress(iterable, total):
            if display_progress_as is None:
                return iterable
            try:
                from tqdm.auto import tqdm
            except ImportError:
                return iterable
            return tqdm(iterable, total=total, desc=display_progress_as)

        # The uint8 fast path bypasses `__getitem__`, so it is only taken when
        # that changes nothing: default tuple positions, no dataset-side
        # transforms / device, no DataLoader workers requested.
        fast = None
        if (features is None and image_index == 2 and mask_index == 3 and
                num_workers == 0 and torch.cuda.is_available()):
            plain = all(getattr(dataset, attr, None) is None
                        for attr in ('transform_images', 'transform_masks',
                                     'device'))
            fast = getattr(dataset, 'slice_uint8', None) if plain else None
        captions = []
        if fast is not None:
            # memory-mapped uint8 dataset: worker thread -> pinned staging ->
            # async H2D on a side stream, overlapped with the previous chunk
            from milan_amd import ingest
            dev = hip.require_device(self.device)
            # Chunks ramp up from 64 neurons: the first fetch is the only one no
            # compute hides, and a chunk's compute has to cover the next
            # chunk's fetch (results do not depend on how neurons are grouped
            # into launches).
            if n > 0:
                # no more neurons per launch than the free memory carries, and ONE
                # workspace allocation at the largest chunk instead of one per
                # ramp step
                probe_im, _ = fast(0, 1)
                ctx = self._context()
                args = (probe_im.shape[1], max(probe_im.shape[-2:]),
                        kwargs.get('beam_size') or self.beam_size,
                        kwargs.get('length') or self.length)
                chunk = max(batch_size,
                            ctx.fit_neurons(min(chunk, n), args[0], *args[1:],
                                            multiple=batch_size))
                ctx.workspace(min(chunk, n), *args)
            spans, lo, size = [], 0, batch_size * max(1, 64 // batch_size)
            while lo < n:
                size = min(size, chunk)
                spans.append((lo, min(n, lo + size)))
                lo += size
                size = (size * 3 // batch_size) * batch_size
            # datasets whose slice_uint8 takes `out=` fill the pinned staging
            # buffers directly (one pass over the bytes)
            import inspect
            into = 'out' in inspect.signature(fast).parameters and n > 0
            alloc = None
            if into:
                probe_im, probe_mk = fast(0, 1)
                n_max = max(hi - lo for lo, hi in spans)

                def alloc():
                    return tuple(
                        torch.empty((n_max,) + tuple(p.shape[1:]),
                                    dtype=torch.uint8, pin_memory=True)
                        for p in (probe_im, probe_mk))

            def fetch(i, out=None):
                images, masks = (fast(*spans[i], out=out) if into else
                                 fast(*spans[i]))
                return images, (masks if mask else None)

            chunks = ingest.ChunkPrefetcher(fetch, len(spans), dev, alloc=alloc)
            for images, masks in progress(chunks, len(spans)):
                with torch.no_grad():
                    output = self(images, masks, group_size=batch_size,
                                  **kwargs)
                captions += list(output.captions)
            return tuple(captions)
        spans = range(0, n, chunk)
        for lo in progress(spans, len(spans)):
            hi = min(n, lo + chunk)
            loader = data.DataLoader(data.Subset(source, range(lo, hi)),
                                     batch_size=hi - lo,
                                     num_workers=num_workers)
            batch = next(iter(loader))
            if features is None:
                inputs = (batch[image_index],
                          batch[mask_index] if mask else None)
            else:
                inputs = tuple(batch)
            with torch.no_grad():
                output = self(*inputs, group_size=batch_size, **kwargs)
            captions += list(output.captions)
        return tuple(captions)

    def bleu(self,
             dataset: data.Dataset,
             annotation_index: int = 4,
             predictions: Optional[Sequence[str]] = None,
             **kwargs: Any) -> metrics.BLEUScore:
        """Corpus BLEU of this model's captions on `dataset` (reference
        :713-738): `predict(dataset, **kwargs)` unless `predictions` are
        given, then `metrics.bleu`."""
        if predictions is None:
            predictions = self.predict(dataset, **kwargs)
        return metrics.bleu(dataset,
                            predictions,
                            annotation_index=annotation_index)

    def bert_score(self,
                   dataset: data.Dataset,
                   annotation_index: int = 4,
                   bert_scorer_batch_size: int = 16,
                   predictions: Optional[Sequence[str]] = None,
                   device: Optional[Union[str, torch.device]] = None,
                   bert_scorer: Optional[Any] = None,
                   **kwargs: Any) -> Mapping[str, float]:
        """Average BERTScore P/R/F ('p', 'r', 'f') of this model's captions on
        `dataset` (reference :771-807): `predict(dataset, **kwargs)` unless
        `predictions` are given, then `metrics.bert_score`.  `bert_scorer`: a
        `milan_amd.bertscore.BERTScorer`; by default `bertscore.load()`."""
        if predictions is None:
            predictions = self.predict(dataset, **kwargs)
        return metrics.bert_score(dataset,
                                  predictions,
                                  annotation_index=annotation_index,
                                  batch_size=bert_scorer_batch_size,
                                  device=device,
                                  bert_scorer=bert_scorer)

    # -- training (reference :873-1070) ----------------------------------------------
    def reset_parameters(self) -> None:
        """Initialise the decoder's own parameters as the reference's torch
        modules do (the constructor leaves them zero): init_h, init_c,
        embedding, attention (query, key, output), feature_gate, LSTMCell and
        output are built in the reference's order, so the draws from torch's
        global generator are the same."""
        fs, hs, es, v = (self.feature_size, self.hidden_size,
                         self.embedding_size, self.vocab_size)
        a = self.attend.hidden_size
        init_h, init_c = nn.Linear(fs, hs), nn.Linear(fs, hs)
        embedding = nn.Embedding(v, es)
        query, key, score = nn.Linear(hs, a), nn.Linear(fs, a), nn.Linear(a, 1)
        gate = nn.Linear(hs, fs)
        lstm = nn.LSTMCell(es + fs, hs)
        output = nn.Linear(hs, v)
        state = {'embedding.weight': embedding.weight}
        for name, module in (('init_h.0', init_h), ('init_c.0', init_c),
                             ('attend.query_to_hidden', query),
                             ('attend.key_to_hidden', key),
                             ('attend.output.0', score),
                             ('feature_gate.0', gate), ('output.1', output)):
            state[f'{name}.weight'] = module.weight
            state[f'{name}.bias'] = module.bias
        state.update({f'lstm.{k}': t for k, t in lstm.state_dict().items()})
        with torch.no_grad():
            for name, param in self.named_parameters():
                if name in state:
                    param.copy_(state[name])

    def _train_params(self) -> Tuple[torch.nn.Parameter, ...]:
        """The 19 tensors milan_decoder_train_step reads, in its order."""
        named = dict(self.named_parameters())
        return tuple(named[name] for name in TRAIN_PARAMS)

    def fit(self,
            dataset: data.Dataset,
            mask: bool = True,
            image_index: int = 2,
            mask_index: int = 3,
            annotation_index: int = 4,
            batch_size: int = 64,
            max_epochs: int = 100,
            patience: int = 4,
            hold_out: Union[float, Sequence[int]] = .1,
            stop_on_bleu: bool = True,
            regularization_weight: float = 1.,
            optimizer_t: Type[optim.Optimizer] = optim.AdamW,
            optimizer_kwargs: Optional[Mapping[str, Any]] = None,
            features: Optional[data.TensorDataset] = None,
            num_workers: int = 0,
            device: Optional[Union[str, torch.device]] = None,
            display_progress_as: Optional[str] = 'train decoder') -> None:
        """Train the decoder on `dataset` (reference :873-1070).

        Same loop as the reference: the hold-out split is by neuron
        (`random_split` on torch's global generator, or `fixed_split`), the
        batches are one sample per annotation, shuffled by a DataLoader;
        `optimizer_t(self.parameters(), **optimizer_kwargs)`; the training
        loss is NLLLoss(ignore_index=pad) plus `regularization_weight` times
        the double-stochasticity regulariser; each epoch ends with the
        validation NLL and a greedy, likelihood-only `bleu` of the validation
        neurons; `EarlyStopping` tracks BLEU (`stop_on_bleu`) or the
        validation loss.

        A batch's loss and the gradients of the decoder's 19 own tensors come
        from `milan_decoder_train_step` (train mode, dropout seeded from the
        device's torch generator when `dropout > 0`); the encoder and LM keep
        `grad=None`, so the optimizer leaves them alone.  Features come from
        `features` or, without it, from `self.encode` under no_grad.  As in the
        reference, the "best" state kept for the restore on stop is
        `state_dict()`, whose tensors share storage with the parameters: the
        model ends with the parameters of the last epoch run.  It is left in
        eval mode.
        """
        if device is not None:
            self.to(device)
        if optimizer_kwargs is None:
            optimizer_kwargs = {}
        device = hip.require_device(self.device)

        class WrapperDataset(data.Dataset):
            """Split by neuron, iterate by annotation (reference :957-987)."""

            def __init__(self, subset: data.Subset):
                self.samples = []
                for index in subset.indices:
                    if features is None:
                        images = dataset[index][image_index]
                        masks = dataset[index][mask_index] if mask else None
                        images_or_features = (images, masks)
                    else:
                        images_or_features = features[index]
                    annotations = dataset[index][annotation_index]
                    if isinstance(annotations, str):
                        annotations = [annotations]
                    for annotation in annotations:
                        self.samples.append((images_or_features, annotation))

            def __getitem__(self, index: int):
                return self.samples[index]

            def __len__(self) -> int:
                return len(self.samples)

        if isinstance(hold_out, float):
            train, val = training.random_split(dataset, hold_out=hold_out)
        else:
            train, val = training.fixed_split(dataset, hold_out)
        train_loader = data.DataLoader(WrapperDataset(train),
                                       num_workers=num_workers,
                                       batch_size=batch_size,
                                       shuffle=True)
        val_loader = data.DataLoader(WrapperDataset(val),
                                     num_workers=num_workers,
                                     batch_size=batch_size)

        optimizer = optimizer_t(self.parameters(), **optimizer_kwargs)
        stopper = training.EarlyStopping(patience=patience,
                                         decreasing=not stop_on_bleu)

        # a context that only carries the decoder's dims, never finalized: the
        # training calls read the live parameters, so optimizer steps never
        # rebuild it (inference after fit rebuilds `_context()`, which keys on
        # the parameters' versions)
        sd = {k: v for k, v in self.state_dict().items()
              if not k.startswith(('encoder.', 'lm.'))}
        ctx = hip.Context(hip.make_dims(sd, len(self.indexer.vocab)), {},
                          device, finalize=False)
        weights = self._train_params()
        grads = [torch.empty_like(p) for p in weights]
        cuda_generator = torch.cuda.default_generators[device.index]

        def prepare(batch):
            images_or_features, captions = batch
            if features is None:
                images, masks = images_or_features
                with torch.no_grad():
                    inputs = self.encode(
                        images.to(device),
                        masks=masks.to(device) if masks is not None else None)
            else:
                inputs, = images_or_features
            targets = torch.tensor(self.indexer(captions))[:, 1:]
            return inputs.to(device, torch.float32), targets

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
            self.encoder.eval()
            train_loss = 0.
            for batch in train_loader:
                inputs, targets = prepare(batch)
                seed = 0
                if self.dropout > 0:
                    seed = int(torch.randint(2**62, (), device=device,
                                             generator=cuda_generator))
                terms = ctx.decoder_train_step(weights, grads, inputs, targets,
                                               self.dropout, seed,
                                               regularization_weight)
                for p, g in zip(weights, grads):
                    p.grad = g
                optimizer.step()
                optimizer.zero_grad()
                regularizer = terms[2] / (inputs.shape[0] * inputs.shape[1])
                loss = terms[0] / terms[1] + regularization_weight * regularizer
                train_loss += loss.item()
            train_loss /= len(train_loader)

            self.eval()
            val_loss = 0.
            for batch in val_loader:
                inputs, targets = prepare(batch)
                terms = ctx.decoder_nll(weights, inputs, targets)
                val_loss += (terms[0] / terms[1]).item()
            val_loss /= len(val_loader)
            val_bleu = self.bleu(val,
                                 strategy=STRATEGY_GREEDY,
                                 mi=False,
                                 device=device,
                                 display_progress_as=None).score

            if not isinstance(progress, range):
                progress.set_description(f'{display_progress_as} '
                                         f'[train_loss={train_loss:.3f}, '
                                         f'val_loss={val_loss:.3f}, '
                                         f'val_bleu={val_bleu:.1f}]')

            stop = stop_on_bleu and stopper(val_bleu)
            stop |= not stop_on_bleu and stopper(val_loss)
            if stop:
                self.load_state_dict(best)
                break

            if stopper.improved:
                best = self.state_dict()
        self.eval()
        ctx.close()

    # -- serialisation (reference serialize.py:175-269, decoders.py:1072-1109) ---------
    def properties(self) -> Mapping[str, Any]:
        return {
            'indexer': self.indexer,
            'encoder': self.encoder,
            'lm': self.lm,
            'embedding_size': self.embedding_size,
            'hidden_size': self.hidden_size,
            'attention_hidden_size': self.attention_hidden_size,
            'dropout': self.dropout,
            'length': self.length,
            'strategy': self.strategy,
            'temperature': self.temperature,
            'beam_size': self.beam_size,
        }

    def serialize(self, state_dict: bool = True) -> Dict[str, Any]:
        def ser(obj):
            if obj is None or not hasattr(obj, 'properties'):
                return obj
            return serialize.serialized(
                {k: ser(v) for k, v in obj.properties().items()})

        out = serialize.serialized(
            {k: ser(v) for k, v in self.properties().items()},
            {'encoder': encoders.key(self.encoder)})
        if state_dict:
            out['state_dict'] = self.state_dict()
        return out

    def save(self, file, **kwargs: Any) -> None:
        torch.save(self.serialize(**kwargs), file)

    @classmethod
    def deserialize(cls,
                    payload: Mapping[str, Any],
                    strict: bool = False,
                    load_state_dict: bool = True) -> 'Decoder':
        payload = dict(payload)
        if (not issubclass(cls, DecoderWithCLIP)
                and 'reranker_kwargs' in serialize.props(payload)):
            # a checkpoint of a DecoderWithCLIP (the reference's included)
            return DecoderWithCLIP.deserialize(payload, strict=strict,
                                               load_state_dict=load_state_dict)
        state_dict = payload.pop('state_dict', None)
        p = dict(serialize.props(payload))
        children = payload.get('children') or {}
        encoder_key = children.get('encoder')
        if encoder_key is None:
            raise ValueError('serialized decoder missing encoder')

        def make_indexer(node) -> lang.Indexer:
            ip = dict(serialize.props(node))
            vocab = lang.Vocab(tuple(serialize.props(ip.pop('vocab'))['tokens']))
            tokenize = ip.pop('tokenize', None)
            return lang.Indexer(vocab, tokenize, **ip)

        indexer = make_indexer(p.pop('indexer'))
        enc_node = p.pop('encoder')
        encoder = encoders.parse(encoder_key)(**serialize.props(enc_node))
        lm = None
        lm_node = p.pop('lm', None)
        if lm_node is not None:
            lp = dict(serialize.props(lm_node))
            lm = lms.LanguageModel(make_indexer(lp.pop('indexer')), **lp)
        module = cls(indexer, encoder, lm=lm, **p)
        if state_dict is not None and load_state_dict:
            module.load_state_dict(state_dict, strict=strict)
        return module

    @classmethod
    def load(cls, file, **kwargs: Any) -> 'Decoder':
        """Load a reference-format checkpoint (serialize.py:255-269).
        Keyword arguments are forwarded to `torch.load`."""
        return cls.deserialize(serialize.load_payload(file, **kwargs))


class DecoderWithCLIP(Decoder):
    """Decoder that uses CLIP to rerank the final beam (reference
    decoders.py:1115-1211).  The CLIP towers run in HIP on the decoder's GPU,
    in exact fp32 whatever `precision` says (milan_amd.rerankers)."""

    def __init__(self,
                 *args: Any,
                 reranker_kwargs: Optional[Mapping[str, Any]] = None,
                 **kwargs: Any):
        kwargs.setdefault('strategy', STRATEGY_BEAM)
        kwargs.setdefault('beam_size', 1000)
        kwargs.setdefault('temperature', .5)
        super().__init__(*args, **kwargs)
        self.reranker_kwargs = dict(reranker_kwargs) if reranker_kwargs else {}
        self.reranker_kwargs.setdefault('name', 'ViT-B/32')
        self.reranker_kwargs.setdefault('jit', False)
        self.reranker_kwargs.setdefault('device', 'cpu')
        self.reranker = rerankers.reranker(**self.reranker_kwargs)

    def forward(  # type: ignore[override]
        self,
        images_or_features: torch.Tensor,
        masks: Optional[torch.Tensor] = None,
        lam: Optional[float] = None,
        **kwargs: Any,
    ) -> DecoderOutput:
        """Beam-decode, then rerank the beam with CLIP.  `images_or_features`
        must be the images (CLIP needs them intact) and `masks` must be given.
        captions / scores / tokens are those of the top-ranked beam; the other
        fields are the beam search's."""
        if masks is None:
            raise ValueError('must specify masks in DecoderWithCLIP')
        if 'strategy' in kwargs:
            raise ValueError('cannot set "strategy" in DecoderWithCLIP')
        images = images_or_features
        outputs = super().forward(images, masks=masks, strategy=STRATEGY_BEAM,
                                  **kwargs)
        beam_captions, beam_scores, beam_tokens = (outputs.beam_captions,
                                                   outputs.beam_scores,
                                                   outputs.beam_tokens)
        assert beam_captions is not None and beam_scores is not None
        assert beam_tokens is not None
        clip_images, clip_masks = images, masks
        if clip_images.dim() == 4:  # (B, 3, H, W): one exemplar per sample
            clip_images, clip_masks = images.unsqueeze(1), masks.unsqueeze(1)
        # (uint8 images stand for x * float32(1 / 255), the floats the reference's
        # dataset hands to both the encoder and CLIP; the reranker converts them chunk
        # by chunk)
        device = self.device
        clip_images, clip_masks = clip_images.to(device), clip_masks.to(device)
        texts = [list(captions) for captions in beam_captions]
        rerankeds = self.reranker(clip_images, clip_masks, texts, lam=lam)
        captions = tuple(reranked[0] for reranked in rerankeds.texts)
        best = torch.tensor([order[0] for order in rerankeds.orders],
                            device=beam_scores.device)
        rows = torch.arange(len(best), device=beam_scores.device)
        return DecoderOutput(captions, beam_scores[rows, best],
                             beam_tokens[rows, best], *outputs[3:])

    def properties(self) -> Mapping[str, Any]:
        # (the CLIP tensors travel in the state dict and the tokenizer is code:
        # neither is a property)
        kwargs = {
            key: value for key, value in self.reranker_kwargs.items()
            if key not in ('weights', 'tokenize')
        }
        # heads that `clip` would infer itself (width // 64) are not written, so that the
        # reference can load the checkpoint (its clip.load rejects unknown keywords)
        dims = self.reranker.clip_with_masks.dims
        for side in ('vision', 'text'):
            if kwargs.get(f'{side}_heads') == dims[f'{side}_width'] // 64:
                del kwargs[f'{side}_heads']
        return {**super().properties(), 'reranker_kwargs': kwargs}

    def serialize(self, state_dict: bool = True) -> Dict[str, Any]:
        """As Decoder.serialize; the state dict also holds CLIP's tensors under
        the names a reference DecoderWithCLIP gives them."""
        out = super().serialize(state_dict=state_dict)
        if state_dict:
            out['state_dict'].update(rerankers.to_reference_keys(
                self.reranker.clip_with_masks.weights))
        return out

    @classmethod
    def deserialize(cls,
                    payload: Mapping[str, Any],
                    strict: bool = False,
                    load_state_dict: bool = True,
                    reranker_kwargs: Optional[Mapping[str, Any]] = None
                    ) -> 'DecoderWithCLIP':
        """`reranker_kwargs` (e.g. `weights=`, `tokenize=`) override the
        serialized ones.  CLIP's tensors are taken from the payload's state
        dict when it has them (a checkpoint of a DecoderWithCLIP, the
        reference's included)."""
        payload = dict(payload)
        props = dict(serialize.props(payload))
        kwargs = dict(props.get('reranker_kwargs') or {})
        kwargs.update(reranker_kwargs or {})
        state = payload.get('state_dict')
        if state is not None:
            clip_state = rerankers.from_reference_keys(state)
            if clip_state and 'weights' not in kwargs:
                kwargs['weights'] = clip_state
            payload['state_dict'] = type(state)(
                (key, value) for key, value in state.items()
                if not key.startswith(rerankers.REFERENCE_PREFIX))
        props['reranker_kwargs'] = kwargs
        payload['properties'] = props
        return super().deserialize(payload, strict=strict,
                                   load_state_dict=load_state_dict)

    @classmethod
    def from_decoder(cls,
                     decoder: Decoder,
                     reranker_kwargs: Optional[Mapping[str, Any]] = None
                     ) -> 'DecoderWithCLIP':
        """Convert a base Decoder to a DecoderWithCLIP."""
        return cls.deserialize(decoder.serialize(),
                               reranker_kwargs=reranker_kwargs)


def decoder(dataset: data.Dataset,
            encoder: encoders.Encoder,
            rerank_with_clip: bool = False,
            annotation_index: int = 4,
            indexer_kwargs: Optional[Mapping[str, Any]] = None,
            **kwargs: Any) -> Decoder:
    """A new Decoder for the annotations of `dataset` (reference
    decoders.py:1214-1259): each sample's annotations are joined with
    `lang.join`, the indexer is built from them (`start`, `stop`, `pad`, `unk`
    default to True; `tokenize` must be given, as for `lms.lm`) and **kwargs go
    to the constructor.  The parameters are initialised as the reference's
    torch modules initialise theirs, with the same draws from torch's global
    generator.  `rerank_with_clip=True` gives a DecoderWithCLIP; its
    `reranker_kwargs` (`weights=`, `tokenize=`) go in **kwargs."""
    indexer_kwargs = dict(indexer_kwargs or {})
    annotations = [
        lang.join(dataset[index][annotation_index])
        for index in range(len(cast(Sized, dataset)))
    ]
    for key in ('start', 'stop', 'pad', 'unk'):
        indexer_kwargs.setdefault(key, True)
    indexer = lang.indexer(annotations, **indexer_kwargs)
    if rerank_with_clip:
        try:
            model: Decoder = DecoderWithCLIP(indexer, encoder, **kwargs)
        except ImportError as error:
            # what this factory raised before the reranker was built, and still does
            # when neither the `clip` package nor reranker_kwargs['weights'] is there
            raise NotImplementedError(str(error)) from error
    else:
        model = Decoder(indexer, encoder, **kwargs)
    model.reset_parameters()
    return model
