"""Rerank MILAN's beam with CLIP (reference `src/milan/rerankers.py`), in HIP.

Per neuron the reference runs CLIP's ViT twice over the k exemplar images --
once with the activation mask multiplied into the CLS query's attention
weights, once without -- and the text tower over every candidate caption, and
ranks the captions by

    (1 - lam) * sum_k cos(masked image_k, text) + lam * sum_k cos(image_k, text).

Here both towers are HIP kernels (csrc/clip.hip) in exact fp32: all images of a
call go through each layer as one batch, the text tower runs once per call and
only over the positions up to the longest caption's end-of-text token.

Neither OpenAI's `clip` package nor its weights ship with this project:
`CLIPWithMasks(weights=...)` takes a state dict (or a path to one) in that
package's layout, and `tokenize=...` a callable with the contract of
`clip.tokenize`.  Both default to the `clip` package when it is importable.
"""
import math
import os
from typing import (Any, Callable, Dict, Mapping, NamedTuple, Optional,
                    Sequence, Tuple, Union)

import torch
from torch import nn

from milan_amd import hip

StrSequence = Sequence[str]

# renormalize.OFFSET_SCALE['pt'] of the reference: its default source statistics
SOURCE_MEAN, SOURCE_STD = (0., 0., 0.), (1., 1., 1.)
# the Normalize of CLIP's preprocess (clip/clip.py)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# prefix of CLIP's tensors in the state dict of a reference DecoderWithCLIP
REFERENCE_PREFIX = 'reranker.clip_with_masks.model.'


def infer_dims(state_dict: Mapping[str, torch.Tensor],
               vision_heads: Optional[int] = None,
               text_heads: Optional[int] = None) -> Dict[str, int]:
    """Dims of a ViT CLIP from its state dict, as `clip.model.build_model`
    infers them (heads = width // 64 unless given)."""
    if 'visual.proj' not in state_dict:
        if any(key.startswith('visual.layer') for key in state_dict):
            raise ValueError('this is the state dict of a ResNet CLIP; only '
                             'the ViT variants (ViT-B/32, ...) are built')
        raise ValueError('not a CLIP state dict: no "visual.proj"')
    try:
        conv1 = state_dict['visual.conv1.weight']
        vision_width, patch = conv1.shape[0], conv1.shape[-1]
        vision_layers = len([
            key for key in state_dict if key.startswith('visual.') and
            key.endswith('.attn.in_proj_weight')
        ])
        tokens = state_dict['visual.positional_embedding'].shape[0]
        grid = round((tokens - 1)**.5)
        if grid * grid + 1 != tokens:
            raise ValueError(f'{tokens} image tokens are not a square grid + 1')
        dims = {
            'resolution': patch * grid,
            'patch': patch,
            'vision_width': vision_width,
            'vision_layers': vision_layers,
            'vision_heads': vision_heads or vision_width // 64,
            'embed_dim': state_dict['text_projection'].shape[1],
            'context_length': state_dict['positional_embedding'].shape[0],
            'vocab_size': state_dict['token_embedding.weight'].shape[0],
            'text_width': state_dict['ln_final.weight'].shape[0],
            'text_layers': len({
                key.split('.')[2] for key in state_dict
                if key.startswith('transformer.resblocks.')
            }),
        }
    except KeyError as error:
        raise ValueError(f'CLIP state dict lacks {error}') from error
    dims['text_heads'] = text_heads or dims['text_width'] // 64
    for side in ('vision', 'text'):
        width, heads = dims[f'{side}_width'], dims[f'{side}_heads']
        if heads < 1 or width % heads:
            raise ValueError(f'{side} width {width} is not a multiple of '
                             f'{heads} heads; pass {side}_heads=')
    return {key: int(value) for key, value in dims.items()}


def from_reference_keys(
        state_dict: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """CLIP's tensors out of the state dict of a reference DecoderWithCLIP
    (`reranker.clip_with_masks.model.*`, whose visual blocks hold the wrapped
    attention's `attn.qkv.weight / .bias`), in OpenAI's layout."""
    out = {}
    for key, value in state_dict.items():
        if not key.startswith(REFERENCE_PREFIX):
            continue
        key = key[len(REFERENCE_PREFIX):]
        key = key.replace('.attn.qkv.weight', '.attn.in_proj_weight')
        key = key.replace('.attn.qkv.bias', '.attn.in_proj_bias')
        out[key] = value
    return out


def to_reference_keys(
        state_dict: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Inverse of `from_reference_keys`."""
    out = {}
    for key, value in state_dict.items():
        if key.startswith('visual.transformer.'):
            key = key.replace('.attn.in_proj_weight', '.attn.qkv.weight')
            key = key.replace('.attn.in_proj_bias', '.attn.qkv.bias')
        out[REFERENCE_PREFIX + key] = value
    return out


def _load_clip(name, jit, kwargs):
    try:
        import clip
    except ImportError as error:
        raise ImportError(
            'the `clip` package is not installed, so CLIP\'s weights cannot be '
            f'loaded by name ({name!r}): pass weights=<state dict or path to '
            'one, in the layout of OpenAI\'s clip> to CLIPWithMasks / '
            'reranker_kwargs') from error
    model, preprocess = clip.load(name, jit=jit, device='cpu', **kwargs)
    heads = {}
    try:
        heads['vision_heads'] = model.visual.transformer.resblocks[0].attn.num_heads
        heads['text_heads'] = model.transformer.resblocks[0].attn.num_heads
    except AttributeError:
        pass
    norm = preprocess.transforms[-1]
    return model.state_dict(), heads, tuple(norm.mean), tuple(norm.std)


class CLIPWithMasks(nn.Module):
    """CLIP model that can use masks (reference rerankers.py:104-254)."""

    def __init__(self,
                 mask_layers: Optional[Sequence[int]] = None,
                 source_mean: Optional[Sequence[float]] = None,
                 source_std: Optional[Sequence[float]] = None,
                 name: str = 'ViT-B/32',
                 jit: bool = False,
                 device: Any = 'cpu',
                 weights: Union[None, str, os.PathLike,
                                Mapping[str, torch.Tensor]] = None,
                 tokenize: Optional[Callable[[str], torch.Tensor]] = None,
                 vision_heads: Optional[int] = None,
                 text_heads: Optional[int] = None,
                 **kwargs: Any):
        """`name`, `jit` and **kwargs go to `clip.load` when `weights` is not
        given.  `device` is kept for serialisation only: the work runs on the
        GPU of the images (or of `.to(...)`)."""
        super().__init__()
        if (source_mean is None) != (source_std is None):
            raise ValueError('set neither or both of source_mean/source_std')
        self.name, self.jit, self.load_device = name, jit, device
        target_mean, target_std = CLIP_MEAN, CLIP_STD
        if weights is None:
            weights, heads, target_mean, target_std = _load_clip(name, jit, kwargs)
            vision_heads = vision_heads or heads.get('vision_heads')
            text_heads = text_heads or heads.get('text_heads')
        elif not isinstance(weights, Mapping):
            weights = torch.load(weights, map_location='cpu', weights_only=True)
        self.dims = infer_dims(weights, vision_heads, text_heads)
        self.weights = {
            key: value.detach().to('cpu', torch.float32)
            for key, value in weights.items()
            if isinstance(value, torch.Tensor) and value.dtype.is_floating_point
        }
        if source_mean is None or source_std is None:
            source_mean, source_std = SOURCE_MEAN, SOURCE_STD
        # the reference's Renormalizer: float64 constants, cast to the data's dtype
        self.renorm_mul_add = tuple(
            [float(s) / float(t) for s, t in zip(source_std, target_std)] +
            [(float(s) - float(t)) / float(u)
             for s, t, u in zip(source_mean, target_mean, target_std)])
        layers = self.dims['vision_layers']
        if mask_layers is None:
            self.mask_layers: Sequence[int] = tuple(range(layers))
        else:
            self.mask_layers = mask_layers
        for layer in self.mask_layers:
            if not 0 <= int(layer) < min(layers, 64):
                raise ValueError(f'mask layer {layer} is not one of the '
                                 f'{layers} visual blocks')
        self.tokenize = tokenize
        # truncate the text tower at the longest caption (exact: it is causal)
        self.truncate_text = True
        self._device: Optional[torch.device] = None
        self._ctx: Optional[hip.ClipContext] = None

    # -- reference properties ---------------------------------------------------
    @property
    def num_patches(self) -> int:
        """Return number of patches used by CLIP ViT."""
        return (self.dims['resolution'] // self.dims['patch'])**2

    @property
    def num_patches_xy(self) -> int:
        """Return number of patches in each dimension of patch grid."""
        return math.isqrt(self.num_patches)

    @property
    def input_resolution(self) -> int:
        """Return input resolution for CLIP model."""
        return self.dims['resolution']

    # -- device plumbing --------------------------------------------------------
    def _apply(self, fn, *args, **kwargs):
        probe = fn(torch.empty(0))
        if probe.device.type == 'cuda':
            self._device = probe.device
        return super()._apply(fn, *args, **kwargs)

    def _context(self, device: torch.device) -> hip.ClipContext:
        device = hip.require_device(device)
        if self._ctx is None or self._ctx.device != device:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.ClipContext(hip.ClipDims(**self.dims), self.weights,
                                        device)
        return self._ctx

    def _pick_device(self, images: torch.Tensor) -> torch.device:
        if images.is_cuda:
            return images.device
        return self._device if self._device is not None else torch.device('cuda')

    @property
    def mask_bits(self) -> int:
        bits = 0
        for layer in self.mask_layers:
            bits |= 1 << int(layer)
        return bits

    # -- the two towers ---------------------------------------------------------
    def tokens(self, texts: Union[StrSequence, torch.Tensor]) -> torch.Tensor:
        """(len(texts), context) token ids of `texts` (a LongTensor passes)."""
        context = self.dims['context_length']
        if isinstance(texts, torch.Tensor):
            ids = texts
        else:
            tokenize = self.tokenize
            if tokenize is None:
                try:
                    import clip
                except ImportError as error:
                    raise NotImplementedError(
                        'CLIP\'s tokenizer (the `clip` package) is not '
                        'installed: pass tokenize=<callable str -> LongTensor '
                        f'(1, {context})> to CLIPWithMasks, or token ids in '
                        'place of texts') from error
                tokenize = clip.tokenize
            if len(texts) == 0:
                return torch.zeros(0, context, dtype=torch.long)
            ids = torch.cat([tokenize(text) for text in texts])
        if ids.dim() != 2 or ids.shape[1] != context or ids.dtype != torch.long:
            raise ValueError(f'token ids must be a LongTensor (rows, {context}), '
                             f'got {ids.dtype} {tuple(ids.shape)}')
        if ids.numel() and (int(ids.min()) < 0 or
                            int(ids.max()) >= self.dims['vocab_size']):
            raise IndexError('index out of range in self')  # nn.Embedding
        return ids

    def encode_texts(self, texts: Union[StrSequence, torch.Tensor],
                     device: Optional[torch.device] = None) -> torch.Tensor:
        """L2-normalised text embeddings (rows, embed) on the GPU."""
        ids = self.tokens(texts)
        ctx = self._context(device or self._device or torch.device('cuda'))
        positions = self.dims['context_length']
        if self.truncate_text and len(ids):
            positions = int(ids.argmax(dim=-1).max()) + 1
        return ctx.encode_texts(ids, positions)

    def _check_images(self, images: torch.Tensor, resize: bool,
                      renormalize: bool) -> None:
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError('images must have shape (batch_size, 3, height, '
                             f'width), got {tuple(images.shape)}')
        res = self.input_resolution
        if tuple(images.shape[-2:]) == (res, res):
            return
        if resize and not renormalize:
            raise NotImplementedError(
                'resize=True, renormalize=False is the one path on which the '
                'reference resizes (bicubic); it is not built. Resize the '
                f'images to {res} x {res} first')
        # the reference's default path renormalises the unresized images and
        # fails in the position-embedding add (rerankers.py:185)
        tokens = (images.shape[-2] // self.dims['patch']) * (
            images.shape[-1] // self.dims['patch'])
        raise RuntimeError(
            f'The size of tensor a ({tokens + 1}) must match the size of tensor b '
            f'({self.num_patches + 1}) at non-singleton dimension 1: images are '
            f'{images.shape[-2]} x {images.shape[-1]}, CLIP takes {res} x {res} '
            '(the reference discards its resized tensor when renormalize=True)')

    def encode_images(self, images: torch.Tensor,
                      masks: Optional[torch.Tensor] = None,
                      both: bool = False,
                      resize: bool = True,
                      renormalize: bool = True) -> torch.Tensor:
        """L2-normalised image embeddings (n, embed), masked when `masks` is
        given; `both`: (2, n, embed) = (masked, unmasked) in one batch."""
        self._check_images(images, resize, renormalize)
        ctx = self._context(self._pick_device(images))
        return ctx.encode_images(
            images, masks, self.mask_bits, both,
            self.renorm_mul_add if renormalize else None)

    def forward(self,
                images: torch.Tensor,
                texts: Union[StrSequence, torch.Tensor],
                masks: Optional[torch.Tensor] = None,
                resize: bool = True,
                renormalize: bool = True) -> torch.Tensor:
        """Cosine similarities (batch_size, len(texts)) between the images and
        the texts (reference :151-232; no logit scale, no softmax)."""
        if masks is not None and len(masks) != len(images):
            raise ValueError('images and masks batch sizes do not align: '
                             f'{len(images)} vs. {len(masks)}')
        device = self._pick_device(images)
        image_emb = self.encode_images(images, masks, resize=resize,
                                       renormalize=renormalize)
        text_emb = self.encode_texts(texts, device)
        # The cosine matrix through the score kernel, so that its dot products are summed in
        # the same order as the reranker's: every image is a "neuron" with k = 1 that scores
        # all rows; with lam = 0 and the same tensor as masked and unmasked the mix is the
        # plain dot product.
        n, rows = len(image_emb), len(text_emb)
        ctx = self._context(device)
        neuron_of = torch.arange(n, dtype=torch.int32).repeat_interleave(rows)
        sims = ctx.rerank_scores(image_emb[:, None], image_emb[:, None],
                                 text_emb.repeat(n, 1), neuron_of, rows, 0.)
        sims = sims.view(n, rows)
        return sims if images.is_cuda else sims.to(images.device)


class RerankerOutput(NamedTuple):
    """Output of a reranking algorithm."""

    texts: Sequence[StrSequence]
    orders: Sequence[Sequence[int]]
    scores: Sequence[Sequence[float]]


class CLIPWithMasksReranker(nn.Module):
    """Rerank sampled captions using CLIP (reference :264-330)."""

    def __init__(self, clip_with_masks: CLIPWithMasks, lam: float = .5):
        super().__init__()
        self.clip_with_masks = clip_with_masks
        self.lam = lam
        # images per call of the image tower (both copies of 64 neurons x 15
        # images at ViT-B/32 take ~5 GB of workspace)
        self.max_images = 960

    def similarities(self,
                     images: torch.Tensor,
                     masks: torch.Tensor,
                     texts: Sequence[Union[StrSequence, torch.Tensor]],
                     lam: Optional[float] = None) -> Tuple[torch.Tensor, ...]:
        """Per neuron, the rerank score of every candidate (unsorted), on the
        GPU."""
        if len(images) != len(masks):
            raise ValueError('images and masks batch sizes do not align: '
                             f'{len(images)} vs. {len(masks)}')
        if len(images) != len(texts):
            raise ValueError('images and texts batch sizes do not align: '
                             f'{len(images)} vs. {len(texts)}')
        if lam is None:
            lam = self.lam
        clip = self.clip_with_masks
        neurons = len(images)
        if neurons == 0:
            return ()
        if images.dim() != 5:
            raise ValueError('images must have shape (batch_size, k, 3, height, '
                             f'width), got {tuple(images.shape)}')
        k = images.shape[1]
        device = clip._pick_device(images)
        ids = [clip.tokens(t) for t in texts]
        counts = [len(i) for i in ids]
        text_emb = clip.encode_texts(torch.cat(ids), device)
        flat_images = images.reshape(neurons * k, *images.shape[2:])
        flat_masks = masks.reshape(neurons * k, 1, *masks.shape[-2:])
        per = max(1, self.max_images // k) * k
        masked, unmasked = [], []
        for lo in range(0, neurons * k, per):
            chunk = flat_images[lo:lo + per]
            if chunk.dtype == torch.uint8:
                # the floats the reference's dataset makes of bytes: x * float32(1 / 255)
                scale = torch.tensor(1. / 255., dtype=torch.float64).to(torch.float32)
                chunk = chunk.to(device).float().mul(scale.to(device))
            emb = clip.encode_images(chunk, flat_masks[lo:lo + per], both=True)
            masked.append(emb[0])
            unmasked.append(emb[1])
        masked = torch.cat(masked).view(neurons, k, -1)
        unmasked = torch.cat(unmasked).view(neurons, k, -1)
        neuron_of = torch.repeat_interleave(
            torch.arange(neurons, dtype=torch.int32), torch.tensor(counts))
        sims = clip._context(device).rerank_scores(masked, unmasked, text_emb,
                                                   neuron_of, 0, lam)
        return tuple(sims.split(counts))

    def forward(
        self,
        images: torch.Tensor,
        masks: torch.Tensor,
        texts: Sequence[Union[StrSequence, torch.Tensor]],
        lam: Optional[float] = None,
    ) -> RerankerOutput:
        """Rerank each neuron's candidate `texts` by CLIP's agreement with its
        top images (batch_size, k, 3, h, w) and masks (batch_size, k, 1, h, w).
        A neuron's candidates may be given as token ids (rows, context); its
        `texts` in the output are then the row numbers."""
        sims = self.similarities(images, masks, texts, lam=lam)
        rerankeds, orders, scores = [], [], []
        for b_texts, sim in zip(texts, sims):
            scoring, indices = sim.sort(descending=True, stable=True)
            indices = indices.tolist()
            if isinstance(b_texts, torch.Tensor):
                reranked = indices
            else:
                reranked = [b_texts[index] for index in indices]
            rerankeds.append(tuple(reranked))
            orders.append(tuple(indices))
            scores.append(tuple(scoring.tolist()))
        return RerankerOutput(tuple(rerankeds), tuple(orders), tuple(scores))


def reranker(lam: float = 1., **kwargs: Any) -> CLIPWithMasksReranker:
    """Create a new CLIPWithMasksReranker.

    The **kwargs are forwarded to CLIPWithMasks.
    """
    clip_with_masks = CLIPWithMasks(**kwargs)
    return CLIPWithMasksReranker(clip_with_masks, lam=lam)
