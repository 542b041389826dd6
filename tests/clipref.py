"""The masked CLIP forward and the reranker as plain functions of a state dict
(OpenAI's layout), in whatever dtype the state dict has: float64 gives the
yardstick the GPU tests measure errors against (the trainref.py pattern).
Pinned to the reference's own outputs by tests/test_clip_ref_host.py.
"""
import math

import torch
from torch.nn import functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}


def _ln(x, sd, prefix):
    return F.layer_norm(x, x.shape[-1:], sd[prefix + '.weight'], sd[prefix + '.bias'], 1e-5)


def _block(x, sd, prefix, heads, causal=False, cls_mask=None):
    """x: (seqs, T, W).  cls_mask: (seqs, T - 1) multiplied into the CLS query's
    post-softmax weights on the patch keys, or None."""
    n, t, w = x.shape
    hd = w // heads
    y = _ln(x, sd, prefix + 'ln_1')
    qkv = y @ sd[prefix + 'attn.in_proj_weight'].T + sd[prefix + 'attn.in_proj_bias']
    q, k, v = (z.view(n, t, heads, hd).transpose(1, 2) for z in qkv.chunk(3, dim=-1))
    att = (q / math.sqrt(hd)) @ k.transpose(-2, -1)
    if causal:
        att = att + torch.full((t, t), float('-inf'), dtype=x.dtype).triu_(1)
    att = att.softmax(dim=-1)
    if cls_mask is not None:
        att = att.clone()
        att[:, :, 0, 1:] = att[:, :, 0, 1:] * cls_mask[:, None, :]
    out = (att @ v).transpose(1, 2).reshape(n, t, w)
    x = x + out @ sd[prefix + 'attn.out_proj.weight'].T + sd[prefix + 'attn.out_proj.bias']
    y = _ln(x, sd, prefix + 'ln_2')
    h = y @ sd[prefix + 'mlp.c_fc.weight'].T + sd[prefix + 'mlp.c_fc.bias']
    h = h * torch.sigmoid(1.702 * h)
    return x + h @ sd[prefix + 'mlp.c_proj.weight'].T + sd[prefix + 'mlp.c_proj.bias']


def n_layers(sd, prefix):
    return len({k[len(prefix):].split('.')[0] for k in sd if k.startswith(prefix)})


def renormalize(images, source_mean=(0., 0., 0.), source_std=(1., 1., 1.)):
    mul = torch.tensor([s / t for s, t in zip(source_std, CLIP_STD)], dtype=torch.float64)
    add = torch.tensor([(s - t) / u for s, t, u in zip(source_mean, CLIP_MEAN, CLIP_STD)],
                       dtype=torch.float64)
    mul, add = mul.to(images.dtype), add.to(images.dtype)
    return images * mul[None, :, None, None] + add[None, :, None, None]


def encode_images(sd, heads, images, masks=None, mask_layers=None, renorm=True):
    """L2-normalised (n, embed).  images (n, 3, R, R), masks (n, 1, R, R) or None."""
    dtype = sd['visual.proj'].dtype
    x = images.to(dtype)
    if renorm:
        x = renormalize(x)
    patch = sd['visual.conv1.weight'].shape[-1]
    x = F.conv2d(x, sd['visual.conv1.weight'], stride=patch)
    n, w, g, _ = x.shape
    x = x.reshape(n, w, g * g).permute(0, 2, 1)
    cls = sd['visual.class_embedding'].expand(n, 1, w)
    x = torch.cat([cls, x], dim=1) + sd['visual.positional_embedding']
    x = _ln(x, sd, 'visual.ln_pre')
    layers = n_layers(sd, 'visual.transformer.resblocks.')
    if mask_layers is None:
        mask_layers = range(layers)
    cm = None
    if masks is not None:
        cm = F.interpolate(masks.to(dtype), size=(g, g), mode='bilinear',
                           align_corners=False).view(n, g * g)
    for layer in range(layers):
        x = _block(x, sd, f'visual.transformer.resblocks.{layer}.', heads,
                   cls_mask=cm if layer in mask_layers else None)
    x = _ln(x[:, 0], sd, 'visual.ln_post') @ sd['visual.proj']
    return x / x.norm(dim=-1, keepdim=True)


def encode_texts(sd, heads, tokens, positions=None):
    """L2-normalised (rows, embed), over the first `positions` positions (all
    by default)."""
    t = tokens.shape[1] if positions is None else positions
    eot = tokens.argmax(dim=-1)
    x = sd['token_embedding.weight'][tokens[:, :t]] + sd['positional_embedding'][:t]
    for layer in range(n_layers(sd, 'transformer.resblocks.')):
        x = _block(x, sd, f'transformer.resblocks.{layer}.', heads, causal=True)
    x = _ln(x, sd, 'ln_final')
    x = x[torch.arange(len(x)), eot] @ sd['text_projection']
    return x / x.norm(dim=-1, keepdim=True)


def similarities(sd, vision_heads, text_heads, images, tokens, masks=None, mask_layers=None):
    """CLIPWithMasks.forward: (n, rows) cosines."""
    a = encode_images(sd, vision_heads, images, masks, mask_layers)
    b = encode_texts(sd, text_heads, tokens)
    return a[:, None].mul(b[None]).sum(dim=-1)


def rerank_scores(sd, vision_heads, text_heads, images, masks, tokens, lam, mask_layers=None):
    """Per neuron the unsorted rerank scores.  images (neurons, k, 3, R, R), masks
    (neurons, k, 1, R, R), tokens: a list of (rows_i, context) id tensors."""
    out = []
    for b_images, b_masks, b_tokens in zip(images, masks, tokens):
        masked = similarities(sd, vision_heads, text_heads, b_images, b_tokens, b_masks,
                              mask_layers).sum(dim=0)
        unmasked = similarities(sd, vision_heads, text_heads, b_images, b_tokens).sum(dim=0)
        out.append((1. - lam) * masked + lam * unmasked)
    return out


WORDS = ('a', 'the', 'dog', 'sky', 'blue', 'red', 'grass', 'tree', 'edge',
         'of', 'and', 'stripes', 'round', 'things', 'water', 'face')


# Seeded inputs of the golden cases (tests/golden/make_golden_clip.py draws them, the tests
# draw them again): images, masks ('random' / 'zeros' / 'ones') and ragged captions.
def synthetic_captions(generator, count, longest):
    out = []
    for _ in range(count):
        n = int(torch.randint(1, longest + 1, (1,), generator=generator))
        ids = torch.randint(0, len(WORDS), (n,), generator=generator).tolist()
        out.append(' '.join(WORDS[i] for i in ids))
    return out


def synthetic_inputs(dims, neurons, k, counts, kind, seed):
    g = torch.Generator().manual_seed(seed)
    res = dims['resolution']
    images = torch.randn(neurons, k, 3, res, res, generator=g)
    if kind == 'zeros':
        masks = torch.zeros(neurons, k, 1, res, res)
    elif kind == 'ones':
        masks = torch.ones(neurons, k, 1, res, res)
    else:
        masks = (torch.rand(neurons, k, 1, res, res, generator=g) > .6).float()
        masks = masks * torch.rand(neurons, k, 1, res, res, generator=g)
    texts = [synthetic_captions(g, c, dims['context_length'] - 2) for c in counts]
    return images, masks, texts


# The encoder of the end-to-end DecoderWithCLIP golden: masked pixels average-pooled to
# 3 x 4 x 4 = 48 features per image.  The generator wraps it in the reference's Encoder, the
# GPU test in this project's, so both decoders see the same features.
POOL_FEATURES = 48


def pool_features(images, masks=None):
    x = images if masks is None else images * masks
    return 16. * F.adaptive_avg_pool2d(x, 4).flatten(1)  # (spread: pooled noise is near 0)


# dims of that golden's synthetic decoder and inputs
DECODER_CASE = dict(config='small', nvocab=30, hidden=32, emb=8, length=6, beam=6, neurons=3,
                    k=3, lam=.5, weight_seed=9, input_seed=31)
