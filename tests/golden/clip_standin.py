"""Stand-in for OpenAI's `clip` package: the ViT and text branches of its model
restated from the published architecture (Radford et al. 2021; ViT of
Dosovitskiy et al. 2021), with the package's state-dict layout and the three
entry points the reference's reranker uses: `load`, `tokenize`, and the model's
`encode_image` / `encode_text`.  Test infrastructure, like allennlp_standin.py:
random weights, tiny dims, a word-hash tokenizer.  It imports nothing from the
reference.
"""
import zlib
from collections import OrderedDict

import torch
from torch import nn

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
DEFAULTS = dict(resolution=64, patch=16, vision_width=32, vision_layers=2,
                vision_heads=4, embed_dim=16, context_length=16, vocab_size=64,
                text_width=24, text_layers=2, text_heads=3)


class QuickGELU(nn.Module):

    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):

    def __init__(self, width, heads, attn_mask=None):
        super().__init__()
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(
            OrderedDict([('c_fc', nn.Linear(width, width * 4)),
                         ('gelu', QuickGELU()),
                         ('c_proj', nn.Linear(width * 4, width))]))
        self.ln_2 = nn.LayerNorm(width)
        self.attn_mask = attn_mask

    def attention(self, x):
        mask = None
        if self.attn_mask is not None:
            mask = self.attn_mask.to(dtype=x.dtype, device=x.device)
        return self.attn(x, x, x, need_weights=False, attn_mask=mask)[0]

    def forward(self, x):
        x = x + self.attention(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):

    def __init__(self, width, layers, heads, attn_mask=None):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[
            ResidualAttentionBlock(width, heads, attn_mask)
            for _ in range(layers)
        ])

    def forward(self, x):
        return self.resblocks(x)


class VisionTransformer(nn.Module):

    def __init__(self, input_resolution, patch_size, width, layers, heads,
                 output_dim):
        super().__init__()
        self.input_resolution = input_resolution
        self.output_dim = output_dim
        self.conv1 = nn.Conv2d(3, width, patch_size, patch_size, bias=False)
        scale = width**-.5
        tokens = (input_resolution // patch_size)**2 + 1
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(tokens, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def forward(self, x):
        x = self.conv1(x)  # (n, width, grid, grid)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
        cls = self.class_embedding.to(x.dtype) + torch.zeros(
            x.shape[0], 1, x.shape[-1], dtype=x.dtype, device=x.device)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.ln_pre(x)
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)
        return self.ln_post(x[:, 0, :]) @ self.proj


class CLIP(nn.Module):

    def __init__(self, resolution, patch, vision_width, vision_layers,
                 vision_heads, embed_dim, context_length, vocab_size, text_width,
                 text_layers, text_heads):
        super().__init__()
        self.context_length, self.vocab_size = context_length, vocab_size
        self.visual = VisionTransformer(resolution, patch, vision_width,
                                        vision_layers, vision_heads, embed_dim)
        mask = torch.full((context_length, context_length), float('-inf')).triu_(1)
        self.transformer = Transformer(text_width, text_layers, text_heads, mask)
        self.token_embedding = nn.Embedding(vocab_size, text_width)
        self.positional_embedding = nn.Parameter(
            .01 * torch.randn(context_length, text_width))
        self.ln_final = nn.LayerNorm(text_width)
        self.text_projection = nn.Parameter(
            text_width**-.5 * torch.randn(text_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * 2.6592)
        # (so that LayerNorms and biases are not the identity in tests)
        for name, p in self.named_parameters():
            if name.endswith('bias') or 'ln_' in name:
                p.data.add_(.1 * torch.randn_like(p))

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        return self.visual(image.type(self.dtype))

    def encode_text(self, text):
        x = self.token_embedding(text).type(self.dtype)
        x = x + self.positional_embedding.type(self.dtype)
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)
        x = self.ln_final(x).type(self.dtype)
        return x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection


class _Normalize:
    mean, std = MEAN, STD


class _Preprocess:
    transforms = [_Normalize()]


_CURRENT = dict(DEFAULTS)
SEED = 0


def configure(seed=0, **dims):
    """Dims / seed of the model the next `load` builds (and `tokenize` serves)."""
    global SEED
    SEED = seed
    _CURRENT.clear()
    _CURRENT.update(DEFAULTS)
    _CURRENT.update(dims)


def available_models():
    return ['ViT-B/32']


def load(name='ViT-B/32', jit=False, device='cpu', **_kwargs):
    generator_state = torch.get_rng_state()
    torch.manual_seed(SEED)
    model = CLIP(**_CURRENT).to(device).eval()
    torch.set_rng_state(generator_state)
    return model, _Preprocess()


def tokenize(texts, context_length=None, truncate=True):
    """<start> = vocab - 2, <end of text> = vocab - 1 (the largest id, as in
    CLIP's BPE vocabulary), words hashed into [1, vocab - 3]."""
    if isinstance(texts, str):
        texts = [texts]
    vocab = _CURRENT['vocab_size']
    context = context_length or _CURRENT['context_length']
    out = torch.zeros(len(texts), context, dtype=torch.long)
    for row, text in enumerate(texts):
        words = [1 + zlib.crc32(w.encode()) % (vocab - 3) for w in text.split()]
        ids = [vocab - 2] + words[:context - 2] + [vocab - 1]
        out[row, :len(ids)] = torch.tensor(ids)
    return out
