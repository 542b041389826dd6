"""DINO's vision transformer with a native forward and taps on `blocks.N.mlp.fc1`.

`dino_vits8/imagenet` is the transformer the reference dissects (`src/exemplars/models.py`:
`LAYERS.DINO_VITS8 = blocks.{0..11}.mlp.fc1`, `transform_hiddens=spatialize_vit_mlp`).
`VisionTransformer` is an `nn.Module` with the module tree and key names of
`facebookresearch/dino`'s `vision_transformer.py`, so a DINO checkpoint loads with
`load_state_dict(strict=True)`.  Weights come from the user; nothing is fetched.

`forward(images)` -> (B, embed_dim), the CLS row after the final norm;
`activations(images, layers)` -> {name: (B, tokens, hidden)}, the outputs of the named
modules.  Both run in libmilan_hip (`hip.VitContext`: exact-fp32 MFMA GEMMs and streaming
attention, one walk that stops after the deepest layer asked for) when the module is in eval
mode, grad is disabled, the images are on the GPU and no forward hook is registered on any
sub-module.  Otherwise `forward_eager` runs: plain torch modules, differentiable, hooks fire.
The native walk runs no sub-module, so it is not taken while a hook is present.

Only `img_size` x `img_size` images are taken: DINO's bicubic interpolation of the position
embedding for other sizes is not built.  Dropout and drop-path are 0 in every DINO model and
are not built either.  Non-finite inputs are not specified.
"""
import math
from typing import Dict, Mapping, Optional, Tuple

import torch
from torch import nn

from milan_amd import hip

EPS = 1e-6


class PatchEmbed(nn.Module):

    def __init__(self, img_size, patch_size, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(3, embed_dim, kernel_size=patch_size, stride=patch_size)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class Attention(nn.Module):

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads)**-0.5
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads)
        q, k, v = qkv.permute(2, 0, 3, 1, 4)
        attn = ((q @ k.transpose(-2, -1)) * self.scale).softmax(dim=-1)
        return self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):

    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):

    def __init__(self, dim, num_heads, hidden):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=EPS)
        self.attn = Attention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim, eps=EPS)
        self.mlp = Mlp(dim, hidden)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class VisionTransformer(nn.Module):
    """DINO's ViT (no distillation token, no head).  `layers` names the taps the native walk
    serves; `max_images` is the number of images per native pass (larger batches are split;
    an image's result does not depend on the split)."""

    def __init__(self,
                 img_size: int = 224,
                 patch_size: int = 8,
                 embed_dim: int = 384,
                 depth: int = 12,
                 num_heads: int = 6,
                 mlp_ratio: float = 4.,
                 max_images: int = 64):
        super().__init__()
        if img_size % patch_size:
            raise ValueError(f'img_size {img_size} is not a multiple of patch_size {patch_size}')
        if embed_dim % num_heads:
            raise ValueError(f'embed_dim {embed_dim} is not a multiple of num_heads {num_heads}')
        self.img_size, self.patch_size = int(img_size), int(patch_size)
        self.embed_dim, self.depth, self.num_heads = int(embed_dim), int(depth), int(num_heads)
        self.hidden = int(embed_dim * mlp_ratio)
        self.max_images = int(max_images)
        tokens = (self.img_size // self.patch_size)**2 + 1
        self.patch_embed = PatchEmbed(img_size, patch_size, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, tokens, embed_dim))
        self.blocks = nn.ModuleList(
            [Block(embed_dim, num_heads, self.hidden) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=EPS)
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.layers: Tuple[str, ...] = tuple(f'blocks.{i}.mlp.fc1' for i in range(depth))
        self._ctx: Optional[hip.VitContext] = None
        self._ctx_key = None

    @property
    def tokens(self) -> int:
        return self.pos_embed.shape[1]

    # -- the two forwards -------------------------------------------------------------
    def _check_size(self, images: torch.Tensor) -> None:
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'images must be (B, 3, H, W), got {tuple(images.shape)}')
        if images.shape[2] != self.img_size or images.shape[3] != self.img_size:
            raise NotImplementedError(
                f'images are {images.shape[2]} x {images.shape[3]}, the model was built for '
                f'{self.img_size} x {self.img_size}: DINO\'s bicubic position-embedding '
                'interpolation for other sizes is not built')

    def forward_eager(self, images: torch.Tensor) -> torch.Tensor:
        """DINO's `VisionTransformer.forward` on this module's own sub-modules."""
        self._check_size(images)
        x = self.patch_embed(images)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1) + self.pos_embed
        for block in self.blocks:
            x = block(x)
        return self.norm(x)[:, 0]

    def runs_natively(self, images: torch.Tensor) -> bool:
        return (not self.training and not torch.is_grad_enabled() and
                images.device.type == 'cuda' and
                not any(m._forward_hooks or m._forward_pre_hooks for m in self.modules()))

    def _native(self, images: torch.Tensor, taps=(), want_output=False):
        self._check_size(images)
        ctx = self._context()
        step = max(1, self.max_images)
        if images.shape[0] <= step:
            return ctx.run(images, taps, want_output)
        parts = [ctx.run(images[i:i + step], taps, want_output)
                 for i in range(0, images.shape[0], step)]
        outs = {t: torch.cat([p[0][t] for p in parts]) for t in parts[0][0]}
        return outs, (torch.cat([p[1] for p in parts]) if want_output else None)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        if not self.runs_natively(images):
            return self.forward_eager(images)
        return self._native(images, want_output=True)[1]

    def activations(self, images: torch.Tensor, layers) -> Dict[str, torch.Tensor]:
        """The outputs of the named modules for `images` (what `nethook.retain_layers`
        retains).  `layers`: a name or a sequence of names from `named_modules()`; an unknown
        name is a KeyError.  When the forward would run natively and every name is one of
        `self.layers`, one native walk up to the deepest of them; anything else runs
        `forward_eager` under `no_grad` with forward hooks."""
        names = [layers] if isinstance(layers, str) else list(layers)
        modules = dict(self.named_modules())
        for name in names:
            if not name or name not in modules:
                raise KeyError(f'layer not found: {name}')
        if self.runs_natively(images) and all(name in self.layers for name in names):
            index = {name: self.layers.index(name) for name in names}
            outs, _ = self._native(images, taps=index.values())
            return {name: outs[index[name]] for name in names}
        self._check_size(images)
        retained: Dict[str, torch.Tensor] = {}
        handles = []

        def retain(name):
            def hook(module, inputs, output):
                retained[name] = output.detach()
            return hook

        for name in dict.fromkeys(names):
            handles.append(modules[name].register_forward_hook(retain(name)))
        try:
            with torch.no_grad():
                self.forward_eager(images)
        finally:
            for handle in handles:
                handle.remove()
        return {name: retained[name] for name in names}

    # -- HIP context, rebuilt when device or weights change ---------------------------
    def dims(self) -> hip.VitDims:
        return hip.VitDims(resolution=self.img_size, patch=self.patch_size, width=self.embed_dim,
                           layers=self.depth, heads=self.num_heads, hidden=self.hidden,
                           eps=self.norm.eps)

    def _context(self) -> hip.VitContext:
        device = hip.require_device(self.pos_embed.device)
        tensors = list(self.parameters()) + list(self.buffers())
        key = (device, tuple(t._version for t in tensors),
               tuple(t.data_ptr() for t in tensors))
        if self._ctx is None or self._ctx_key != key:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.VitContext(self.dims(), self.state_dict(), device)
            self._ctx_key = key
        return self._ctx


def dino_vits8(**kwargs) -> VisionTransformer:
    """ViT-S/8: 224 x 224, 785 tokens, width 384, 12 blocks, 6 heads."""
    return VisionTransformer(patch_size=8, embed_dim=384, depth=12, num_heads=6, **kwargs)


def dino_vits16(**kwargs) -> VisionTransformer:
    """ViT-S/16: 224 x 224, 197 tokens, width 384, 12 blocks, 6 heads."""
    return VisionTransformer(patch_size=16, embed_dim=384, depth=12, num_heads=6, **kwargs)


def infer_dims(state_dict: Mapping[str, torch.Tensor],
               num_heads: Optional[int] = None) -> Dict[str, object]:
    """Constructor arguments of the model a DINO state dict belongs to (heads = width // 64
    unless given)."""
    try:
        conv = state_dict['patch_embed.proj.weight']
        tokens = state_dict['pos_embed'].shape[1]
        depth = len([k for k in state_dict if k.startswith('blocks.') and
                     k.endswith('.mlp.fc1.weight')])
        hidden = state_dict['blocks.0.mlp.fc1.weight'].shape[0]
    except KeyError as error:
        raise ValueError(f'not a DINO ViT state dict: no {error}') from error
    width, patch = conv.shape[0], conv.shape[-1]
    grid = math.isqrt(tokens - 1)
    if grid * grid + 1 != tokens:
        raise ValueError(f'{tokens} tokens are not a square grid + 1')
    return dict(img_size=patch * grid, patch_size=patch, embed_dim=width, depth=depth,
                num_heads=num_heads or max(1, width // 64), mlp_ratio=hidden / width)


def from_state_dict(state_dict: Mapping[str, torch.Tensor],
                    num_heads: Optional[int] = None, **kwargs) -> VisionTransformer:
    """The model a DINO state dict belongs to, with the weights loaded (strict), in eval
    mode."""
    model = VisionTransformer(**infer_dims(state_dict, num_heads), **kwargs)
    model.load_state_dict(state_dict, strict=True)
    return model.eval()
