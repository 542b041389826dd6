"""BigGAN's generator with a native forward and taps on its blocks.

`biggan/imagenet` and `biggan/places365` are the generators the reference dissects
(`src/exemplars/models.py`: `LAYERS.BIGGAN = layer0 .. layer5`, batch 32, 256 x 256).
`Generator` is an `nn.Module` with the module tree and key names of pretorched's
`gans/biggan.py` (`shared`, `linear`, `blocks.i.0.{conv1,conv2,conv_sc,bn1,bn2}`,
`blocks.i.1.{theta,phi,g,o,gamma}`, `output_layer.0/.2`, the spectral-norm buffers `u0` / `sv0`
and the batch-norm buffers `stored_mean` / `stored_var` included), so a pretorched checkpoint
loads with `load_state_dict(strict=True)`.  Weights come from the user; nothing is fetched.

`SeqBigGAN(generator)` is the `nn.Sequential` the reference hooks: children `preprocess`,
`layer0`, ..., `attnK` after the block at the attention resolution, ..., `output`; it takes
`GInputs(z, y)` (y: class indices or soft labels; always embedded) and hands
`GBlockDataBag(h, ys)` from child to child.  `generate(inputs, layer, images)` returns
(the bag after `layer` or None, the images or None).

Both run in libmilan_hip (`hip.GanContext`: exact-fp32 MFMA convolutions, conditional batch
norms folded to one scale and shift per sample and channel, the streaming attention of
`milan_sagan_attention`; one walk that stops after the deepest layer asked for when no
images are wanted) when the module is in eval mode, grad is disabled, the inputs are on the
GPU, no forward hook is registered on any sub-module and the attention block has a width the
kernel takes.  Otherwise `forward_eager` runs: plain torch modules, differentiable, hooks
fire.  The native walk runs no sub-module, so it is not taken while a hook is present.

Eval mode is what dissection uses and what the native walk covers.  In training mode the
eager modules normalise with batch statistics and spectral norm updates `u0`, as pretorched's
do; the running statistics are not updated (pretorched's `F.batch_norm` call does update them).
Non-finite inputs are not specified.
"""
import collections
import math
from typing import Any, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from milan_amd import hip

# channel multipliers (in, out) of the GBlocks per output resolution (appendix B of the paper)
ARCH = {
    512: ((16, 16, 8, 8, 4, 2, 1), (16, 8, 8, 4, 2, 1, 1)),
    256: ((16, 16, 8, 8, 4, 2), (16, 8, 8, 4, 2, 1)),
    128: ((16, 16, 8, 4, 2), (16, 8, 4, 2, 1)),
    64: ((16, 16, 8, 4), (16, 8, 4, 2)),
    32: ((4, 4, 4), (4, 4, 4)),
}
OUT_BN_EPS = 1e-5  # the output batch norm keeps its own default, whatever BN_eps is


class GInputs(NamedTuple):
    """Inputs of the sequential generator."""
    z: torch.Tensor
    y: torch.Tensor


class GBlockDataBag(NamedTuple):
    """What one child of the sequential generator hands to the next."""
    h: torch.Tensor
    ys: Sequence[torch.Tensor]


def sn_sigma(weight: torch.Tensor, u0: torch.Tensor, eps: float = 1e-12):
    """(sv, u): the singular-value estimate of one power iteration from u0 on `weight`
    viewed (out, -1), and the updated left vector."""
    w = weight.reshape(weight.shape[0], -1)
    with torch.no_grad():
        v = F.normalize(u0 @ w, eps=eps)
        u = F.normalize(v @ w.t(), eps=eps)
    return ((v @ w.t()) @ u.t()).squeeze(), u


class _SN:
    """Spectral normalisation of `self.weight`: one power iteration from the buffer `u0`
    per forward; `u0` and `sv0` move in training mode only."""

    def _sn_init(self, outputs: int, eps: float):
        self.sn_eps = eps
        self.register_buffer('u0', torch.randn(1, outputs))
        self.register_buffer('sv0', torch.ones(1))

    def normalised_weight(self) -> torch.Tensor:
        sv, u = sn_sigma(self.weight, self.u0, self.sn_eps)
        if self.training:
            with torch.no_grad():
                self.u0.copy_(u)
                self.sv0.fill_(float(sv))
        return self.weight / sv


class SNConv2d(nn.Conv2d, _SN):

    def __init__(self, cin, cout, kernel_size=3, padding=1, bias=True, eps=1e-12):
        nn.Conv2d.__init__(self, cin, cout, kernel_size, padding=padding, bias=bias)
        self._sn_init(cout, eps)

    def forward(self, x):
        return F.conv2d(x, self.normalised_weight(), self.bias, self.stride, self.padding)


class SNLinear(nn.Linear, _SN):

    def __init__(self, n_in, n_out, bias=True, eps=1e-12):
        nn.Linear.__init__(self, n_in, n_out, bias)
        self._sn_init(n_out, eps)

    def forward(self, x):
        return F.linear(x, self.normalised_weight(), self.bias)


def _conv(sn, eps):
    if sn:
        return lambda cin, cout, kernel_size=3, padding=1, bias=True: SNConv2d(
            cin, cout, kernel_size, padding, bias, eps)
    return lambda cin, cout, kernel_size=3, padding=1, bias=True: nn.Conv2d(
        cin, cout, kernel_size, padding=padding, bias=bias)


def _linear(sn, eps):
    if sn:
        return lambda n_in, n_out, bias=True: SNLinear(n_in, n_out, bias, eps)
    return lambda n_in, n_out, bias=True: nn.Linear(n_in, n_out, bias)


class CCBN(nn.Module):
    """Class-conditional batch norm: (1 + gain(y)) * bn(x) + bias(y)."""

    def __init__(self, channels, cond, linear, eps):
        super().__init__()
        self.gain = linear(cond, channels, bias=False)
        self.bias = linear(cond, channels, bias=False)
        self.eps = eps
        self.register_buffer('stored_mean', torch.zeros(channels))
        self.register_buffer('stored_var', torch.ones(channels))

    def forward(self, x, y):
        gain = (1 + self.gain(y)).view(y.size(0), -1, 1, 1)
        bias = self.bias(y).view(y.size(0), -1, 1, 1)
        if self.training:
            out = F.batch_norm(x, None, None, None, None, True, 0., self.eps)
        else:
            out = F.batch_norm(x, self.stored_mean, self.stored_var, None, None, False, 0.,
                               self.eps)
        return out * gain + bias


class BN(nn.Module):
    """The output layer's plain batch norm, with `gain` / `bias` parameters."""

    def __init__(self, channels, eps=OUT_BN_EPS):
        super().__init__()
        self.gain = nn.Parameter(torch.ones(channels))
        self.bias = nn.Parameter(torch.zeros(channels))
        self.eps = eps
        self.register_buffer('stored_mean', torch.zeros(channels))
        self.register_buffer('stored_var', torch.ones(channels))

    def forward(self, x, y=None):
        if self.training:
            return F.batch_norm(x, None, None, self.gain, self.bias, True, 0., self.eps)
        return F.batch_norm(x, self.stored_mean, self.stored_var, self.gain, self.bias, False,
                            0., self.eps)


class GBlock(nn.Module):

    def __init__(self, cin, cout, conv, bn):
        super().__init__()
        self.conv1 = conv(cin, cout)
        self.conv2 = conv(cout, cout)
        self.conv_sc = conv(cin, cout, kernel_size=1, padding=0)
        self.bn1 = bn(cin)
        self.bn2 = bn(cout)

    def forward(self, x, y):
        h = F.interpolate(F.relu(self.bn1(x, y)), scale_factor=2)
        h = self.conv2(F.relu(self.bn2(self.conv1(h), y)))
        return h + self.conv_sc(F.interpolate(x, scale_factor=2))


class Attention(nn.Module):
    """SAGAN's non-local block; `gamma` starts at 0."""

    def __init__(self, ch, conv):
        super().__init__()
        self.ch = ch
        self.theta = conv(ch, ch // 8, kernel_size=1, padding=0, bias=False)
        self.phi = conv(ch, ch // 8, kernel_size=1, padding=0, bias=False)
        self.g = conv(ch, ch // 2, kernel_size=1, padding=0, bias=False)
        self.o = conv(ch // 2, ch, kernel_size=1, padding=0, bias=False)
        self.gamma = nn.Parameter(torch.tensor(0.))

    def forward(self, x, y=None):
        n, _, hh, ww = x.shape
        theta = self.theta(x).view(n, self.ch // 8, hh * ww)
        phi = F.max_pool2d(self.phi(x), [2, 2]).view(n, self.ch // 8, hh * ww // 4)
        g = F.max_pool2d(self.g(x), [2, 2]).view(n, self.ch // 2, hh * ww // 4)
        beta = F.softmax(torch.bmm(theta.transpose(1, 2), phi), -1)
        o = self.o(torch.bmm(g, beta.transpose(1, 2)).view(n, self.ch // 2, hh, ww))
        return self.gamma * o + x


class Generator(nn.Module):
    """pretorched's BigGAN `Generator` with a shared class embedding (`G_shared=True`, as
    every released BigGAN has).  Argument names are pretorched's.  `max_images` is the number
    of samples per native pass (larger batches are split; a sample's result does not depend
    on the split)."""

    def __init__(self,
                 G_ch: int = 64,
                 dim_z: int = 128,
                 bottom_width: int = 4,
                 resolution: int = 128,
                 G_attn: str = '64',
                 n_classes: int = 1000,
                 shared_dim: int = 0,
                 hier: bool = False,
                 BN_eps: float = 1e-5,
                 SN_eps: float = 1e-12,
                 G_param: str = 'SN',
                 max_images: int = 8,
                 skip_init: bool = False,
                 **ignored: Any):
        super().__init__()
        if resolution not in ARCH:
            raise ValueError(f'resolution {resolution} is not one of {sorted(ARCH)}')
        if G_param not in ('SN', 'none', None):
            raise ValueError(f"G_param {G_param!r}: 'SN' or 'none'")
        ins, outs = ARCH[resolution]
        attn = [int(item) for item in str(G_attn).split('_') if item and int(item)]
        if len(attn) > 1:
            raise NotImplementedError(f'G_attn {G_attn!r}: one attention block is built')
        self.ch, self.bottom_width, self.resolution = int(G_ch), int(bottom_width), resolution
        self.n_classes, self.hier = int(n_classes), bool(hier)
        self.shared_dim = int(shared_dim) if shared_dim > 0 else int(dim_z)
        self.attn_resolution = attn[0] if attn else 0
        self.BN_eps, self.sn = float(BN_eps), G_param == 'SN'
        self.max_images = int(max_images)
        self.num_slots = len(ins) + 1 if hier else 1
        self.z_chunk_size = dim_z // self.num_slots if hier else 0
        self.dim_z = self.z_chunk_size * self.num_slots if hier else int(dim_z)

        conv, linear = _conv(self.sn, SN_eps), _linear(self.sn, SN_eps)
        cond = self.shared_dim + self.z_chunk_size

        def bn(channels):
            return CCBN(channels, cond, linear, self.BN_eps)

        self.shared = nn.Embedding(n_classes, self.shared_dim)
        self.linear = linear(self.dim_z // self.num_slots, self.ch * ins[0] * bottom_width**2)
        blocks: List[nn.ModuleList] = []
        names: List[str] = []
        for i, (a, b) in enumerate(zip(ins, outs)):
            block = [GBlock(self.ch * a, self.ch * b, conv, bn)]
            names.append(f'layer{i}')
            if 8 << i == self.attn_resolution:
                block.append(Attention(self.ch * b, conv))
                names.append(f'attn{i}')
            blocks.append(nn.ModuleList(block))
        self.blocks = nn.ModuleList(blocks)
        self.output_layer = nn.Sequential(BN(self.ch * outs[-1]), nn.ReLU(),
                                          conv(self.ch * outs[-1], 3))
        if not skip_init:  # (weights that are about to be loaded need none)
            for module in self.modules():
                if isinstance(module, (nn.Conv2d, nn.Linear, nn.Embedding)):
                    nn.init.orthogonal_(module.weight)
        self.layers: Tuple[str, ...] = tuple(names)
        self._ctx: Optional[hip.GanContext] = None
        self._ctx_key = None

    @property
    def z_dim(self) -> int:
        return self.dim_z

    @property
    def image_side(self) -> int:
        """Side of the images: every block doubles bottom_width.  `resolution` names the
        block table and is the side only at bottom_width 4."""
        return self.bottom_width << len(self.blocks)

    @property
    def attention_channels(self) -> int:
        """Channels of the attention block, 0 without one."""
        for block in self.blocks:
            if len(block) > 1:
                return block[1].ch
        return 0

    # -- the eager pieces (what SeqBigGAN's children run) ---------------------------------
    def embed(self, y: torch.Tensor) -> torch.Tensor:
        return y @ self.shared.weight if y.ndim > 1 else self.shared(y)

    def preprocess(self, z: torch.Tensor, y: torch.Tensor) -> GBlockDataBag:
        """`y` already embedded -> the first block's input and every block's condition."""
        if self.hier:
            zs = torch.split(z, self.z_chunk_size, 1)
            z, ys = zs[0], [torch.cat([y, item], 1) for item in zs[1:]]
        else:
            ys = [y] * len(self.blocks)
        h = self.linear(z)
        return GBlockDataBag(h.view(h.size(0), -1, self.bottom_width, self.bottom_width), ys)

    def forward_eager(self, z: torch.Tensor, y: torch.Tensor, embed: bool = False):
        """pretorched's `Generator.forward` on this module's own sub-modules."""
        h, ys = self.preprocess(z, self.embed(y) if embed else y)
        for index, blocklist in enumerate(self.blocks):
            for block in blocklist:
                h = block(h, ys[index])
        return torch.tanh(self.output_layer(h))

    # -- which path -----------------------------------------------------------------------
    def native_refusal(self, *tensors: torch.Tensor, roots: Sequence[nn.Module] = ()):
        """None when the native walk would run for these inputs, else why it would not."""
        if self.training:
            return 'the module is in training mode'
        if torch.is_grad_enabled():
            return 'grad is enabled'
        if any(t.device.type != 'cuda' for t in tensors):
            return 'the inputs are not on the GPU'
        for root in (self, *roots):
            if any(m._forward_hooks or m._forward_pre_hooks for m in root.modules()):
                return 'a sub-module carries a forward hook'
        c = self.attention_channels
        if c and (c % 32 or c > 384):
            return (f'the attention block has {c} channels: milan_sagan_attention takes a '
                    'multiple of 32 up to 384')
        side = self.attn_resolution // 4 * self.bottom_width
        if c and side % 2:
            return f'the attention block sees {side} x {side} pixels: the pooling needs even sides'
        if self.ch % 4:
            return f'G_ch {self.ch} is not a multiple of 4'
        return None

    def runs_natively(self, *tensors: torch.Tensor) -> bool:
        return self.native_refusal(*tensors) is None

    def forward(self, z: torch.Tensor, y: torch.Tensor, embed: bool = False) -> torch.Tensor:
        if not self.runs_natively(z, y):
            return self.forward_eager(z, y, embed)
        return self._native(z, y, embedded=not embed, want_images=True)[1]

    def _native(self, z, y, embedded, taps=(), want_images=False):
        ctx = self._context()
        step, n = max(1, self.max_images), z.shape[0]
        if n <= step:
            return ctx.run(z, y, embedded, taps, want_images)
        parts = [ctx.run(z[i:i + step], y[i:i + step], embedded, taps, want_images)
                 for i in range(0, n, step)]
        outs = {t: torch.cat([p[0][t] for p in parts]) for t in parts[0][0]}
        return outs, (torch.cat([p[1] for p in parts]) if want_images else None)

    # -- HIP context, rebuilt when device or weights change -------------------------------
    def dims(self) -> 'hip.GanDims':
        return hip.GanDims(ch=self.ch, dim_z=self.dim_z, shared_dim=self.shared_dim,
                           n_classes=self.n_classes, resolution=self.resolution,
                           bottom_width=self.bottom_width,
                           attn_resolution=self.attn_resolution, hier=int(self.hier),
                           bn_eps=self.BN_eps, out_bn_eps=self.output_layer[0].eps)

    def folded_state_dict(self) -> Dict[str, torch.Tensor]:
        """The state dict with spectral norm folded in: every weight that has a `u0` is
        divided by its eval-mode singular-value estimate, and the SN buffers are dropped."""
        sd = self.state_dict()
        out = {}
        for key, value in sd.items():
            if key.endswith(('.u0', '.sv0')):
                continue
            u0 = sd.get(key[:-len('weight')] + 'u0') if key.endswith('.weight') else None
            if u0 is not None:
                module = self.get_submodule(key[:-len('.weight')])
                value = value / sn_sigma(value, u0, module.sn_eps)[0]
            out[key] = value
        return out

    def _context(self) -> 'hip.GanContext':
        device = hip.require_device(self.shared.weight.device)
        tensors = list(self.parameters()) + list(self.buffers())
        key = (device, tuple(t._version for t in tensors),
               tuple(t.data_ptr() for t in tensors))
        if self._ctx is None or self._ctx_key != key:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = hip.GanContext(self.dims(), self.folded_state_dict(), device)
            self._ctx_key = key
        return self._ctx


class _Preprocess(nn.Module):

    def __init__(self, generator: Generator):
        super().__init__()
        self.generator = generator

    def forward(self, inputs: GInputs) -> GBlockDataBag:
        z, y = inputs
        return self.generator.preprocess(z, self.generator.embed(y))


class _Block(nn.Module):

    def __init__(self, block: nn.Module, index: int):
        super().__init__()
        self.block = block
        self.index = index

    def forward(self, inputs: GBlockDataBag) -> GBlockDataBag:
        return GBlockDataBag(self.block(inputs.h, inputs.ys[self.index]), inputs.ys)


class _Output(nn.Module):

    def __init__(self, generator: Generator):
        super().__init__()
        self.generator = generator

    def forward(self, inputs: GBlockDataBag) -> torch.Tensor:
        return torch.tanh(self.generator.output_layer(inputs.h))


class SeqBigGAN(nn.Sequential):
    """The generator as the `nn.Sequential` the reference dissects.  `generator_or_config`:
    a `Generator`, or a mapping of `Generator`'s arguments."""

    def __init__(self, generator_or_config: Union[Generator, Mapping[str, Any]]):
        generator = (generator_or_config if isinstance(generator_or_config, Generator) else
                     Generator(**dict(generator_or_config)))
        modules: List[Tuple[str, nn.Module]] = [('preprocess', _Preprocess(generator))]
        for index, blocks in enumerate(generator.blocks):
            for block in blocks:
                key = 'layer' if isinstance(block, GBlock) else 'attn'
                modules.append((key + str(index), _Block(block, index)))
        modules.append(('output', _Output(generator)))
        super().__init__(collections.OrderedDict(modules))

    @property
    def generator(self) -> Generator:
        return self.preprocess.generator

    @property
    def layers(self) -> Tuple[str, ...]:
        return self.generator.layers

    def forward_eager(self, inputs: GInputs) -> torch.Tensor:
        return nn.Sequential.forward(self, inputs)

    def native_refusal(self, inputs: GInputs):
        return self.generator.native_refusal(*inputs, roots=(self,))

    def runs_natively(self, inputs: GInputs) -> bool:
        return self.native_refusal(inputs) is None

    def forward(self, inputs: GInputs) -> torch.Tensor:
        if not self.runs_natively(inputs):
            return self.forward_eager(inputs)
        return self.generator._native(inputs.z, inputs.y, embedded=False, want_images=True)[1]

    def generate(self, inputs: GInputs, layer: Optional[str] = None, images: bool = True):
        """(the GBlockDataBag that child `layer` returns, or None; the images, or None).
        Natively one walk, which stops after `layer` when no images are wanted; otherwise
        `forward_eager` under `no_grad` with a forward hook (as far as needed)."""
        if not isinstance(inputs, GInputs):
            inputs = GInputs(*inputs)
        if layer is not None and layer not in self.layers:
            raise KeyError(f'layer not found: {layer}')
        if layer is None and not images:
            raise ValueError('generate: neither a layer nor the images are asked for')
        gen = self.generator
        if self.runs_natively(inputs):
            taps = () if layer is None else (self.layers.index(layer),)
            outs, pictures = gen._native(inputs.z, inputs.y, embedded=False, taps=taps,
                                         want_images=images)
            bag = None
            if layer is not None:
                y = gen.embed(inputs.y)
                ys = ([torch.cat([y, item], 1)
                       for item in torch.split(inputs.z, gen.z_chunk_size, 1)[1:]]
                      if gen.hier else [y] * len(gen.blocks))
                bag = GBlockDataBag(outs[taps[0]], ys)
            return bag, pictures
        with torch.no_grad():
            data: Any = inputs
            bag = None
            for name, child in self.named_children():
                data = child(data)
                if name == layer:
                    bag = data
                    if not images:
                        return bag, None
            return bag, data


def biggan(resolution: int = 256, **kwargs: Any) -> Generator:
    """The generator of the released BigGAN at 128, 256 or 512 pixels (ch 96, shared_dim 128,
    hierarchical z of 120 / 140 / 128 columns, attention at 64 / 128 / 64, eps 1e-4 in batch
    norm and spectral norm), without weights: load a pretorched checkpoint into it."""
    if resolution not in (128, 256, 512):
        raise ValueError(f'no released BigGAN at resolution {resolution}')
    config = dict(G_ch=96, dim_z={128: 120, 256: 140, 512: 128}[resolution],
                  resolution=resolution, G_attn={128: '64', 256: '128', 512: '64'}[resolution],
                  n_classes=1000, shared_dim=128, hier=True, BN_eps=1e-4, SN_eps=1e-4,
                  G_param='SN')
    return Generator(**{**config, **kwargs})


def infer_config(state_dict: Mapping[str, torch.Tensor]) -> Dict[str, Any]:
    """`Generator`'s structural arguments from a pretorched BigGAN state dict (BN_eps is not
    stored in a state dict and stays the caller's).  G_ch comes from the first block's input
    channels and bottom_width from the rows of `linear` (G_ch * multiplier * bottom_width^2)."""
    try:
        n_classes, shared_dim = state_dict['shared.weight'].shape
        rows, z_in = state_dict['linear.weight'].shape
        cond = state_dict['blocks.0.0.bn1.gain.weight'].shape[1]
        first = state_dict['blocks.0.0.conv1.weight'].shape[1]
    except KeyError as error:
        raise ValueError(f'not a BigGAN generator state dict: no {error}') from error
    blocks = len({k.split('.')[1] for k in state_dict if k.startswith('blocks.')})
    resolution = {len(v[0]): k for k, v in ARCH.items()}.get(blocks)
    if resolution is None:
        raise ValueError(f'{blocks} blocks match no BigGAN architecture')
    ch = first // ARCH[resolution][0][0]
    bottom_width = math.isqrt(rows // first)
    if ch * ARCH[resolution][0][0] != first or first * bottom_width**2 != rows:
        raise ValueError(f'linear has {rows} rows and the first block {first} input channels: '
                         f'no G_ch and bottom_width give both at resolution {resolution}')
    hier = cond > shared_dim
    attn = [8 << int(k.split('.')[1]) for k in state_dict if k.endswith('.1.gamma')]
    return dict(G_ch=ch, dim_z=z_in * (blocks + 1) if hier else z_in, bottom_width=bottom_width,
                resolution=resolution, G_attn='_'.join(map(str, attn)) or '0',
                n_classes=n_classes, shared_dim=shared_dim, hier=hier,
                G_param='SN' if 'linear.u0' in state_dict else 'none')


def from_state_dict(state_dict: Mapping[str, torch.Tensor], **kwargs: Any) -> Generator:
    """The generator a pretorched state dict belongs to, with the weights loaded (strict), in
    eval mode.  Pass `BN_eps` (1e-4 in the released 256 x 256 models) and anything else that
    a state dict does not tell."""
    model = Generator(**{**infer_config(state_dict), 'skip_init': True, **kwargs})
    model.load_state_dict(state_dict, strict=True)
    return model.eval()
