"""DINO's vision transformer restated with torch.nn.functional (facebookresearch/dino,
vision_transformer.py), independent of milan_amd.vits' modules.  Runs in the dtype of its
inputs: in float64 it is the oracle of tests/test_vit_host.py, tests/test_gpu_attention.py
and tests/test_gpu_vit.py; in float32 on the CPU it defines the error an fp32 implementation
is entitled to.

    x   = conv(images; patch_embed.proj, stride p)            -> (n, G*G, W), row-major (gy, gx)
    x   = cat(cls_token, x) + pos_embed                       -> (n, T, W)
    per block:  y = LN(x; norm1) ; qkv = y qkv.W^T + qkv.b
                x = x + attention(qkv) proj.W^T + proj.b
                y = LN(x; norm2) ; h = y fc1.W^T + fc1.b      <- the tap
                x = x + gelu_erf(h) fc2.W^T + fc2.b
    out = LN(x; norm)[:, 0]

Bound for a comparison against float64 (the rule of tests/test_gpu_clip.py with the suite's
fp32-GEMM class as the floor): max|got - want| <= max(4 x e32, FEATURE_CLASS x max|want|), e32
= the max error of the float32 run against the float64 run of that same case.
"""
import math

import torch
import torch.nn.functional as F

from featclass import FEATURE_CLASS

EPS = 1e-6


def make_dims(res, patch, width, heads, depth, hidden):
    return dict(res=res, patch=patch, width=width, heads=heads, depth=depth, hidden=hidden)


def tokens(dims):
    return (dims['res'] // dims['patch'])**2 + 1


def weights(dims, seed):
    """A seeded float64 state dict under DINO's names that leaves nothing at its init value:
    LayerNorm weights around 1 with spread, non-zero biases, pos_embed and cls_token of order
    1; the matrices are scaled 1 / sqrt(fan_in) so that activations stay of order 1."""
    g = torch.Generator().manual_seed(seed)
    W, H, p = dims['width'], dims['hidden'], dims['patch']

    def normal(*shape, std=1.):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * std

    def ln(prefix, sd):
        sd[prefix + '.weight'] = 1. + normal(W, std=.2)
        sd[prefix + '.bias'] = normal(W, std=.2)

    def linear(prefix, sd, n_out, n_in, gain=1.):
        sd[prefix + '.weight'] = normal(n_out, n_in, std=gain / math.sqrt(n_in))
        sd[prefix + '.bias'] = normal(n_out, std=.3)

    sd = {'cls_token': normal(1, 1, W), 'pos_embed': normal(1, tokens(dims), W)}
    sd['patch_embed.proj.weight'] = normal(W, 3, p, p, std=2. / math.sqrt(3 * p * p))
    sd['patch_embed.proj.bias'] = normal(W, std=.3)
    for i in range(dims['depth']):
        b = f'blocks.{i}.'
        ln(b + 'norm1', sd)
        linear(b + 'attn.qkv', sd, 3 * W, W, gain=1.5)
        linear(b + 'attn.proj', sd, W, W)
        ln(b + 'norm2', sd)
        linear(b + 'mlp.fc1', sd, H, W)
        linear(b + 'mlp.fc2', sd, W, H)
    ln('norm', sd)
    return sd


def images(dims, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, dims['res'], dims['res'], generator=g, dtype=torch.float64)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def attention(qkv, heads):
    """qkv (B, T, 3 W): q | k | v, heads contiguous inside each -> (B, T, W)."""
    B, T, W3 = qkv.shape
    W = W3 // 3
    hd = W // heads
    q, k, v = qkv.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    p = F.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, T, W)


def forward(sd, x, dims):
    """(taps: list of (n, T, hidden) per block, out: (n, W)) in the dtype of sd and x."""
    W, p = dims['width'], dims['patch']
    x = F.conv2d(x, sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'], stride=p)
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat((sd['cls_token'].expand(x.shape[0], -1, -1), x), dim=1) + sd['pos_embed']
    taps = []
    for i in range(dims['depth']):
        b = f'blocks.{i}.'
        y = F.layer_norm(x, (W,), sd[b + 'norm1.weight'], sd[b + 'norm1.bias'], EPS)
        qkv = F.linear(y, sd[b + 'attn.qkv.weight'], sd[b + 'attn.qkv.bias'])
        a = attention(qkv, dims['heads'])
        x = x + F.linear(a, sd[b + 'attn.proj.weight'], sd[b + 'attn.proj.bias'])
        y = F.layer_norm(x, (W,), sd[b + 'norm2.weight'], sd[b + 'norm2.bias'], EPS)
        h = F.linear(y, sd[b + 'mlp.fc1.weight'], sd[b + 'mlp.fc1.bias'])
        taps.append(h)
        x = x + F.linear(F.gelu(h), sd[b + 'mlp.fc2.weight'], sd[b + 'mlp.fc2.bias'])
    out = F.layer_norm(x, (W,), sd['norm.weight'], sd['norm.bias'], EPS)[:, 0]
    return taps, out


def bound(want64, ref32):
    """max(4 x e32, FEATURE_CLASS x max|want|) and e32 for one tensor."""
    e32 = float((ref32.double() - want64).abs().max())
    return max(4 * e32, FEATURE_CLASS * float(want64.abs().max())), e32


def check(what, got, want64, ref32):
    """Assert the bound; print and return the measured multiple of it."""
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f'{what}: non-finite values'
    limit, e32 = bound(want64, ref32)
    err = float((got - want64).abs().max())
    print(f'VIT {what}: max|err| {err:.3g}, e32 {e32:.3g}, scale '
          f'{float(want64.abs().max()):.3g}, {err / limit:.3f} x bound')
    assert err <= limit, f'{what}: max|err| {err:g} > bound {limit:g} (e32 {e32:g})'
    return err / limit
