"""BigGAN's generator (Brock et al. 2019, as ajbrock/BigGAN-PyTorch and pretorched build it)
restated with torch.nn.functional from the model's description, independent of
milan_amd.generators' modules, on a state dict under pretorched's names.

    y    = shared.weight[class]  or  soft labels @ shared.weight          (n, shared_dim)
    z    = chunks z_0 .. z_B when hierarchical; block i is conditioned on cat(y, z_{i+1})
    h    = linear(z_0) viewed (n, C, bw, bw)
    GBlock i:  t = up2(relu(ccbn1(h, y_i)));  t = conv2(relu(ccbn2(conv1(t), y_i)))
               h = t + conv_sc(up2(h))                                    <- tap layer{i}
    ccbn(x, y) = (x - stored_mean) / sqrt(stored_var + eps) * (1 + gain(y)) + bias(y)
    Attention after the block at the attention resolution (SAGAN's non-local block):
        theta = conv1x1(h), phi = maxpool2(conv1x1(h)), g = maxpool2(conv1x1(h))
        beta = softmax_j(theta_i . phi_j)   no scale factor
        h = gamma * conv1x1_o(sum_j beta_ij g_j) + h                      <- tap attn{i}
    images = tanh(conv3x3(relu(bn(h))))            (the output bn has eps 1e-5 of its own)
    Spectral norm, eval mode: every weight with a `u0` buffer is divided by the singular-value
    estimate of ONE power iteration from u0 (v = normalize(u0 W), u = normalize(v W^T),
    sv = v W^T u^T), W viewed (out, -1); u0 is not updated.

The attention alone, pixel-major as milan_sagan_attention takes it: theta (n, H W, dk),
phi_g (n, H W / 4, dk + dv) = phi | g.

Runs in the dtype of its inputs: in float64 it is the oracle of tests/test_biggan_host.py,
tests/test_gpu_sagan_attention.py, tests/test_gpu_biggan.py and
tests/test_gpu_biggan_shapes.py (SHAPE_CASES, at the end); in float32 on the CPU it
defines the error an fp32 implementation is entitled to.  The bound is vitref.check's:
max|got - want| <= max(4 x e32, FEATURE_CLASS x max|want|), e32 = the max error of the float32
run against the float64 run of that same case.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from featclass import FEATURE_CLASS


def widths(channels):
    """(dk, dv) of a block with `channels` channels."""
    return channels // 8, channels // 2


def attention(theta, phi_g):
    """theta (n, Tq, dk), phi_g (n, Tk, dk + dv) -> (n, Tq, dv)."""
    dk = theta.shape[2]
    phi, g = phi_g[..., :dk], phi_g[..., dk:]
    return F.softmax(theta @ phi.transpose(1, 2), dim=-1) @ g


def pool_nhwc(x, height, width):
    """2 x 2 max-pool of pixel-major rows: (n, H W, c) -> (n, H W / 4, c)."""
    n, _, c = x.shape
    x = x.reshape(n, height // 2, 2, width // 2, 2, c)
    return x.amax(dim=(2, 4)).reshape(n, height * width // 4, c)


def inputs(n, height, width, channels, seed):
    """Seeded float64 Gaussian theta and phi | g of n images."""
    g = torch.Generator().manual_seed(seed)
    dk, dv = widths(channels)
    theta = torch.randn(n, height * width, dk, generator=g, dtype=torch.float64)
    phi_g = torch.randn(n, height * width // 4, dk + dv, generator=g, dtype=torch.float64)
    return theta, phi_g


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
    print(f'BIGGAN {what}: max|err| {err:.3g}, e32 {e32:.3g}, scale '
          f'{float(want64.abs().max()):.3g}, {err / limit:.3f} x bound')
    assert err <= limit, f'{what}: max|err| {err:g} > bound {limit:g} (e32 {e32:g})'
    return err / limit


# ---- the generator -------------------------------------------------------------------------
# channel multipliers (in, out) of the GBlocks per output resolution; block i doubles the side,
# from bottom_width to 8, 16, ...: the table of the paper's appendix B as BigGAN-PyTorch has it
ARCH = {
    512: ((16, 16, 8, 8, 4, 2, 1), (16, 8, 8, 4, 2, 1, 1)),
    256: ((16, 16, 8, 8, 4, 2), (16, 8, 8, 4, 2, 1)),
    128: ((16, 16, 8, 4, 2), (16, 8, 4, 2, 1)),
    64: ((16, 16, 8, 4), (16, 8, 4, 2)),
    32: ((4, 4, 4), (4, 4, 4)),
}
OUT_BN_EPS = 1e-5


def make_dims(resolution, ch, attn, dim_z, shared_dim, n_classes, hier=True, bottom_width=4,
              bn_eps=1e-4, sn=True):
    """`attn`: the resolution whose block is followed by attention, or 0.  dim_z is rounded
    down to a multiple of the slot count when hierarchical, as the model does."""
    blocks = len(ARCH[resolution][0])
    chunk = dim_z // (blocks + 1) if hier else 0
    return dict(resolution=resolution, ch=ch, attn=attn, dim_z=chunk * (blocks + 1) if hier
                else dim_z, chunk=chunk, shared_dim=shared_dim, n_classes=n_classes, hier=hier,
                bottom_width=bottom_width, bn_eps=bn_eps, sn=sn)


def blocks_of(dims):
    """[(in_channels, out_channels, has_attention)] per GBlock."""
    ins, outs = ARCH[dims['resolution']]
    return [(dims['ch'] * a, dims['ch'] * b, 8 << i == dims['attn'])
            for i, (a, b) in enumerate(zip(ins, outs))]


def layer_names(dims):
    names = []
    for i, (_, _, attn) in enumerate(blocks_of(dims)):
        names.append(f'layer{i}')
        if attn:
            names.append(f'attn{i}')
    return names


def weights(dims, seed):
    """A seeded float64 state dict under pretorched's names that leaves nothing at its init
    value: gamma nonzero, stored_mean / stored_var non-trivial, u0 random."""
    g = torch.Generator().manual_seed(seed)
    sd = collections.OrderedDict()

    def normal(*shape, std=1.):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * std

    def sn(prefix, out):
        if dims['sn']:
            sd[prefix + '.u0'] = normal(1, out)
            sd[prefix + '.sv0'] = torch.ones(1, dtype=torch.float64)

    def conv(prefix, cout, cin, k, bias=True, gain=3.):
        # (spectral norm brings the matrix to norm ~1: `gain` only matters without it)
        sd[prefix + '.weight'] = normal(cout, cin, k, k, std=gain / math.sqrt(cin * k * k))
        if bias:
            sd[prefix + '.bias'] = normal(cout, std=.2)
        sn(prefix, cout)

    def stats(prefix, c):
        sd[prefix + '.stored_mean'] = normal(c, std=.3)
        sd[prefix + '.stored_var'] = .5 + torch.rand(c, generator=g, dtype=torch.float64)

    def ccbn(prefix, c, cond):
        for part in ('gain', 'bias'):
            sd[f'{prefix}.{part}.weight'] = normal(c, cond, std=2. / math.sqrt(cond))
            sn(f'{prefix}.{part}', c)
        stats(prefix, c)

    bw, arch = dims['bottom_width'], blocks_of(dims)
    cond = dims['shared_dim'] + dims['chunk']
    z_in = dims['chunk'] if dims['hier'] else dims['dim_z']
    sd['shared.weight'] = normal(dims['n_classes'], dims['shared_dim'])
    sd['linear.weight'] = normal(arch[0][0] * bw * bw, z_in, std=3. / math.sqrt(z_in))
    sd['linear.bias'] = normal(arch[0][0] * bw * bw, std=.2)
    sn('linear', arch[0][0] * bw * bw)
    for i, (cin, cout, attn) in enumerate(arch):
        b = f'blocks.{i}.0.'
        conv(b + 'conv1', cout, cin, 3)
        conv(b + 'conv2', cout, cout, 3)
        conv(b + 'conv_sc', cout, cin, 1)
        ccbn(b + 'bn1', cin, cond)
        ccbn(b + 'bn2', cout, cond)
        if attn:
            a = f'blocks.{i}.1.'
            sd[a + 'gamma'] = torch.tensor(.7, dtype=torch.float64)
            conv(a + 'theta', cout // 8, cout, 1, bias=False, gain=4.)
            conv(a + 'phi', cout // 8, cout, 1, bias=False, gain=4.)
            conv(a + 'g', cout // 2, cout, 1, bias=False)
            conv(a + 'o', cout, cout // 2, 1, bias=False)
    last = arch[-1][1]
    sd['output_layer.0.gain'] = 1. + normal(last, std=.2)
    sd['output_layer.0.bias'] = normal(last, std=.2)
    stats('output_layer.0', last)
    conv('output_layer.2', 3, last, 3)
    return sd


def tap_shapes(dims):
    """[(channels, side)] per name of layer_names(dims): block i doubles bottom_width << i."""
    shapes = []
    for i, (_, cout, attn) in enumerate(blocks_of(dims)):
        shapes += [(cout, dims['bottom_width'] << (i + 1))] * (2 if attn else 1)
    return shapes


def image_side(dims):
    return dims['bottom_width'] << len(ARCH[dims['resolution']][0])


def latents(dims, n, seed):
    """Seeded (z (n, dim_z) float64, hard y (n,) int64, soft y (n, n_classes) float64)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, dims['dim_z'], generator=g, dtype=torch.float64)
    hard = torch.randint(0, dims['n_classes'], (n,), generator=g)
    soft = torch.softmax(torch.randn(n, dims['n_classes'], generator=g, dtype=torch.float64), 1)
    return z, hard, soft


def cast(sd, dtype):
    return collections.OrderedDict(
        (k, v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items())


def sn_weight(weight, u0, eps=1e-12):
    """The eval-mode spectrally normalised weight: weight / sv of one power iteration."""
    w = weight.reshape(weight.shape[0], -1)
    v = F.normalize(u0 @ w, eps=eps)
    u = F.normalize(v @ w.t(), eps=eps)
    sv = ((v @ w.t()) @ u.t()).squeeze()
    return weight / sv


def _w(sd, prefix):
    w = sd[prefix + '.weight']
    return sn_weight(w, sd[prefix + '.u0']) if prefix + '.u0' in sd else w


def _up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def _ccbn(sd, prefix, x, y, eps):
    gain = 1. + F.linear(y, _w(sd, prefix + '.gain'))
    bias = F.linear(y, _w(sd, prefix + '.bias'))
    mean, var = sd[prefix + '.stored_mean'], sd[prefix + '.stored_var']
    out = (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
    return out * gain[:, :, None, None] + bias[:, :, None, None]


def attention_block(sd, prefix, x):
    n, c, hh, ww = x.shape
    theta = F.conv2d(x, _w(sd, prefix + 'theta'))
    phi = F.max_pool2d(F.conv2d(x, _w(sd, prefix + 'phi')), 2)
    g = F.max_pool2d(F.conv2d(x, _w(sd, prefix + 'g')), 2)
    theta = theta.reshape(n, c // 8, hh * ww).transpose(1, 2)
    phi_g = torch.cat((phi.reshape(n, c // 8, -1), g.reshape(n, c // 2, -1)), 1).transpose(1, 2)
    o = attention(theta, phi_g).transpose(1, 2).reshape(n, c // 2, hh, ww)
    return sd[prefix + 'gamma'] * F.conv2d(o, _w(sd, prefix + 'o')) + x


def forward(sd, z, y, dims):
    """(taps: OrderedDict layer name -> (n, C, H, W), images (n, 3, R, R)) in the dtype of sd
    and z.  y: class indices (n,) or soft labels (n, n_classes)."""
    y = sd['shared.weight'][y] if y.dim() == 1 else y @ sd['shared.weight']
    arch = blocks_of(dims)
    if dims['hier']:
        zs = torch.split(z, dims['chunk'], 1)
        z, ys = zs[0], [torch.cat((y, item), 1) for item in zs[1:]]
    else:
        ys = [y] * len(arch)
    bw, eps = dims['bottom_width'], dims['bn_eps']
    h = F.linear(z, _w(sd, 'linear'), sd['linear.bias']).reshape(z.shape[0], -1, bw, bw)
    taps = collections.OrderedDict()
    for i, (_, _, attn) in enumerate(arch):
        b = f'blocks.{i}.0.'
        t = _up2(torch.relu(_ccbn(sd, b + 'bn1', h, ys[i], eps)))
        t = F.conv2d(t, _w(sd, b + 'conv1'), sd[b + 'conv1.bias'], padding=1)
        t = torch.relu(_ccbn(sd, b + 'bn2', t, ys[i], eps))
        t = F.conv2d(t, _w(sd, b + 'conv2'), sd[b + 'conv2.bias'], padding=1)
        h = t + F.conv2d(_up2(h), _w(sd, b + 'conv_sc'), sd[b + 'conv_sc.bias'])
        taps[f'layer{i}'] = h
        if attn:
            h = attention_block(sd, f'blocks.{i}.1.', h)
            taps[f'attn{i}'] = h
    o = 'output_layer.0.'
    h = (h - sd[o + 'stored_mean'][None, :, None, None]) / torch.sqrt(
        sd[o + 'stored_var'][None, :, None, None] + OUT_BN_EPS)
    h = torch.relu(h * sd[o + 'gain'][None, :, None, None] + sd[o + 'bias'][None, :, None, None])
    images = torch.tanh(F.conv2d(h, _w(sd, 'output_layer.2'), sd['output_layer.2.bias'],
                                 padding=1))
    return taps, images


# ---- the architectures, bottom widths and batches off the golden's path ----------------------
# name -> (dims, batch).  What each reaches in the native walk is listed in
# tests/test_gpu_biggan_shapes.py; tests/test_biggan_host.py runs the eager modules on some.
SHAPE_CASES = {
    'r128': (make_dims(128, 16, 64, 30, 12, 7), 3),
    'r256': (make_dims(256, 16, 128, 35, 9, 6), 1),
    'r256flat': (make_dims(256, 4, 32, 21, 9, 6, hier=False), 2),
    'r512': (make_dims(512, 8, 64, 24, 5, 3), 1),
    'bw3': (make_dims(32, 8, 16, 32, 16, 10, bottom_width=3), 5),
    'bw5': (make_dims(32, 8, 8, 32, 16, 10, bottom_width=5), 3),
    'bw1': (make_dims(64, 16, 32, 10, 5, 1, bottom_width=1), 7),
    'n80': (make_dims(32, 20, 0, 18, 7, 5, hier=False), 3),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(dims, float64 weights, (z, hard y, soft y)) of a SHAPE_CASES entry, seeded by its
    position in the table."""
    dims, batch = SHAPE_CASES[name]
    index = list(SHAPE_CASES).index(name)
    return dims, weights(dims, seed=700 + index), latents(dims, batch, seed=800 + index)


@functools.lru_cache(maxsize=None)
def shape_reference(name, soft=False):
    """(float64 (taps, images), float32 (taps, images)) of a SHAPE_CASES entry for hard or soft
    labels: computed once per process and left unchanged."""
    dims, sd, (z, hard, soft_y) = shape_case(name)
    with torch.no_grad():
        want = forward(sd, z, soft_y if soft else hard, dims)
        ref32 = forward(cast(sd, torch.float32), z.float(), soft_y.float() if soft else hard, dims)
    return want, ref32
