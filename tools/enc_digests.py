"""Digests of what the ResNet encoder pass computes and launches, for a bit-for-bit comparison of
two builds of libmilan_hip, in the style of tools/gemm_digests.py.  One line per
case: the first 16 hex digits of the sha256 of the result's bytes, the launches that
milan_profile_read_kernels counted per kernel family while the case ran, and the status word.

    MILAN_LIB=<one build>     python tools/enc_digests.py > a.txt
    MILAN_LIB=<another build> python tools/enc_digests.py > b.txt
    diff a.txt b.txt

The knobs of the pass are read once per process, so the cases run in fresh child processes, one
per knob setting (KNOBS), each under its own time limit; the parent stops at the first child
that fails.  The default child walks every axis -- four trunks (resnet50 at width 64 and 16,
resnet18 at width 16, resnet101 at width 64) in the three precisions and 'auto'; on the
width-64 resnet50 each fusion bit off alone, masks absent / uint8 / float / all-empty, float
images (one with a NaN pixel: the poison path), image sharing with duplicates, encode_spatial,
encoder_absmax, and the extents 96 x 96, 64 x 80, 33 x 47 and 8 x 8 -- the others the width-64
resnet50 alone, MILAN_ENC_SUB=3 on seven images.  A call the library refuses prints its error
instead of a digest.  The record: profiles/enc_plan.txt.
"""
import hashlib
import os
import pathlib
import subprocess
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO)]

from milan_amd import hip, synthetic  # noqa: E402

KNOBS = ({}, {'MILAN_ENC_SUB': '3'}, {'MILAN_STEM_U8': '0'}, {'MILAN_POOL_VEC': '0'},
         {'MILAN_PP': '0'})
PREFIX = 'encoder.encoder.model.'
FUSION_BITS = ('chain', 'wide', 'stem', 'conv3', 'skip_empty', 'bneck', 'sparse_tail', 'tail_lists')


def dg(t):
    if not torch.is_tensor(t):
        t = torch.tensor(float(t), dtype=torch.float64)
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def counted(ctx, tag, run):
    """`run()` with the profiler on: its digest, the launches per family, the status word."""
    hip.profile_enable(True)
    try:
        try:
            digest = dg(run())
        except Exception as error:  # a refusal is a line too: both builds have to refuse alike
            digest = f'{type(error).__name__}: {str(error)[:80]}'
        families = hip.profile_read_kernels()
    finally:
        hip.profile_enable(False)
    print(tag, digest, ' '.join(f'{name}:{int(row["launches"])}'
                                for name, row in families.items() if row['launches']),
          'status', ctx.status(), flush=True)


def make(arch, width, dev):
    sd = synthetic.resnet_state_dict(arch, seed=3, width=width, prefix=PREFIX)
    return hip.Context(hip.make_dims(sd, 10, blocks=synthetic.RESNET_BLOCKS[arch]), sd, dev)


def batch(n, h, w, seed=5):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=g)
    masks = torch.zeros(n, 1, h, w, dtype=torch.uint8)
    for i in range(1, n):   # (image 0 has an empty mask)
        masks[i, 0, (h * i) // (2 * n):(h * i) // (2 * n) + max(1, h // 3),
              (w * i) // (3 * n):(w * i) // (3 * n) + max(1, w // 2)] = 1
    return images, masks


def precisions(ctx, tag, run):
    for precision in ('f32', 'split_f16', 'f16', 'auto'):
        saved = ctx.on_saturation
        try:
            ctx.set_precision('split_f16' if precision == 'auto' else precision)
            if precision == 'auto':
                ctx.on_saturation = 'f32'
        except Exception as error:
            print(tag, precision, f'{type(error).__name__}: {str(error)[:80]}', flush=True)
            continue
        counted(ctx, f'{tag} {precision}', lambda: run(precision == 'auto'))
        ctx.on_saturation = saved
    ctx.set_precision('split_f16')


def axes(ctx, setting):
    """every axis of the pass on the width-64 resnet50, split_f16"""
    images, masks = batch(5, 96, 96)
    tag = f'{setting} resnet50 w64'
    for bit in FUSION_BITS:
        if bit == 'sparse_tail':
            ctx.set_fusion(sparse_tail=False, tail_lists=False)
        else:
            ctx.set_fusion(**{bit: False})
        counted(ctx, f'{tag} {bit}=0', lambda: ctx.encode(images, masks, check=False))
    ctx.set_fusion()
    floats = masks.float() * 0.75
    for name, m in (('none', None), ('u8', masks), ('float', floats), ('empty', masks * 0)):
        counted(ctx, f'{tag} masks={name}', lambda: ctx.encode(images, m, check=False))
    real = images.float() / 255
    counted(ctx, f'{tag} float images', lambda: ctx.encode(real, masks, check=False))
    poisoned = real.clone()
    poisoned[2, 1, 40, 50] = float('nan')   # data, not a fault: image 2 leaves as NaN
    counted(ctx, f'{tag} float images, one NaN pixel', lambda: ctx.encode(poisoned, masks, check=False))
    counted(ctx, f'{tag} spatial of them', lambda: ctx.encode_spatial(poisoned, masks, check=False))
    twice = torch.cat([images, images[1:3], images[:1]])
    masks8 = torch.cat([masks, masks[3:5], masks[1:2]])
    ctx.set_image_sharing(True)
    counted(ctx, f'{tag} sharing', lambda: ctx.encode(twice, masks8, check=False))
    counted(ctx, f'{tag} sharing, no masks', lambda: ctx.encode(twice, None, check=False))
    ctx.set_image_sharing(False)
    counted(ctx, f'{tag} sharing off', lambda: ctx.encode(twice, masks8, check=False))
    counted(ctx, f'{tag} spatial', lambda: ctx.encode_spatial(images, masks, check=False))
    counted(ctx, f'{tag} spatial, no masks', lambda: ctx.encode_spatial(images, None, check=False))
    counted(ctx, f'{tag} absmax', lambda: ctx.encoder_absmax(images))
    for h, w in ((96, 96), (64, 80), (33, 47), (8, 8)):
        im, mk = batch(5, h, w, seed=h + w)
        precisions(ctx, f'{tag} {h}x{w}', lambda auto: ctx.encode(im, mk, check=auto))


def child():
    dev = hip.require_device(torch.device('cuda:0'))
    setting = sys.argv[2]
    default = setting == 'default'
    trunks = (('resnet50', 64), ('resnet50', 16), ('resnet18', 16), ('resnet101', 64))
    n = 7 if 'MILAN_ENC_SUB' in setting else 5
    images, masks = batch(n, 96, 96)
    for arch, width in trunks if default else trunks[:1]:
        ctx = make(arch, width, dev)
        tag = f'{setting} {arch} w{width}'
        precisions(ctx, f'{tag} lists', lambda auto: ctx.encode(images, masks, check=auto))
        ctx.set_fusion(tail_lists=False)
        precisions(ctx, f'{tag} copies', lambda auto: ctx.encode(images, masks, check=auto))
        ctx.set_fusion()
        if (arch, width) == trunks[0]:
            if default:
                axes(ctx, setting)
            else:
                counted(ctx, f'{tag} spatial', lambda: ctx.encode_spatial(images, masks, check=False))
                counted(ctx, f'{tag} no masks', lambda: ctx.encode(images, None, check=False))
        ctx.close()
    torch.cuda.synchronize()
    print(f'{setting} done', flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child()
    for knobs in KNOBS:
        setting = ','.join(f'{k}={v}' for k, v in knobs.items()) or 'default'
        run = subprocess.run(['timeout', '-k', '10', '300', sys.executable, __file__, '--child',
                              setting], env=dict(os.environ, **knobs))
        if run.returncode != 0:
            sys.exit(f'the child with {setting} ended with {run.returncode}')


if __name__ == '__main__':
    main()
