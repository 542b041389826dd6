"""Digests of what launch_gemm computes and launches, for a bit-for-bit comparison of two builds
of libmilan_hip, in the style of tools/seq_digests.py.  One line per case: the
first 16 hex digits of the sha256 of the result's bytes and, after it, the launches that
milan_profile_read_kernels counted per kernel family while the case ran.

    MILAN_LIB=<one build>     python tools/gemm_digests.py > a.txt
    MILAN_LIB=<another build> python tools/gemm_digests.py > b.txt
    diff a.txt b.txt

The knobs of the launch path are read once per process, so the cases run in fresh child
processes, one per knob setting (KNOBS), each under its own time limit; the parent stops at the
first child that fails.  Cases: hip.conv2d_nhwc over small shapes (at most 4 images of 14 x 14),
the two vocabulary widths as 1x1 convs of K = 512 (launch_gemm) and through hip.linear (the
AlexNet head's own kernel, which does not pass through launch_gemm: a control), one
Context.encode of a small trunk with the tail lists on, one Places-AlexNet classify at width 8.
The record: profiles/gemm_plan.txt.
"""
import hashlib
import os
import pathlib
import subprocess
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO), str(REPO / 'tests')]

from milan_amd import hip, synthetic  # noqa: E402

KNOBS = ({}, {'MILAN_PP': '0'}, {'MILAN_PP': '2'}, {'MILAN_PP128': '0'}, {'MILAN_TAP_INNER': '0'},
         {'MILAN_TAP_SKIP': '0'}, {'MILAN_PP_PERSIST': '1'}, {'MILAN_GROUP_LAUNCH': '0'})
CONV_PRECISIONS = ('f32', 'split_f16', 'split_f16_tap_major', 'split_f16_tap_linear')


def dg(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def counted(tag, run):
    """`run()` with the profiler on: its digest and the launches per family."""
    hip.profile_enable(True)
    try:
        digest = dg(run())
        families = hip.profile_read_kernels()
    finally:
        hip.profile_enable(False)
    print(tag, digest, ' '.join(f'{name}:{int(row["launches"])}'
                                for name, row in families.items() if row['launches']), flush=True)


def convs(dev, setting):
    g = torch.Generator().manual_seed(17)
    for cin in (32, 64):
        for n in (64, 128, 256, 264):
            for k, pad in ((1, 0), (3, 1), (5, 2)):
                for stride in (1, 2):
                    for images in (1, 4):
                        x = torch.randn(images, 14, 14, cin, generator=g).to(dev)
                        w = (torch.randn(n, cin, k, k, generator=g) / (cin * k * k)**0.5).to(dev)
                        b = torch.randn(n, generator=g).to(dev)
                        ho = (14 + 2 * pad - k) // stride + 1
                        res = torch.randn(images, ho, ho, n, generator=g).to(dev)
                        for precision in CONV_PRECISIONS:
                            for residual in (None, res):
                                tag = (f'{setting} conv n{n} cin{cin} {k}x{k} s{stride} i{images} '
                                       f'{precision} res{int(residual is not None)}')
                                counted(tag, lambda: hip.conv2d_nhwc(
                                    x, w, b, stride, pad, relu=True, residual=residual,
                                    precision=precision))


def vocabulary(dev, setting):
    g = torch.Generator().manual_seed(23)
    for n in (5004, 3904):
        for rows in (3, 300):
            x = torch.randn(rows, 512, generator=g).to(dev)
            w = (torch.randn(n, 512, generator=g) / 512**0.5).to(dev)
            b = torch.randn(n, generator=g).to(dev)
            for precision in ('f32', 'split_f16'):
                counted(f'{setting} conv1x1 n{n} k512 rows{rows} {precision}',
                        lambda: hip.conv2d_nhwc(x.view(rows, 1, 1, 512), w.view(n, 512, 1, 1), b,
                                                precision=precision))
            packed = hip.linear_pack(w)
            counted(f'{setting} linear n{n} k512 rows{rows}', lambda: hip.linear(x, packed, b))


def encode(dev, setting):
    """the widest trunk whose last stage reaches the row-list tiles, on few small images"""
    blocks = synthetic.RESNET_BLOCKS['resnet50']
    sd = synthetic.resnet_state_dict('resnet50', seed=3, width=64, prefix='encoder.encoder.model.')
    ctx = hip.Context(hip.make_dims(sd, 10, blocks=blocks), sd, dev)
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (5, 3, 96, 96), dtype=torch.uint8, generator=g)
    masks = torch.zeros(5, 1, 96, 96, dtype=torch.uint8)
    for i in range(1, 5):
        masks[i, 0, 10 * i:10 * i + 30, 5 * i:5 * i + 40] = 1
    for precision in ('f32', 'split_f16'):
        ctx.set_precision(precision)
        counted(f'{setting} encode resnet50 w64 {precision} lists', lambda: ctx.encode(images, masks))
        ctx.set_fusion(sparse_tail=True, tail_lists=False)
        counted(f'{setting} encode resnet50 w64 {precision} copies', lambda: ctx.encode(images, masks))
        ctx.set_fusion()
        print(f'{setting} encode status', ctx.status())
    ctx.close()


def places(dev, setting):
    import test_gpu_places as P
    for width in (8, 16):
        ctx = P.make_context(P.model_sd(width), lrn=True)
        images = P.pictures((227, 227), 2)
        for precision in P.PRECISIONS:
            ctx.set_precision(precision)
            counted(f'{setting} places w{width} {precision} classify', lambda: ctx.classify(images))
        ctx.close()


def child():
    dev = hip.require_device(torch.device('cuda:0'))
    setting = sys.argv[2]
    convs(dev, setting)
    vocabulary(dev, setting)
    encode(dev, setting)
    places(dev, setting)
    torch.cuda.synchronize()
    print(f'{setting} done', flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child()
    for knobs in KNOBS:
        setting = ','.join(f'{k}={v}' for k, v in knobs.items()) or 'default'
        run = subprocess.run(['timeout', '-k', '10', '240', sys.executable, __file__, '--child',
                              setting], env=dict(os.environ, **knobs))
        if run.returncode != 0:
            sys.exit(f'the child with {setting} ended with {run.returncode}')


if __name__ == '__main__':
    main()
