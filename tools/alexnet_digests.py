"""Digests of what the two AlexNets compute on the HIP trunk, for a bit-for-bit comparison of
two builds of libmilan_hip, in the style of tools/tower_digests.py.  One line per
case: the first 16 hex digits of the sha256 of each result tensor's bytes, the status word, and
the workspace byte counts (milan_classify_workspace_bytes, milan_activations_workspace_bytes;
milan_workspace_bytes for the encoder).  Fixed seeds, small shapes.

    MILAN_LIB=<one build>     python tools/alexnet_digests.py > a.txt
    MILAN_LIB=<another build> python tools/alexnet_digests.py > b.txt
    diff a.txt b.txt

One library per process.  The torchvision AlexNet's classifier side runs a second time in a
child process with MILAN_ENC_SUB=3 (the knob is read once per process): 7 images in passes of
3 + 3 + 1.  The record of the refactor that gave the two nets one trunk is
profiles/alexnet_unify.txt.
"""
import hashlib
import os
import pathlib
import subprocess
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO), str(REPO / 'tests')]

import alexref  # noqa: E402
import placesref  # noqa: E402
import test_gpu_alexnet as A  # noqa: E402
import test_gpu_places as P  # noqa: E402
from milan_amd import hip, synthetic  # noqa: E402

PRECISIONS = ('f32', 'split_f16')
SUB = os.environ.get('MILAN_ENC_SUB', 'unset')


def dg(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def sweep_units(ch):
    return [(level, u) for level in range(5) for u in sorted({0, 5, ch[level] - 1})]


def workspace(tag, ctx, h, w):
    for n in (1, 7, 200):
        for sweep in (0, 1, 15):
            print(tag, f'workspace n={n} sweep={sweep}',
                  int(ctx.lib.milan_classify_workspace_bytes(ctx._h, n, h, w, sweep)),
                  int(ctx.lib.milan_activations_workspace_bytes(ctx._h, n, h, w)))


def classifier_line(tag, ctx, images, base, ch, classes):
    """logits, predictions, the five taps, taps [3, 1], a sweep with targets, the status word."""
    ctx.set_ablation(base)
    logits = ctx.classify(images)
    preds = ctx.classify(images, return_logits=False)
    taps = ctx.activations(images, range(5))
    two = ctx.activations(images, [3, 1])
    targets = torch.arange(len(images)) % classes
    swept, correct = ctx.classify_sweep(images, sweep_units(ch), targets)
    print(tag, 'logits', dg(logits), 'preds', dg(preds),
          ' '.join(f'L{l} {dg(taps[l])}' for l in range(5)), 'L3,1', dg(two[3]), dg(two[1]),
          'sweep', dg(swept), 'correct', dg(correct), 'status', ctx.status())
    ctx.set_ablation([])


def alexnet_classifier():
    for width in (8, 32):
        ctx = A.make_context(alexref.make_state_dict(61, width, 72, 10))
        for geo in ((63, 63), (95, 127)):
            tag = f'alexnet.w{width}.{geo[0]}x{geo[1]} sub={SUB}'
            images = alexref.make_images(61, 7, geo)
            for precision in PRECISIONS:
                ctx.set_precision(precision)
                classifier_line(f'{tag} {precision}', ctx, images, [(0, 1), (2, 5)],
                                alexref.channels(width), 10)
            workspace(tag, ctx, *geo)
        ctx.close()


def alexnet_encoder():
    g = torch.Generator().manual_seed(9)
    images = torch.randint(256, (6, 3, 96, 96), generator=g, dtype=torch.uint8)
    masks = (torch.rand(6, 1, 96, 96, generator=g) > 0.6).to(torch.uint8)
    for width in (8, 32):
        ctx = A.make_context(alexref.make_state_dict(61, width, 72, 10), head=False)
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            features = ctx.encode(images, masks)
            print(f'alexnet.w{width} {precision} encode', tuple(features.shape), dg(features),
                  'status', ctx.status())
        print(f'alexnet.w{width} encoder workspace',
              *[int(ctx.lib.milan_workspace_bytes(ctx._h, n, 1, 96, 1, 1)) for n in (1, 7)])
        ctx.close()


def places():
    base = [(1, 3), (3, 5)]
    for width, lrn, groups, n in ((8, False, True, 5), (8, True, True, 5), (16, False, True, 5),
                                  (16, True, True, 5), (64, False, True, 2), (8, False, False, 5)):
        ctx = P.make_context(P.model_sd(width, groups), lrn=lrn)
        ch = placesref.channels(width)
        tag = f'places.w{width}.lrn{int(lrn)}.groups{int(groups)}'
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            classifier_line(f'{tag}.227x227 {precision}', ctx, P.pictures((227, 227), n), base,
                            ch, P.CLASSES)
            ctx.set_ablation(base)
            for geo in ((99, 131), (35, 38)):
                taps = ctx.activations(P.pictures(geo, n), range(5))
                print(f'{tag}.{geo[0]}x{geo[1]} {precision}',
                      ' '.join(f'L{l} {dg(taps[l])}' for l in range(5)), 'status', ctx.status())
            ctx.set_ablation([])
        workspace(f'{tag}.227x227', ctx, 227, 227)
        ctx.close()
    bare = P.make_context(P.model_sd(8), head=False)
    for precision in PRECISIONS:
        bare.set_precision(precision)
        print(f'places.w8.headless.227x227 {precision} L4',
              dg(bare.activations(P.pictures((227, 227)), [4])[4]), 'status', bare.status())
    workspace('places.w8.headless.227x227', bare, 227, 227)
    bare.close()


def resnet_workspace():
    sd = {A.PREFIX + k: v
          for k, v in synthetic.resnet_state_dict('resnet18', seed=1, width=8).items()}
    ctx = hip.Context(hip.make_dims(sd, 1, blocks=(2, 2, 2, 2)), sd, torch.device('cuda'))
    workspace('resnet18.w8.33x47', ctx, 33, 47)
    ctx.close()


def main():
    hip.require_device(torch.device('cuda:0'))
    alexnet_classifier()
    if '--child' in sys.argv:
        torch.cuda.synchronize()
        return
    alexnet_encoder()
    places()
    resnet_workspace()
    torch.cuda.synchronize()
    print('done sub=' + SUB, flush=True)
    child = subprocess.run(['timeout', '-k', '10', '300', sys.executable, __file__, '--child'],
                           env=dict(os.environ, MILAN_ENC_SUB='3'))
    if child.returncode != 0:
        sys.exit(f'the MILAN_ENC_SUB=3 child ended with {child.returncode}')
    print('done sub=3')


if __name__ == '__main__':
    main()
