#!/usr/bin/env python3
"""Times of the Places365 AlexNet on the HIP trunk, in the style of
tools/bench_activations.py.

    python tools/bench_places.py [--images 64] [--steps 7] [--warmup 3] [--out profiles/places.txt]
    MILAN_GROUP_LAUNCH=0 python tools/bench_places.py ...     # the per-group baseline

Full width (96 / 256 / 384 / 384 / 256 channels, 4096 hidden, 365 classes), 227 x 227,
precision 'auto', seeded weights, images resident on the device; median (min, max) of `--steps`
wall times after `--warmup` calls, clocks read before the run.  One JSON line each for

  - `classify`, and `activations` at conv2, conv4 and conv5 (the walk stops at the level);
  - the eager torch forward of the same module on the same device, in fp32;
  - the device time of the GEMM kernels of one classify call (torch's profiler), which is what
    the grouped launch changes: run the tool once as it is and once with MILAN_GROUP_LAUNCH=0
    (the knob is read once per process) and compare the two `gemm_kernels` lines;
  - the LRN kernel alone on pool1's tensor (images x 27 x 27 pixels x 96 channels), fp32 and
    split: effective GB/s = bytes read once + bytes written once / device time.
"""
import argparse
import json
import os
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO / 'tools')]

from bench_activations import clocks, kernel_us, median_ms  # noqa: E402
from milan_amd import classifiers, hip, synthetic  # noqa: E402


def gemm_device_us(fn, warmup, steps):
    """Sum per call of the device time of the implicit-GEMM kernels, and their count per call."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    total, count = 0.0, 0
    for event in prof.events():
        if 'igemm' in event.name:
            duration = getattr(event, 'device_time', None)
            if duration is None:
                duration = getattr(event, 'cuda_time', 0.0)
            total += float(duration)
            count += 1
    return total / steps, count / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    form = 'per-group launches' if os.environ.get('MILAN_GROUP_LAUNCH') == '0' else 'grouped launch'
    lines = [f'clocks: {clocks()}', f'form: {form}']

    def record(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    model = classifiers.PlacesAlexNetClassifier(precision='auto')
    model.load_state_dict(synthetic.places_alexnet_state_dict(seed=3), strict=True)
    model.eval().to('cuda')
    g = torch.Generator().manual_seed(4)
    images = torch.randn(args.images, 3, 227, 227, generator=g).cuda()
    with torch.no_grad():
        med, lo, hi = median_ms(lambda: model(images), args.warmup, args.steps)
        record(what='classify', form=form, images=args.images, ms=med, min_ms=lo, max_ms=hi,
               images_per_s=args.images / med * 1e3)
        for layer in ('conv2', 'conv4', 'conv5'):
            med, lo, hi = median_ms(lambda: model.activations(images, layer), args.warmup,
                                    args.steps)
            record(what=f'activations {layer}', form=form, ms=med, min_ms=lo, max_ms=hi)
        us, count = gemm_device_us(lambda: model(images), args.warmup, args.steps)
        record(what='gemm_kernels', form=form, device_us_per_call=us, launches_per_call=count)
        eager = classifiers.PlacesAlexNetClassifier(precision='f32')
        eager.load_state_dict(model.state_dict())
        eager.eval().to('cuda')
        med, lo, hi = median_ms(lambda: eager.forward_eager(images), args.warmup, args.steps)
        record(what='eager torch forward fp32', ms=med, min_ms=lo, max_ms=hi)
    pixels, channels = args.images * 27 * 27, 96
    x = torch.rand(pixels, channels, device='cuda')
    for split in (False, True):
        us, found = kernel_us(lambda: hip.lrn(x, 5, 1e-4, 0.75, split=split), 'lrn_kernel',
                              args.warmup, args.steps)
        record(what='lrn kernel', split=split, pixels=pixels, channels=channels, device_us=us,
               effective_gb_per_s=(2 * x.numel() * 4 / (us * 1e-6) / 1e9) if us else None)
    lines.append(f'clocks after: {clocks()}')
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
