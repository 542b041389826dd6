"""Activation taps on the HIP trunk: resnet18 at torchvision's width (64), 224 x 224 images,
seeded random weights, images already on the device.

Per level (conv1, layer1..layer4):
  (a) the time of `ResNetClassifier.activations([L])` and of `classify` on the same images:
      the walk stops at the level, so by multiply-adds the ratio should be DESIGN 4.20's
      prefix fraction;
  (b) the time of the layout kernel alone (`tap_nchw_kernel`, read from torch's profiler:
      the device-side duration of the kernel, not a difference of wall times) and its
      effective bandwidth (bytes read + bytes written) / time.  The yardstick is the HBM
      rate tools/bench_exemplars.py reports for its streaming kernels on the same machine.

    python tools/bench_activations.py [--images 64] [--steps 7] [--warmup 3]
                                      [--precision auto] [--out profiles/activations.txt]

Prints the device clocks read before the run and one JSON line per level; `--out` appends the
same text to a file.  A report, not an assertion: no time is fixed in advance.
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd')]

from milan_amd import classifiers, synthetic  # noqa: E402


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True,
                             timeout=30).stdout
    except (OSError, subprocess.TimeoutExpired):
        return 'rocm-smi not available'
    lines = [l.split(':', 1)[-1].strip() for l in out.splitlines()
             if 'GPU[0]' in l and ('sclk' in l or 'mclk' in l)]
    return '; '.join(lines) or 'no clock lines'


def wall(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - start, out


def median_ms(fn, warmup, steps):
    times = [wall(fn)[0] for _ in range(warmup + steps)][warmup:]
    return 1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times)


def kernel_us(fn, name, warmup, steps):
    """Median device-side duration of the kernels whose name holds `name`, in us."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    found = []
    for event in prof.events():
        if name in event.name:
            duration = getattr(event, 'device_time', None)
            if duration is None:
                duration = getattr(event, 'cuda_time', 0.0)
            found.append(float(duration))
    return (statistics.median(found), len(found)) if found else (None, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--precision', default='auto')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'clocks: {clocks()}']
    g = torch.Generator().manual_seed(0)
    images = torch.randn(args.images, 3, 224, 224, generator=g).cuda()
    sd = synthetic.resnet_state_dict('resnet18', seed=5, width=64, with_fc=False)
    sd['fc.weight'] = torch.randn(10, 512, generator=g) * 512**-0.5
    sd['fc.bias'] = 0.05 * torch.randn(10, generator=g)
    model = classifiers.ResNetClassifier('resnet18', num_classes=10, precision=args.precision)
    model.load_state_dict(sd, strict=True)
    model.eval().to('cuda')
    with torch.no_grad():
        t_cls = median_ms(lambda: model(images), args.warmup, args.steps)
        lines.append(json.dumps(dict(
            workload=f'resnet18 width 64, 224x224, {args.images} images, precision '
                     f'{args.precision}, median of {args.steps} after {args.warmup} warm-up',
            classify_ms=round(t_cls[0], 3), classify_min_max_ms=[round(t_cls[1], 3),
                                                                round(t_cls[2], 3)])))
        for layer in model.layers:
            run = lambda: model.activations(images, [layer])  # noqa: E731
            t_act = median_ms(run, args.warmup, args.steps)
            shape = tuple(run()[layer].shape)
            moved = 2 * 4 * shape[0] * shape[1] * shape[2] * shape[3]
            us, launches = kernel_us(run, 'tap_nchw_kernel', 1, args.steps)
            lines.append(json.dumps(dict(
                layer=layer, shape=list(shape),
                activations_ms=round(t_act[0], 3),
                activations_min_max_ms=[round(t_act[1], 3), round(t_act[2], 3)],
                activations_over_classify=round(t_act[0] / t_cls[0], 4),
                layout_kernel_us=None if us is None else round(us, 2),
                layout_kernel_launches_seen=launches,
                layout_bytes=moved,
                layout_GBs=None if not us else round(moved / us / 1e3, 1))))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
