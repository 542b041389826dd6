#!/usr/bin/env python3
"""Times of VGG-16 on the HIP trunk, in the form of tools/bench_places.py.

    python tools/bench_vgg.py [--images 64] [--steps 7] [--warmup 3] [--out profiles/vgg.txt]

Full width (64 .. 512 channels, 4096 hidden, 1000 classes), 224 x 224, precision 'auto', seeded
weights, images resident on the device.  The yardstick is the eager fp32 forward of the same
module on the same device in the same session: native and eager runs alternate, one wall time
each per step, every one ending in a synchronise; median (min, max) of `--steps` after
`--warmup`.  One JSON line each for `classify`, `activations` at each of the five levels (the
walk stops at the level; the eager side runs the whole forward with one hook) and `unit_scores`
over one level (the sweep; eager: one hooked forward per unit), with the eager / native ratio.

Per-kernel device time comes from a run of its own under the profiler,

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o vgg -- python tools/bench_vgg.py --profile-run
    python tools/bench_vgg.py --trace DIR/vgg_kernel_trace.csv [--out profiles/vgg.txt]

`--profile-run` only classifies four times; `--trace` reads the kernel trace, takes the last
classify call (from its vgg_first_kernel on) and
prints, per kernel, the device time and -- for the convs, in network order -- the achieved
TF-eq (2 x MACs / time), for vgg_first_kernel, maxpool2s2_kernel and vgg_tail_kernel the bytes
read once plus written once over the kernel time.
"""
import argparse
import csv
import json
import pathlib
import sys

import torch
from torch.utils import data

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO / 'tools')]

from bench_activations import clocks, wall  # noqa: E402
from milan_amd import ablations, classifiers, synthetic  # noqa: E402

import statistics  # noqa: E402

CONFIG, SIDE = 'vgg16', 224


def make_model(precision):
    model = classifiers.VGGClassifier(CONFIG, precision=precision)
    model.load_state_dict(synthetic.vgg_state_dict(CONFIG, seed=3), strict=True)
    return model.eval().to('cuda')


def alternate(native, eager, warmup, steps):
    """(native, eager) wall times in ms, the two taking turns; [(median, min, max)] x 2."""
    times = ([], [])
    for _ in range(warmup + steps):
        times[0].append(wall(native)[0])
        times[1].append(wall(eager)[0])
    out = []
    for series in times:
        kept = series[warmup:]
        out.append((1e3 * statistics.median(kept), 1e3 * min(kept), 1e3 * max(kept)))
    return out


def bench(args):
    lines = [f'clocks: {clocks()}']

    def record(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    model = make_model('auto')
    eager = make_model('f32')
    g = torch.Generator().manual_seed(4)
    images = torch.randn(args.images, 3, SIDE, SIDE, generator=g).cuda()

    def report(what, native_fn, eager_fn, **extra):
        (med, lo, hi), (emed, elo, ehi) = alternate(native_fn, eager_fn, args.warmup, args.steps)
        record(what=what, images=args.images, native_ms=med, native_min_ms=lo, native_max_ms=hi,
               eager_ms=emed, eager_min_ms=elo, eager_max_ms=ehi, eager_over_native=emed / med,
               native_images_per_s=args.images / med * 1e3, **extra)

    with torch.no_grad():
        assert model.runs_natively(images)
        report('classify', lambda: model(images), lambda: eager.forward_eager(images))
        ctx = model._native_context()
        record(what='split convs', trace={f'{b}.{j}': v for (b, j), v in ctx.vgg_trace().items()},
               saturation_fallbacks=ctx.saturation_fallbacks)
        modules = dict(eager.named_modules())
        for layer in model.layers:
            def eager_tap(layer=layer):
                # (nethook's retain: one forward hook, the whole forward)
                kept = []
                handle = modules[layer].register_forward_hook(
                    lambda module, inputs, output: kept.append(output.detach()))
                try:
                    eager.forward_eager(images)
                finally:
                    handle.remove()
                return kept[0]

            report(f'activations {layer}', lambda: model.activations(images, layer), eager_tap)
        # ImageClassifier.unit_scores over `--units` units of one level (block 3's last conv):
        # natively one classify_sweep per batch; the eager side is the loop it stands for, one
        # hooked forward per unit, on the same device-resident batch
        layer = model.layers[2]
        units = [(layer, u) for u in range(args.units)]
        targets = torch.zeros(args.images, dtype=torch.int64, device='cuda')
        dataset = data.TensorDataset(images, targets)
        scorer = ablations.ImageClassifier(model)

        def native_scores():
            return scorer.unit_scores(dataset, units, batch_size=args.images,
                                      display_progress_as=None)

        def eager_scores():
            out = []
            for pair in units:
                with ablations.ablated(eager, [pair]):   # (forward hooks: forward_eager sees them)
                    hits = eager.forward_eager(images).argmax(dim=1) == targets
                out.append(float(hits.sum()) / args.images)
            return out

        report(f'unit_scores {layer}', native_scores, eager_scores, units=len(units))
    lines.append(f'clocks after: {clocks()}')
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def profile_run(args):
    model = make_model('auto')
    g = torch.Generator().manual_seed(4)
    images = torch.randn(args.images, 3, SIDE, SIDE, generator=g).cuda()
    with torch.no_grad():
        for _ in range(4):
            model(images)
            torch.cuda.synchronize()


def read_trace(args):
    rows = []
    with open(args.trace, newline='') as f:
        for row in csv.DictReader(f):
            rows.append((int(row['Start_Timestamp']), int(row['End_Timestamp']),
                         row['Kernel_Name']))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if 'vgg_first_kernel' in r[2]]
    if not starts:
        raise SystemExit('no vgg_first_kernel in the trace')
    call = rows[starts[-1]:]
    n = args.images
    lines = [f'kernel trace: {pathlib.Path(args.trace).name}', f'images: {n}']
    blocks = synthetic.VGG_BLOCKS[CONFIG]
    ch = [m * 64 for m in synthetic.VGG_CHANNELS]
    convs, cin = [], 3
    for b, count in enumerate(blocks):
        for j in range(count):
            convs.append((f'conv{b + 1}_{j + 1}', SIDE >> b, cin, ch[b]))
            cin = ch[b]
    convs = convs[1:]   # (conv1_1 is vgg_first_kernel)
    pools = [(SIDE >> b, ch[b]) for b in range(4)]
    helpers = ('vgg_first', 'maxpool2s2', 'vgg_tail', 'linear_mfma', 'row_argmax',
               'channel_mask', 'tap_nchw')
    total = 0.0
    for start, end, name in call:
        us = (end - start) / 1e3
        total += us
        short = name.split('(')[0][-72:]
        entry = dict(kernel=short, device_us=round(us, 2))
        if 'vgg_first' in name:
            moved = n * SIDE * SIDE * (3 + 64) * 4
            entry.update(layer='conv1_1', bytes=moved, gb_per_s=round(moved / us / 1e3, 1))
        elif 'maxpool2s2' in name and pools:
            side, c = pools.pop(0)
            moved = n * side * side * c * 4 * 5 // 4
            entry.update(layer=f'pool {side}x{side}x{c}', bytes=moved,
                         gb_per_s=round(moved / us / 1e3, 1))
        elif 'vgg_tail' in name:
            moved = n * (14 * 14 + 49) * 512 * 4
            entry.update(layer='pool5 + avgpool', bytes=moved, gb_per_s=round(moved / us / 1e3, 1))
        elif not any(h in name for h in helpers) and convs:
            layer, side, ci, co = convs.pop(0)
            macs = n * side * side * ci * co * 9
            entry.update(layer=layer, gmac=round(macs / 1e9, 2),
                         tf_eq=round(2 * macs / us / 1e6, 1))
        lines.append(json.dumps(entry))
    lines.append(json.dumps(dict(what='one classify call, sum of kernel times', device_ms=total / 1e3)))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--units', type=int, default=16, help='units of the sweep line')
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--trace', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.trace is not None:
        read_trace(args)
    elif args.profile_run:
        profile_run(args)
    else:
        bench(args)


if __name__ == '__main__':
    main()
