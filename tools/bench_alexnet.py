"""AlexNet on the HIP trunk: the Linear kernel of the head, classification and the
unit-ablation sweep, at torchvision's sizes (width 64, hidden 4096, 1000 classes, 224 x 224).

  (a) `hip.linear` (fp32 MFMA, packed weights) on fc6 / fc7 / linear8 at M = 1, 8, 64, 256 rows
      against `hip.linear_rowwise` (the ResNet head's kernel: one wavefront per output and
      row) on the same operands, the two alternating inside every sample.  Beside them two
      floors computed from the shapes: the packed weight's bytes over the copy bandwidth this
      run measures itself (a device-to-device copy of 1 GiB), and 2 M K N over the fp32-MFMA
      peak (157.3 TFLOP/s).  Every launch reads another copy of the weight, enough copies to
      exceed the 256 MiB last-level cache, so the weights come from HBM as they do in a
      forward pass.  Times are device events around `--launches` launches.
  (b) images per second of `AlexNetClassifier.forward` on 64 images, and
      `ImageClassifier.unit_scores` over all 64 + 192 + 384 + 256 + 256 = 1152 units against
      the one-unit-at-a-time loop (the two must give the same numbers), beside the
      multiply-add count of DESIGN 4.23 (0.36 of 1152 full passes).

    python tools/bench_alexnet.py [--steps 7] [--out profiles/alexnet_classify.txt]

Prints the device clocks read before the run and JSON lines; `--out` appends the same text to
a file.  A report, not an assertion: no time is fixed in advance.
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

import torch
from torch.utils import data

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd')]

from milan_amd import ablations, classifiers, hip  # noqa: E402

MFMA_F32_PEAK = 157.3e12
LAST_LEVEL_CACHE = 256 << 20
SHAPES = (('fc6', 4096, 9216), ('fc7', 4096, 4096), ('linear8', 1000, 4096))
ROWS = (1, 8, 64, 256)
COUNT_RATIO = 0.36   # multiply-adds of the sweep over 1152 full passes


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True,
                             timeout=30).stdout
    except (OSError, subprocess.TimeoutExpired):
        return 'rocm-smi not available'
    lines = [l.split(':', 1)[-1].strip() for l in out.splitlines()
             if 'GPU[0]' in l and ('sclk' in l or 'mclk' in l)]
    return '; '.join(lines) or 'no clock lines'


def device_ms(fn, launches):
    """Milliseconds per launch of `fn(i)`, i = 0 .. launches-1, by device events."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for i in range(launches):
        fn(i)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def wall(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - start, out


def spread(seconds, factor):
    """median / min / max of samples in seconds, in the unit `factor` converts to."""
    return dict(median=round(statistics.median(seconds) * factor, 2),
                min=round(min(seconds) * factor, 2), max=round(max(seconds) * factor, 2))


def copy_bandwidth(steps):
    src = torch.empty(1 << 28, dtype=torch.float32, device='cuda').normal_()
    dst = torch.empty_like(src)
    samples = [device_ms(lambda i: dst.copy_(src), 4) for _ in range(steps + 2)][2:]
    nbytes = 2 * src.numel() * 4   # read + write
    return nbytes / (statistics.median(samples) * 1e-3), [nbytes / (s * 1e-3) for s in samples]


def bench_linear(args, lines, bandwidth):
    g = torch.Generator().manual_seed(0)
    for name, n_out, n_in in SHAPES:
        weight = (torch.randn(n_out, n_in, generator=g) * n_in**-0.5).cuda()
        bias = (0.05 * torch.randn(n_out, generator=g)).cuda()
        first = hip.linear_pack(weight)
        packed_bytes = first[0].numel() * 4
        copies = LAST_LEVEL_CACHE * 2 // packed_bytes + 2
        packs = [first] + [(first[0].clone(), n_out, n_in) for _ in range(copies - 1)]
        raws = [weight] + [weight.clone() for _ in range(copies - 1)]
        for rows in ROWS:
            x = torch.randn(rows, n_in, generator=g).clamp_(min=0).cuda()
            new = lambda i: hip.linear(x, packs[i % copies], bias, relu=True)   # noqa: E731
            old = lambda i: hip.linear_rowwise(x, raws[i % copies], bias)        # noqa: E731
            want = torch.relu(x.double() @ weight.double().t() + bias.double())
            err = float((new(0).double() - want).abs().max() / want.abs().max())
            for fn in (new, old):   # warm-up: code objects, every copy touched once
                device_ms(fn, copies)
            t_new, t_old = [], []
            for _ in range(args.steps):
                t_new.append(device_ms(new, args.launches) * 1e-3)
                t_old.append(device_ms(old, args.launches) * 1e-3)
            stream_floor = packed_bytes / bandwidth
            mfma_floor = 2.0 * rows * n_in * n_out / MFMA_F32_PEAK
            med_new, med_old = statistics.median(t_new), statistics.median(t_old)
            lines.append(json.dumps(dict(
                layer=name, shape=[rows, n_in, n_out], packed_MB=round(packed_bytes / 1e6, 1),
                weight_copies_rotated=copies, launches_per_sample=args.launches,
                samples=args.steps,
                linear_mfma_us=spread(t_new, 1e6), linear_rowwise_us=spread(t_old, 1e6),
                rowwise_over_mfma=round(med_old / med_new, 2),
                mfma_wins_beyond_spread=min(t_old) > max(t_new),
                rowwise_wins_beyond_spread=min(t_new) > max(t_old),
                weight_stream_floor_us=round(stream_floor * 1e6, 2),
                mfma_peak_floor_us=round(mfma_floor * 1e6, 2),
                floor_over_time=round(max(stream_floor, mfma_floor) / med_new, 3),
                bound_by='weight stream' if stream_floor >= mfma_floor else 'fp32 MFMA',
                achieved_TFLOPs=round(2.0 * rows * n_in * n_out / med_new / 1e12, 2),
                achieved_weight_GBs=round(packed_bytes / med_new / 1e9, 1),
                error_over_max_want=float(f'{err:.3g}'))))
        del packs, raws


def bench_classify(args, lines):
    g = torch.Generator().manual_seed(1)
    model = classifiers.AlexNetClassifier(precision=args.precision)
    with torch.no_grad():   # activations of order one through the depth
        for module in model.modules():
            if isinstance(module, (torch.nn.Conv2d, torch.nn.Linear)):
                fan_in = module.weight[0].numel()
                module.weight.copy_(torch.randn(module.weight.shape, generator=g) *
                                    (2.0 / fan_in)**0.5)
                module.bias.copy_(0.05 * torch.randn(module.bias.shape, generator=g))
    model.eval().to('cuda')
    images = torch.randn(args.images, 3, 224, 224, generator=g).cuda()
    with torch.no_grad():
        targets = model(images).argmax(dim=-1)
        times = [wall(lambda: model(images))[0]
                 for _ in range(args.warmup + args.steps)][args.warmup:]
    dataset = data.TensorDataset(images, targets)
    classifier = ablations.ImageClassifier(model)
    units = [(layer, u) for layer, c in zip(model.layers, (64, 192, 384, 256, 256))
             for u in range(c)]
    kwargs = dict(batch_size=args.images, device='cuda', display_progress_as=None)
    classifier.unit_scores(dataset, units[:2], **kwargs)   # warm-up
    t_sweep, swept = wall(lambda: classifier.unit_scores(dataset, units, **kwargs))
    t_loop, looped = wall(lambda: [classifier.accuracy(dataset, ablate=[u], **kwargs)
                                   for u in units])
    lines.append(json.dumps(dict(
        workload=f'AlexNetClassifier width 64, hidden 4096, 1000 classes, 224x224, '
                 f'{args.images} images, precision {args.precision}',
        classify_ms=spread(times, 1e3),
        classify_images_per_s=round(args.images / statistics.median(times), 1),
        saturation_fallbacks=model._context().saturation_fallbacks,
        unit_scores_s=round(t_sweep, 3), loop_s=round(t_loop, 3),
        sweep_over_loop=round(t_sweep / t_loop, 4), multiply_add_count_ratio=COUNT_RATIO,
        units=len(units), same_scores=swept == looped, distinct_scores=len(set(swept)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--precision', default='auto')
    ap.add_argument('--skip-sweep', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.require_device('cuda')   # (no GPU: an error, never a CPU timing)
    lines = [f'clocks: {clocks()}']
    bandwidth, samples = copy_bandwidth(args.steps)
    lines.append(json.dumps(dict(copy_1GiB_GBs=round(bandwidth / 1e9, 1),
                                 copy_min_max_GBs=[round(min(samples) / 1e9, 1),
                                                   round(max(samples) / 1e9, 1)])))
    bench_linear(args, lines, bandwidth)
    if not args.skip_sweep:
        bench_classify(args, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
