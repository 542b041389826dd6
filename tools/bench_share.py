"""What image sharing costs and saves on the benchmark's chunk.

The benchmark's model and chunk (ResNet-101 at width 64, 640 neurons x 15 exemplars of
224 x 224, beam 50 + rerank, split-f16) with a given share of the chunk's images replaced by
copies of other images of the SAME chunk; the masks stay distinct.  Sharing off and on
alternate in one process on one device (off, on, off, on, ...), and the two halves of the
`off` legs are compared with each other for that device's noise.  Per duplicate rate:

  * ms per pass of the encoder stages (HIP-event regions, milan_profile_read_stages);
  * the dedup kernels' own time: the `enc_input` region (mask pyramid + hash + classes +
    compaction + counters + input conversion) on minus off;
  * trunk_images / slots from the device-side counters;
  * neuron-descriptions / s, host clock around whole steps ending in a synchronise.

Nothing here is a pass / fail threshold, and none of it enters bench.py's `value`.  How often
real exemplar sets repeat an image inside a chunk is not measured: the rates are inputs.

    python tools/bench_share.py --out profiles/share_images.txt
"""
import argparse
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
for p in (REPO, REPO / 'neuron-descriptions_amd'):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

from milan_amd import hip, synthetic  # noqa: E402

ENC_STAGES = ('enc_input', 'enc_stem', 'enc_stem_tail', 'enc_layer1', 'enc_layer2',
              'enc_layer3', 'enc_layer4', 'enc_pool')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--neurons', type=int, default=640)
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--beam', type=int, default=50)
    ap.add_argument('--length', type=int, default=15)
    ap.add_argument('--vocab', type=int, default=5000)
    ap.add_argument('--rates', default='0,25,50', help='duplicate rates in percent')
    ap.add_argument('--rounds', type=int, default=4,
                    help='off/on pairs per rate (the off legs split in two for the noise)')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--precision', default='split_f16')
    ap.add_argument('--out', type=pathlib.Path, default=None)
    return ap.parse_args(argv)


def with_duplicates(images, rate, seed):
    """`rate` percent of the chunk's slots (chosen at random) become copies of other slots that
    keep their own image; returns the images and the number of distinct images left"""
    flat = images.reshape((-1,) + tuple(images.shape[2:])).clone()
    m = len(flat)
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(m, generator=g)
    n_dup = m * rate // 100
    dup, keep = perm[:n_dup], perm[n_dup:]
    if n_dup:
        src = keep[torch.randint(0, len(keep), (n_dup,), generator=g)]
        flat[dup.to(flat.device)] = flat[src.to(flat.device)]
    return flat.reshape(images.shape), m - n_dup


def timed_leg(ctx, images, masks, args, share):
    """one describe step with profiling on -> (seconds, stage table)"""
    ctx.set_image_sharing(share)
    torch.cuda.synchronize()
    hip.profile_enable(True)
    t0 = time.perf_counter()
    ctx.describe(images, masks, hip.RERANK, args.length, args.beam, False, 0.2,
                 group_size=16, check=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stages = hip.profile_read_stages()
    hip.profile_enable(False)
    return dt, {k: stages[k]['region_ms'] for k in ENC_STAGES}


def mean(xs):
    return sum(xs) / max(1, len(xs))


def main(argv=None):
    args = parse_args(argv)
    device = hip.require_device('cuda')
    blocks = synthetic.RESNET_BLOCKS['resnet101']
    sd = synthetic.milan_state_dict(args.vocab + 4, 'resnet101', seed=0)
    ctx = hip.Context(hip.make_dims(sd, args.vocab, blocks=blocks), sd, device)
    ctx.set_precision(args.precision)
    del sd
    base, masks = synthetic.exemplars(args.neurons, k=args.k, size=args.size, seed=1,
                                      device=str(device))
    lines = [f'image sharing on the benchmark chunk: resnet101 w64, {args.neurons} neurons x '
             f'{args.k} x {args.size}^2, beam {args.beam} + rerank, {args.precision}; '
             f'{args.rounds} alternating off/on steps per rate on {torch.cuda.get_device_name()}',
             'ms are per encoder pass (one chunk); noise = |mean of the even off legs - mean of '
             'the odd off legs|', '']
    for rate in [int(r) for r in args.rates.split(',')]:
        images, distinct = with_duplicates(base, rate, seed=100 + rate)
        for share in (False, True) * args.warmup:
            timed_leg(ctx, images, masks, args, share)
        ctx.image_sharing_stats(clear=True)
        legs = {False: [], True: []}
        for _ in range(args.rounds):
            for share in (False, True):
                legs[share].append(timed_leg(ctx, images, masks, args, share))
        slots, trunk = ctx.image_sharing_stats(clear=True)
        status = ctx.status(clear=True)
        off, on = legs[False], legs[True]

        def rate_of(ls):
            return args.neurons / mean([dt for dt, _ in ls])

        def stage(ls, k):
            return mean([st[k] for _, st in ls])

        noise_s = abs(mean([dt for dt, _ in off[0::2]]) - mean([dt for dt, _ in off[1::2]]))
        enc_off = sum(stage(off, k) for k in ENC_STAGES)
        enc_on = sum(stage(on, k) for k in ENC_STAGES)
        enc_noise = abs(sum(stage(off[0::2], k) for k in ENC_STAGES) -
                        sum(stage(off[1::2], k) for k in ENC_STAGES))
        lines += [
            f'duplicate rate {rate:3d} %: distinct images {distinct} of {args.neurons * args.k}; '
            f'trunk_images / slots = {trunk} / {slots} = {trunk / max(1, slots):.4f}; '
            f'status {status}',
            f'  neuron-descriptions/s   off {rate_of(off):8.1f}   on {rate_of(on):8.1f}   '
            f'(x{rate_of(on) / rate_of(off):.3f}; off-vs-off noise '
            f'{noise_s / mean([dt for dt, _ in off]) * 100:.2f} %)',
            f'  encoder stages, ms      off {enc_off:8.2f}   on {enc_on:8.2f}   '
            f'(off-vs-off noise {enc_noise:.2f} ms)',
        ]
        for k in ENC_STAGES:
            lines.append(f'    {k:<14} off {stage(off, k):8.2f}   on {stage(on, k):8.2f}')
        lines.append(f'  dedup kernels (enc_input on - off): '
                     f'{stage(on, "enc_input") - stage(off, "enc_input"):.2f} ms')
        lines.append('')
    ctx.close()
    text = '\n'.join(lines)
    print(text)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + '\n')


if __name__ == '__main__':
    main()
