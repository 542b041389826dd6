"""The native BigGAN generator walk and its attention kernel, at the reference's dissection
workload (biggan/imagenet: BigGAN-256, ch 96, attention at 128 x 128 with C = 192).

  (a) `hip.sagan_attention` (streaming fp32-MFMA kernel) at 128 x 128 pixels, C = 192, batch
      4, against torch's eager `bmm` + `softmax` + `bmm` in float32 on the same tensors, which
      is what pretorched's `Attention.forward` runs.  First a self-check of both against a
      float64 computation done in query chunks on the GPU.  After a warm-up the two alternate
      inside every sample; a sample is `--launches` launches between device events.  Beside the
      times: 2 Tq Tk (dk + dv) FLOP per image over the median, against the 157.3 TFLOP/s
      fp32-MFMA peak, and the peak memory each side allocates on top of its inputs.
      (Kernel-only time: `--only attention --native-only` under `rocprofv3 --kernel-trace
      --stats`.)
  (b) `SeqBigGAN.generate(inputs, 'layer5')` (the tap and the images) and
      `generate(inputs, 'layer0', images=False)` (the hiddens-only pass, which stops after
      block 0), native, at BigGAN-256 with ch 96 and random weights, batch 8 and batch 32,
      against `forward_eager` under `no_grad` with a retain hook on that child of the same
      module -- what a user without the native walk runs; the hook path cannot stop early.
      Same alternating protocol.  (Per-kernel shares of the native walk: `--only tap
      --native-only` under `rocprofv3 --kernel-trace --stats`.)

    python tools/bench_biggan.py [--steps 7] [--launches 10] [--out profiles/biggan.txt]

Prints the device clocks read before the run and JSON lines; `--out` appends the same text to
a file.  A report, not an assertion: no time is fixed in advance.
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd')]

from milan_amd import generators, hip  # noqa: E402

MFMA_F32_PEAK = 157.3e12


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
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / launches


def spread(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3),
                max=round(max(ms), 3))


def alternate(steps, warmup, launches, ours, theirs):
    for fn in (ours, theirs):
        if fn is not None:
            device_ms(fn, warmup)
    t_ours, t_theirs = [], []
    for _ in range(steps):
        t_ours.append(device_ms(ours, launches))
        if theirs is not None:
            t_theirs.append(device_ms(theirs, launches))
    return t_ours, t_theirs


def peak_extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2**20, 1)


def versus(row, t_new, t_old, ours, theirs):
    row[f'{ours}_ms'] = spread(t_new)
    if t_old:
        row[f'{theirs}_ms'] = spread(t_old)
        row[f'{theirs}_over_{ours}'] = round(statistics.median(t_old) / statistics.median(t_new), 2)
        row[f'{ours}_wins_beyond_spread'] = min(t_old) > max(t_new)
        row[f'{theirs}_wins_beyond_spread'] = min(t_new) > max(t_old)


def bench_attention(args, lines):
    n, side, C = args.attention_images, 128, 192
    dk, dv, Tq = C // 8, C // 2, side * side
    Tk = Tq // 4
    g = torch.Generator().manual_seed(0)
    # scores of order a few, as a trained block has: theta . phi over dk = 24 columns
    theta = (torch.randn(n, Tq, dk, generator=g) * .5).cuda()
    phi_g = torch.randn(n, Tk, dk + dv, generator=g).cuda()
    # pretorched's layout: (n, channels, pixels)
    theta_t = theta.transpose(1, 2).contiguous()
    phi_t = phi_g[..., :dk].transpose(1, 2).contiguous()
    g_t = phi_g[..., dk:].transpose(1, 2).contiguous()

    def native():
        return hip.sagan_attention(theta, phi_g, side, side)

    def eager():
        beta = torch.softmax(torch.bmm(theta_t.transpose(1, 2), phi_t), -1)
        return torch.bmm(g_t, beta.transpose(1, 2))

    got = native()
    err_native = err_eager = scale = 0.
    other = None if args.native_only else eager().transpose(1, 2)
    for q0 in range(0, Tq, 2048):  # float64, 2048 queries at a time
        want = torch.softmax(theta[:, q0:q0 + 2048].double() @
                             phi_g[..., :dk].double().transpose(1, 2), -1) @ phi_g[..., dk:].double()
        scale = max(scale, float(want.abs().max()))
        err_native = max(err_native, float((got[:, q0:q0 + 2048].double() - want).abs().max()))
        if other is not None:
            err_eager = max(err_eager, float((other[:, q0:q0 + 2048].double() - want).abs().max()))
    del other
    assert err_native <= 1e-5 * scale, (err_native, scale)
    row = dict(kernel='sagan_attention',
               shape=dict(images=n, pixels=f'{side}x{side}', C=C, queries=Tq, keys=Tk, dk=dk, dv=dv),
               launches_per_sample=args.launches, samples=args.steps,
               max_abs_err_vs_float64=dict(native=float(f'{err_native:.3g}'),
                                           eager=float(f'{err_eager:.3g}'),
                                           scale=float(f'{scale:.3g}')),
               native_peak_extra_MB=peak_extra_mb(native))
    if not args.native_only:
        row['eager_peak_extra_MB'] = peak_extra_mb(eager)
    t_new, t_old = alternate(args.steps, args.warmup, args.launches, native,
                             None if args.native_only else eager)
    flop = 2.0 * Tq * Tk * (dk + dv) * n
    med = statistics.median(t_new) * 1e-3
    row.update(achieved_TFLOPs=round(flop / med / 1e12, 1),
               of_fp32_mfma_peak=round(flop / med / MFMA_F32_PEAK, 3))
    versus(row, t_new, t_old, 'native', 'eager')
    lines.append(json.dumps(row))


def biggan256(max_images):
    model = generators.biggan(256, max_images=max_images, skip_init=True).eval().cuda()
    assert model.attention_channels == 192 and model.attn_resolution == 128
    g = torch.Generator(device='cuda').manual_seed(1)
    with torch.no_grad():  # activations of order one through the depth
        for name, p in model.state_dict().items():
            if name.endswith('stored_var'):
                p.copy_(.5 + torch.rand(p.shape, generator=g, device='cuda'))
            elif name.endswith('gamma'):
                p.fill_(.5)
            elif name.endswith('sv0'):
                p.fill_(1.)
            elif name.endswith('output_layer.0.gain'):
                p.fill_(1.)
            elif p.dim() >= 2 and not name.endswith('u0'):
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g, device='cuda') * 2. * fan_in**-.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g, device='cuda') * (1. if name.endswith('u0') else .1))
    return generators.SeqBigGAN(model)


def bench_tap(args, lines):
    seq = biggan256(args.max_images)
    gen = seq.generator
    g = torch.Generator().manual_seed(2)
    for n in args.batches:
        inputs = generators.GInputs(torch.randn(n, gen.dim_z, generator=g).cuda(),
                                    torch.randint(0, 1000, (n,), generator=g).cuda())
        for layer, images in (('layer5', True), ('layer0', False)):
            child = getattr(seq, layer)

            def native():
                with torch.no_grad():
                    return seq.generate(inputs, layer=layer, images=images)

            def eager():
                kept = []
                handle = child.register_forward_hook(lambda m, i, o: kept.append(o.h.detach()))
                try:
                    with torch.no_grad():
                        pictures = seq.forward_eager(inputs)
                finally:
                    handle.remove()
                return kept[0], pictures

            with torch.no_grad():
                assert seq.runs_natively(inputs), seq.native_refusal(inputs)
            bag, pictures = native()
            row = dict(workload=f'BigGAN-256 ch 96, generate({layer!r}, images={images}), '
                                f'batch {n}, {args.max_images} samples per native pass',
                       launches_per_sample=args.tap_launches, samples=args.steps,
                       native_peak_extra_MB=peak_extra_mb(native))
            if not args.native_only:
                hiddens, theirs = eager()
                row['tap_max_abs_diff_vs_eager_over_max'] = float(
                    f'{float((bag.h - hiddens).abs().max() / hiddens.abs().max()):.3g}')
                if images:
                    row['images_max_abs_diff_vs_eager'] = float(
                        f'{float((pictures - theirs).abs().max()):.3g}')
                del hiddens, theirs
                row['eager_peak_extra_MB'] = peak_extra_mb(eager)
            del bag, pictures
            t_new, t_old = alternate(args.steps, 1, args.tap_launches, native,
                                     None if args.native_only else eager)
            versus(row, t_new, t_old, 'native', 'eager_hook')
            row['native_samples_per_s'] = round(n / statistics.median(t_new) * 1e3, 1)
            lines.append(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--attention-images', type=int, default=4)
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 32])
    ap.add_argument('--max-images', type=int, default=8)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--tap-launches', type=int, default=2)
    ap.add_argument('--only', choices=('attention', 'tap'), default=None)
    ap.add_argument('--native-only', action='store_true',
                    help='skip the torch side (for a kernel trace of the native path)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    hip.require_device('cuda')   # (no GPU: an error, never a CPU timing)
    lines = [f'clocks: {clocks()}']
    if args.only in (None, 'attention'):
        bench_attention(args, lines)
    if args.only in (None, 'tap'):
        bench_tap(args, lines)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text)


if __name__ == '__main__':
    main()
