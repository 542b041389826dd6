"""The native DINO ViT-S/8 walk and its attention kernel, at the reference's dissection
workload (dino_vits8, 224 x 224, batch 32: 32 x 6 sequence-heads of 785 tokens, head size 64).

  (a) `hip.attention` (streaming fp32-MFMA kernel) against torch's own
      `F.scaled_dot_product_attention` in float32 on the same q, k, v.  After a warm-up the
      two alternate inside every sample; a sample is `--launches` launches between device
      events.  Beside the times: 4 T^2 hd FLOP per sequence-head over the median, against the
      157.3 TFLOP/s fp32-MFMA peak.  (Kernel-only time: run this tool with `--only attention
      --native-only` under `rocprofv3 --kernel-trace --stats`.)
  (b) `VisionTransformer.activations(images, 'blocks.11.mlp.fc1')`, native, against the same
      module's `forward_eager` under `no_grad` with a retain hook on that layer -- what a user
      without the native walk runs.  Same alternating protocol.  (Per-kernel shares of the
      native walk: `--only tap --native-only` under `rocprofv3 --kernel-trace --stats`.)

    python tools/bench_vit.py [--steps 7] [--launches 20] [--out profiles/vit_taps.txt]

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
import torch.nn.functional as F

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd')]

from milan_amd import hip, vits  # noqa: E402

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


def alternate(args, ours, theirs):
    for fn in (ours, theirs):
        if fn is not None:
            device_ms(fn, args.warmup)
    t_ours, t_theirs = [], []
    for _ in range(args.steps):
        t_ours.append(device_ms(ours, args.launches))
        if theirs is not None:
            t_theirs.append(device_ms(theirs, args.launches))
    return t_ours, t_theirs


def bench_attention(args, lines):
    seqs, T, heads, hd = args.images, 785, 6, 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(seqs, T, 3 * heads * hd, generator=g).cuda()
    q, k, v = qkv.reshape(seqs, T, 3, heads, hd).permute(2, 0, 3, 1, 4).contiguous()

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v)

    got = hip.attention(qkv, heads)
    want = sdpa().transpose(1, 2).reshape(seqs, T, heads * hd)
    t_new, t_old = alternate(args, lambda: hip.attention(qkv, heads),
                             None if args.native_only else sdpa)
    flop = 4.0 * T * T * hd * seqs * heads
    med = statistics.median(t_new) * 1e-3
    row = dict(kernel='attention', shape=dict(seqs=seqs, T=T, heads=heads, head_size=hd),
               launches_per_sample=args.launches, samples=args.steps,
               hip_attention_ms=spread(t_new), achieved_TFLOPs=round(flop / med / 1e12, 1),
               of_fp32_mfma_peak=round(flop / med / MFMA_F32_PEAK, 3),
               max_abs_diff_vs_torch=float(f'{float((got - want).abs().max()):.3g}'))
    if t_old:
        row.update(torch_sdpa_fp32_ms=spread(t_old),
                   torch_over_hip=round(statistics.median(t_old) / statistics.median(t_new), 2),
                   hip_wins_beyond_spread=min(t_old) > max(t_new),
                   torch_wins_beyond_spread=min(t_new) > max(t_old))
    lines.append(json.dumps(row))


def bench_tap(args, lines):
    g = torch.Generator().manual_seed(1)
    model = vits.dino_vits8(max_images=args.images)
    with torch.no_grad():   # activations of order one through the depth
        for name, p in model.named_parameters():
            if name.endswith('norm1.weight') or name.endswith('norm2.weight') or \
                    name == 'norm.weight':
                p.copy_(1. + .1 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and 'token' not in name and 'pos_embed' not in name:
                p.copy_(torch.randn(p.shape, generator=g) * p[0].numel()**-0.5)
            else:
                p.copy_(.1 * torch.randn(p.shape, generator=g))
    model.eval().cuda()
    images = torch.randn(args.images, 3, 224, 224, generator=g).cuda()
    layer = 'blocks.11.mlp.fc1'
    module = dict(model.named_modules())[layer]

    def native():
        with torch.no_grad():
            return model.activations(images, layer)[layer]

    def eager():
        kept = []
        handle = module.register_forward_hook(lambda m, i, o: kept.append(o.detach()))
        try:
            with torch.no_grad():
                model.forward_eager(images)
        finally:
            handle.remove()
        return kept[0]

    with torch.no_grad():
        assert model.runs_natively(images)
    a = native()
    row = dict(workload=f'dino_vits8 {layer}, {args.images} images of 224 x 224',
               launches_per_sample=args.tap_launches, samples=args.steps)
    if not args.native_only:
        b = eager()
        row['max_abs_diff_vs_eager_over_max'] = float(
            f'{float((a - b).abs().max() / b.abs().max()):.3g}')
    saved = args.launches
    args.launches = args.tap_launches
    t_new, t_old = alternate(args, native, None if args.native_only else eager)
    args.launches = saved
    row['native_ms'] = spread(t_new)
    row['native_images_per_s'] = round(args.images / statistics.median(t_new) * 1e3, 1)
    if t_old:
        row.update(eager_hook_ms=spread(t_old),
                   eager_over_native=round(statistics.median(t_old) / statistics.median(t_new), 2),
                   native_wins_beyond_spread=min(t_old) > max(t_new),
                   eager_wins_beyond_spread=min(t_new) > max(t_old))
    lines.append(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--tap-launches', type=int, default=3)
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
