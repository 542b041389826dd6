"""Cost of a beam-search step by beam width and selection path, at the
benchmark's decoder dims (vocabulary 5004, 15 exemplars of 3904 features, split_f16).

    python tools/bench_beam_wide.py [--neurons 64] [--length 15] [--steps 3] \
        [--config 124:0 124:1 125:0 256:0 1000:0]

A configuration is `beam:path` (path as in `Context.set_beam_path`: 0 = by beam width,
1 = the wide kernels forced).  Prints one JSON line per configuration: ms per decode step
(the search stage's HIP-event time over `length` steps, median of `--steps` calls) and
the token hash of the result, which must agree between the paths of one beam.

    python tools/bench_beam_wide.py --kernel-stats DIR

summarises the result databases that `rocprofv3 --kernel-trace --stats` runs of this
script (one process per configuration) left in DIR: the share of the selection
kernels in the GPU time of that process.
"""
import argparse
import hashlib
import json
import pathlib
import statistics
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd')]

SELECTION = ('beam_merge_wide_kernel', 'row_select_wide_reg_kernel', 'row_select_wide_kernel',
             'beam_merge_kernel', 'row_select_reg_kernel', 'row_select_kernel')


def kernel_stats(directory):
    import sqlite3
    for path in sorted(pathlib.Path(directory).rglob('*.db')):
        db = sqlite3.connect(str(path))
        rows = db.execute('select name, count(*), sum(end - start) from kernels '
                          'group by name order by 3 desc').fetchall()
        total = sum(r[2] for r in rows) or 1
        share = {}
        for name, calls, ns in rows:
            for kernel in SELECTION:
                if f'::{kernel}(' in name or f'::{kernel}<' in name or name.endswith(kernel):
                    share[kernel] = round(share.get(kernel, 0.) + ns / total, 4)
        top = [[name[:60], calls, round(ns / total, 4)] for name, calls, ns in rows[:6]]
        print(json.dumps(dict(file=path.name, gpu_ms=round(total / 1e6, 2), share=share,
                              top=top)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--neurons', type=int, default=64)
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--length', type=int, default=15)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--precision', default='split_f16')
    ap.add_argument('--config', nargs='+',
                    default=['124:0', '124:1', '125:0', '256:0', '1000:0'])
    ap.add_argument('--kernel-stats')
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)

    import torch
    from milan_amd import hip, synthetic
    nv = 5000
    sd = synthetic.decoder_state_dict(nv + 4, seed=0)
    ctx = hip.Context(hip.make_dims(sd, nv), sd, 'cuda')
    ctx.set_precision(args.precision)
    feats = torch.rand(args.neurons, args.k, 3904,
                       generator=torch.Generator().manual_seed(1)).cuda()
    for config in args.config:
        beam, path = (int(x) for x in config.split(':'))
        ctx.set_beam_path(path)
        run = lambda: ctx.decode(feats, hip.BEAM, args.length, beam, False, 0.2)  # noqa: E731
        for _ in range(args.warmup):
            out = run()
        torch.cuda.synchronize()
        stage_ms = {}
        for _ in range(args.steps):
            hip.profile_enable(True)
            out = run()
            torch.cuda.synchronize()
            stages = hip.profile_read_stages()
            hip.profile_enable(False)
            for name in ('dec_init', 'dec_search', 'dec_lm'):
                stage_ms.setdefault(name, []).append(stages[name]['region_ms'])
        med = {name: statistics.median(v) for name, v in stage_ms.items()}
        digest = hashlib.sha256(out['beam_tokens'].cpu().numpy().tobytes()).hexdigest()[:12]
        print(json.dumps(dict(
            beam=beam, path='wide forced' if path else 'auto', neurons=args.neurons,
            length=args.length, precision=args.precision,
            ms_per_step=round(med['dec_search'] / args.length, 3),
            search_ms=round(med['dec_search'], 2), init_ms=round(med['dec_init'], 3),
            select_ms=round(med['dec_lm'], 3),
            workspace_gib=round(ctx.workspace(args.neurons, args.k, 0, beam,
                                              args.length).numel() / 2**30, 2),
            beam_tokens_sha256=digest)), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
