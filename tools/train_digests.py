"""Digests of what the LM and decoder training paths compute, for a bit-for-bit comparison of
two builds of libmilan_hip.  One line per case: the first 16 hex digits of the
sha256 of every output tensor's bytes (loss terms, every gradient, log-probs, picked log-probs,
attentions, the feature gradient) and the workspace byte counts.  Fixed seeds, small shapes: the
ones at which the parts the two trainers share (embedding gather, dropout, the LSTM cell, the
log-softmax pair, the output layer, the split-K GEMM and its combine) take each of their paths.

    MILAN_LIB=<one build>     python tools/train_digests.py [--full] > a.txt
    MILAN_LIB=<another build> python tools/train_digests.py [--full] > b.txt
    diff a.txt b.txt

The LM cases are the whole product of their values (48); the decoder's are 34, or with --full
the whole product (144).

One library per process.  The record of the refactor that introduced csrc/tgemm.hip and the
shared training kernels is profiles/train_refactor.txt.
"""
import hashlib
import itertools
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO), str(REPO / 'tests'),
                str(REPO / 'tests' / 'golden')]

from milan_amd import hip  # noqa: E402
from test_gpu_lm_train import random_state  # noqa: E402
from test_gpu_train_fuzz import decoder_setup, lm_batch  # noqa: E402

DEVICE = torch.device('cuda:0')
# V: not a multiple of 4, below and above one 256-thread stride.  (rows, L): one step, a few,
# and N = 256 positions, at which dW_out and dW_ih split K in two (combine kernel, scratch).
VOCABS, HIDDEN, SHAPES, DROPOUT = (37, 300), (8, 20), ((3, 1), (3, 5), (16, 16)), (0., .5)
LM_E, LM_LAYERS = 12, (1, 3)
# k up to the kMaxK bound; A = 72 > 64: more than one lane stride in the attention kernels
# (milan_create takes attention sizes that are multiples of 4 only)
DEC_F, DEC_E, DEC_K, DEC_A = 24, 12, (1, 3, 64), (8, 72)


def dg(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def dgs(tensors):
    return ' '.join(dg(t) for t in tensors)


def nan_like(tensors):
    return [torch.full_like(t, float('nan')) for t in tensors]


def upstream(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEVICE)


def lm_cases():
    index = 0
    for layers, h, v, (rows, length), p in itertools.product(LM_LAYERS, HIDDEN, VOCABS, SHAPES,
                                                             DROPOUT):
        index += 1
        sd = random_state(v, LM_E, h, layers, seed=index)
        inputs, targets = lm_batch(v, rows, length, 100 + index)  # pads, one all-pad row
        inputs, targets = inputs.to(DEVICE), targets.to(DEVICE)
        dims = hip.make_dims({f'lm.{k}': t for k, t in sd.items()}, v - 4)
        ctx = hip.Context(dims, {}, DEVICE, finalize=False)
        params = [t.to(DEVICE).contiguous() for t in sd.values()]
        seed = 0x5eed0000 + index
        tag = f'lm layers={layers} H={h} V={v} rows={rows} L={length} p={p}'
        print(tag, 'workspace',
              int(ctx.lib.milan_lm_train_workspace_bytes(ctx._h, rows, length)),
              int(ctx.lib.milan_lm_grad_workspace_bytes(ctx._h, rows, length)))
        print(tag, 'nll', dg(ctx.lm_nll(params, inputs, targets)))
        grads = nan_like(params)
        loss = ctx.lm_train_step(params, grads, inputs, targets, p, seed)
        print(tag, 'step loss', dg(loss), 'grads', dgs(grads))
        d_lp, d_pk = upstream((rows, length, v), index), upstream((rows, length), 50 + index)
        for name, want_lp, want_pk in (('dlogprobs', True, False), ('dpicked', False, True),
                                       ('both', True, True)):
            logprobs, picked, ws = ctx.lm_forward_train(
                params, inputs, p, seed, targets=targets if want_pk else None,
                want_logprobs=want_lp)
            grads = nan_like(params)
            ctx.lm_backward(params, grads, inputs, p, seed, d_lp if want_lp else None,
                            d_pk if want_pk else None, targets if want_pk else None, ws)
            outs = [t for t in (logprobs, picked) if t is not None]
            print(tag, f'autograd {name} out', dgs(outs), 'grads', dgs(grads))
        ctx.close()


def decoder_shapes(full):
    """(k, A, H, V, (rows, L), p).  --full: the whole product, 144 cases.  Otherwise the 34 that
    vary one group at a time: H, V, (rows, L) and p at k = 3, A = 8 (what the shared kernels
    see), then k and A (what only the attention kernels see) at a small and a split-K shape."""
    every = list(itertools.product(DEC_K, DEC_A, HIDDEN, VOCABS, SHAPES, DROPOUT))
    bases = ((8, 37, (3, 5), .5), (20, 300, (16, 16), 0.))
    return [c for c in every if full or c[:2] == (3, 8) or c[2:] in bases]


def decoder_cases(full):
    for k, a, h, v, (rows, length), p in decoder_shapes(full):
        # (the seeds of a case: a function of the case, so both sets draw the same)
        index = 1000 * k + 100 * a + 10 * h + v + rows + length + int(2 * p)
        case = dict(V=v, F=DEC_F, H=h, E=DEC_E, A=a, rows=rows, k=k, L=length)
        _, feats, targets, ctx, params = decoder_setup(DEVICE, case, index)
        feats, targets = feats.to(DEVICE), targets.to(DEVICE)
        seed = 0xdec0000 + index
        tag = f'decoder k={k} A={a} H={h} V={v} rows={rows} L={length} p={p}'
        print(tag, 'workspace',
              int(ctx.lib.milan_decoder_train_workspace_bytes(ctx._h, rows, k, length)),
              int(ctx.lib.milan_decoder_grad_workspace_bytes(ctx._h, rows, k, length)))
        print(tag, 'nll', dg(ctx.decoder_nll(params, feats, targets)))
        for reg in (0., 1.):
            grads = nan_like(params)
            loss = ctx.decoder_train_step(params, grads, feats, targets, p, seed, reg)
            print(tag, f'step reg={reg} loss', dg(loss), 'grads', dgs(grads))
        d_lp, d_at = upstream((rows, length, v), index), upstream((rows, length, k), 50 + index)
        for want_lp, want_at, want_df in itertools.product((True, False), repeat=3):
            if not (want_lp or want_at):
                continue
            logprobs, attentions, ws = ctx.decoder_forward_train(params, feats, targets, p, seed)
            grads = nan_like(params)
            dfeat = torch.full_like(feats, float('nan')) if want_df else None
            ctx.decoder_backward(params, grads, feats, targets, p, seed,
                                 d_lp if want_lp else None, d_at if want_at else None, dfeat, ws)
            name = f'dlogprobs={int(want_lp)} dattentions={int(want_at)} dfeatures={int(want_df)}'
            print(tag, f'autograd {name} out', dgs([logprobs, attentions]), 'grads', dgs(grads),
                  'dfeatures', dg(dfeat) if want_df else '-')
        ctx.close()


def main():
    hip.require_device(DEVICE)
    lm_cases()
    decoder_cases('--full' in sys.argv[1:])
    torch.cuda.synchronize()
    print('done')


if __name__ == '__main__':
    main()
