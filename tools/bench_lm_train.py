#!/usr/bin/env python3
"""Throughput of LanguageModel training steps: the HIP path (milan_lm_train_step
+ torch AdamW, what `LanguageModel.fit` runs per batch) against the same model
built from torch.nn modules (nn.Embedding / nn.LSTM / nn.Linear, autograd) on
the same GPU, same batches, same optimizer.

Benchmark LM: V = 5004, E = 128, H = 512, 2 layers, dropout 0.5, batch 128,
synthetic captions of 5..15 words (L = 16 with <start> / <stop>).  Batches
are indexed on the host before the timed window; a step is forward + loss +
backward + optimizer step; the window ends with a device synchronise.
tokens/s counts the non-pad targets.

    python tools/bench_lm_train.py --steps 50 --warmup 10 [--only hip|torch] [--out f.json]

`--autograd` times, in the same process and on the same batches, the fused step
and a user's loop on the differentiable training-mode `LanguageModel.forward`
(DESIGN.md 4.16): forward + `F.nll_loss(ignore_index=pad)` + `backward()` +
AdamW, and `forward(reduce=True)` with a sum loss.  There is no threshold: the
fused step of the same run is the yardstick.

Needs an MI355X; prints one JSON line.
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'neuron-descriptions_amd'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from milan_amd import hip, lang, lms  # noqa: E402

V_WORDS, E, H, LAYERS, BATCH, DROPOUT = 5000, 128, 512, 2, 128, 0.5


def batches(indexer, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    zipf = 1.0 / torch.arange(1, V_WORDS + 1, dtype=torch.float64)
    out = []
    for _ in range(n):
        texts = []
        for _ in range(BATCH):
            k = int(torch.randint(5, 16, (), generator=g))
            ids = torch.multinomial(zipf, k, replacement=True, generator=g)
            texts.append(' '.join(f'w{i}' for i in ids.tolist()))
        inputs = torch.tensor(indexer(texts, start=True, stop=False, pad=True, unk=True))
        targets = torch.tensor(indexer(texts, start=False, stop=True, pad=True, unk=True))
        out.append((inputs, targets))
    return out


def timed(step, data, warmup, steps):
    for i in range(warmup):
        step(*data[i % len(data)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(*data[i % len(data)])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_hip(indexer, data, dev, warmup, steps):
    torch.manual_seed(0)
    model = lms.LanguageModel(indexer, E, H, LAYERS, DROPOUT)
    model.reset_parameters()
    model.to(dev)
    named = dict(model.named_parameters())
    weights = [named[n] for n in model._param_names()]
    grads = [torch.empty_like(p) for p in weights]
    sd = {f'lm.{k}': v for k, v in model.state_dict().items()}
    ctx = hip.Context(hip.make_dims(sd, len(indexer.vocab)), {}, dev, finalize=False)
    opt = torch.optim.AdamW(model.parameters())
    gen = torch.cuda.default_generators[dev.index]

    def step(inputs, targets):  # host tensors, as fit passes them
        seed = int(torch.randint(2**62, (), device=dev, generator=gen))
        ctx.lm_train_step(weights, grads, inputs, targets, DROPOUT, seed)
        for p, g in zip(weights, grads):
            p.grad = g
        opt.step()
        opt.zero_grad()

    seconds = timed(step, data, warmup, steps)
    ctx.close()
    return seconds


def bench_autograd(indexer, data, dev, warmup, steps, reduce=False):
    """A user's loop on the training-mode forward: log-probs + nll_loss, or
    (reduce) the sequence scores with a sum loss; backward; AdamW."""
    torch.manual_seed(0)
    model = lms.LanguageModel(indexer, E, H, LAYERS, DROPOUT)
    model.reset_parameters()
    model.to(dev)
    model.requires_grad_(True)
    model.train()
    opt = torch.optim.AdamW(model.parameters())
    pad = indexer.pad_index
    data = [(i.to(dev), t.to(dev)) for i, t in data]

    def step(inputs, targets):
        if reduce:
            loss = -model(inputs, reduce=True).sum()
        else:
            lp = model(inputs)
            loss = F.nll_loss(lp.reshape(-1, lp.shape[-1]), targets.reshape(-1),
                              ignore_index=pad)
        loss.backward()
        opt.step()
        opt.zero_grad()

    return timed(step, data, warmup, steps)


def bench_torch(indexer, data, dev, warmup, steps):
    torch.manual_seed(0)
    v = len(indexer)
    emb = nn.Embedding(v, E, padding_idx=indexer.pad_index).to(dev)
    lstm = nn.LSTM(E, H, LAYERS, dropout=DROPOUT, batch_first=True).to(dev)
    out = nn.Sequential(nn.Linear(H, v), nn.LogSoftmax(dim=-1)).to(dev)
    params = list(emb.parameters()) + list(lstm.parameters()) + list(out.parameters())
    opt = torch.optim.AdamW(params)
    crit = nn.NLLLoss(ignore_index=indexer.pad_index)
    lstm.train()
    data = [(i.to(dev), t.to(dev)) for i, t in data]

    def step(inputs, targets):
        hiddens, _ = lstm(emb(inputs))
        loss = crit(out(hiddens).permute(0, 2, 1), targets)
        loss.backward()
        opt.step()
        opt.zero_grad()

    return timed(step, data, warmup, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--only', choices=('hip', 'torch'))
    ap.add_argument('--autograd', action='store_true',
                    help='the fused step against the differentiable forward')
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = hip.require_device('cuda')
    indexer = lang.Indexer(lang.Vocab(tuple(f'w{i}' for i in range(V_WORDS))),
                           _tokenize)
    data = batches(indexer, 16)
    tokens = [int((t != indexer.pad_index).sum()) for _, t in data]
    per_step = sum(tokens) / len(tokens)
    result = dict(model=dict(V=len(indexer), E=E, H=H, layers=LAYERS, batch=BATCH,
                             L=int(data[0][0].shape[1]), dropout=DROPOUT),
                  steps=args.steps, warmup=args.warmup, tokens_per_step=per_step)
    legs = [('hip', bench_hip), ('torch', bench_torch)]
    if args.autograd:
        ctx = hip.Context(hip.make_dims(
            {f'lm.{k}': v for k, v in
             lms.LanguageModel(indexer, E, H, LAYERS, DROPOUT).state_dict().items()},
            len(indexer.vocab)), {}, dev, finalize=False)
        rows, length = data[0][0].shape
        result['workspace_bytes'] = dict(
            train_step=int(ctx.lib.milan_lm_train_workspace_bytes(ctx._h, rows, length)),
            autograd=int(ctx.lib.milan_lm_grad_workspace_bytes(ctx._h, rows, length)))
        ctx.close()
        legs = [('hip', bench_hip), ('autograd', bench_autograd),
                ('autograd_reduce',
                 lambda *a: bench_autograd(*a, reduce=True))]
    for name, fn in legs:
        if args.only and args.only != name:
            continue
        seconds = fn(indexer, data, dev, args.warmup, args.steps)
        result[name] = dict(ms_per_step=1e3 * seconds / args.steps,
                            tokens_per_s=per_step * args.steps / seconds)
    if 'hip' in result and 'torch' in result:
        result['hip_over_torch_time'] = (result['hip']['ms_per_step'] /
                                         result['torch']['ms_per_step'])
    for name in ('autograd', 'autograd_reduce'):
        if name in result and 'hip' in result:
            result[f'{name}_over_hip_time'] = (result[name]['ms_per_step'] /
                                               result['hip']['ms_per_step'])
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + '\n')


def _tokenize(texts):
    if isinstance(texts, str):
        return tuple(texts.split())
    return tuple(tuple(t.split()) for t in texts)


if __name__ == '__main__':
    main()
