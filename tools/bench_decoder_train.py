#!/usr/bin/env python3
"""Throughput of Decoder training steps: the HIP path (milan_decoder_train_step
+ torch AdamW, what `Decoder.fit` runs per batch) against the same decoder
built from torch.nn modules (Linear / Embedding / LSTMCell, the reference's
teacher-forced loop, autograd) on the same GPU, same batches, same optimizer.

Benchmark decoder: F = 3904 (the pyramid ResNet-101 features), H = 512,
E = 128, attention hidden 512, V = 5004, k = 15 features per row, batch 64,
dropout 0.5, regularisation weight 1, synthetic captions of 5..14 words
(L = 16 targets with <stop>).  Features are precomputed (the encoder is frozen)
and, like the batches, sit on the device before the timed window; a step is
forward + loss + backward + optimizer step; the window ends with a device
synchronise.

The `autograd` leg is a user's own loop on the differentiable training-mode
`Decoder.forward` (milan_decoder_forward_train / milan_decoder_backward): the
reference's loss in torch on its outputs, loss.backward(), AdamW.

    python tools/bench_decoder_train.py --steps 30 --warmup 5 [--only hip|autograd|torch] [--out f.json]

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
from torch import nn  # noqa: E402

from milan_amd import decoders, encoders, hip, lang  # noqa: E402

V_WORDS, F, E, H, K, BATCH, L, DROPOUT, REG = 5000, 3904, 128, 512, 15, 64, 16, .5, 1.


class _Features(encoders.Encoder):
    feature_shape = (F,)


def batches(indexer, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    zipf = 1.0 / torch.arange(1, V_WORDS + 1, dtype=torch.float64)
    out = []
    for _ in range(n):
        texts = []
        for _ in range(BATCH):
            k = int(torch.randint(5, L - 1, (), generator=g))
            ids = torch.multinomial(zipf, k, replacement=True, generator=g)
            texts.append(' '.join(f'w{i}' for i in ids.tolist()))
        targets = torch.tensor(indexer(texts, length=L - 1))[:, 1:]
        feats = torch.rand(BATCH, K, F, generator=g)
        out.append((feats, targets))
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
    model = decoders.Decoder(indexer, _Features(), embedding_size=E, hidden_size=H,
                             dropout=DROPOUT)
    torch.manual_seed(0)
    model.reset_parameters()
    model.to(dev)
    weights = model._train_params()
    grads = [torch.empty_like(p) for p in weights]
    sd = {k: v for k, v in model.state_dict().items()}
    ctx = hip.Context(hip.make_dims(sd, len(indexer.vocab)), {}, dev, finalize=False)
    opt = torch.optim.AdamW(model.parameters())
    gen = torch.cuda.default_generators[dev.index]
    data = [(f.to(dev), t.to(dev)) for f, t in data]

    def step(feats, targets):
        seed = int(torch.randint(2**62, (), device=dev, generator=gen))
        ctx.decoder_train_step(weights, grads, feats, targets, DROPOUT, seed, REG)
        for p, g in zip(weights, grads):
            p.grad = g
        opt.step()
        opt.zero_grad()

    seconds = timed(step, data, warmup, steps)
    ctx.close()
    return seconds


def bench_autograd(indexer, data, dev, warmup, steps):
    """A user's own loop on the differentiable training-mode forward: the
    forward (milan_decoder_forward_train), the reference's loss in torch on its
    outputs, loss.backward() (milan_decoder_backward) and AdamW."""
    model = decoders.Decoder(indexer, _Features(), embedding_size=E, hidden_size=H,
                             dropout=DROPOUT)
    torch.manual_seed(0)
    model.reset_parameters()
    model.to(dev).train()
    opt = torch.optim.AdamW(model.parameters())
    crit = nn.NLLLoss(ignore_index=indexer.pad_index)
    data = [(f.to(dev), t.to(dev)) for f, t in data]

    def step(feats, targets):
        out = model(feats, length=targets.shape[1], strategy=targets, mi=False)
        loss = crit(out.predictions.permute(0, 2, 1), targets)
        loss = loss + REG * ((1 - out.attentions.sum(dim=1))**2).mean()
        loss.backward()
        opt.step()
        opt.zero_grad()

    seconds = timed(step, data, warmup, steps)
    ctx = model._train_context()
    ws = int(ctx.lib.milan_decoder_grad_workspace_bytes(ctx._h, BATCH, K, L))
    step_ws = int(ctx.lib.milan_decoder_train_workspace_bytes(ctx._h, BATCH, K, L))
    return seconds, dict(workspace_bytes=ws, train_step_workspace_bytes=step_ws)


class TorchDecoder(nn.Module):
    """The reference's decoder modules and teacher-forced training loss."""

    def __init__(self, v):
        super().__init__()
        self.init_h = nn.Sequential(nn.Linear(F, H), nn.Tanh())
        self.init_c = nn.Sequential(nn.Linear(F, H), nn.Tanh())
        self.embedding = nn.Embedding(v, E)
        self.query = nn.Linear(H, H)
        self.key = nn.Linear(F, H)
        self.score = nn.Linear(H, 1)
        self.feature_gate = nn.Sequential(nn.Linear(H, F), nn.Sigmoid())
        self.lstm = nn.LSTMCell(E + F, H)
        self.output = nn.Sequential(nn.Dropout(DROPOUT), nn.Linear(H, v),
                                    nn.LogSoftmax(dim=-1))

    def forward(self, feats, targets, start):
        pooled = feats.mean(dim=1)
        h, c = self.init_h(pooled), self.init_c(pooled)
        keys = self.key(feats)
        current = torch.full((len(feats),), start, dtype=torch.long, device=feats.device)
        preds, atts = [], []
        for t in range(targets.shape[1]):
            hidden = torch.tanh(self.query(h).unsqueeze(1) + keys)
            a = torch.softmax(self.score(hidden).squeeze(-1), dim=1)
            gated = (a.unsqueeze(-1) * feats).sum(dim=1) * self.feature_gate(h)
            h, c = self.lstm(torch.cat((self.embedding(current), gated), -1), (h, c))
            preds.append(self.output(h))
            atts.append(a)
            current = targets[:, t]
        return torch.stack(preds, 1), torch.stack(atts, 1)


def bench_torch(indexer, data, dev, warmup, steps):
    torch.manual_seed(0)
    model = TorchDecoder(len(indexer)).to(dev).train()
    opt = torch.optim.AdamW(model.parameters())
    crit = nn.NLLLoss(ignore_index=indexer.pad_index)
    data = [(f.to(dev), t.to(dev)) for f, t in data]

    def step(feats, targets):
        preds, atts = model(feats, targets, indexer.start_index)
        loss = crit(preds.permute(0, 2, 1), targets)
        loss = loss + REG * ((1 - atts.sum(dim=1))**2).mean()
        loss.backward()
        opt.step()
        opt.zero_grad()

    return timed(step, data, warmup, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=('hip', 'autograd', 'torch'))
    ap.add_argument('--out')
    args = ap.parse_args()
    dev = hip.require_device('cuda')
    indexer = lang.Indexer(lang.Vocab(tuple(f'w{i}' for i in range(V_WORDS))),
                           _tokenize, True, True, True, True)
    data = batches(indexer, 8)
    tokens = [int((t != indexer.pad_index).sum()) for _, t in data]
    per_step = sum(tokens) / len(tokens)
    result = dict(model=dict(V=len(indexer), F=F, E=E, H=H, k=K, batch=BATCH,
                             L=int(data[0][1].shape[1]), dropout=DROPOUT,
                             regularization_weight=REG),
                  steps=args.steps, warmup=args.warmup, tokens_per_step=per_step)
    for name, fn in (('hip', bench_hip), ('autograd', bench_autograd),
                     ('torch', bench_torch)):
        if args.only and args.only != name:
            continue
        seconds = fn(indexer, data, dev, args.warmup, args.steps)
        extra = {}
        if isinstance(seconds, tuple):
            seconds, extra = seconds
        result[name] = dict(ms_per_step=1e3 * seconds / args.steps,
                            tokens_per_s=per_step * args.steps / seconds, **extra)
    if 'hip' in result and 'torch' in result:
        result['hip_over_torch_time'] = (result['hip']['ms_per_step'] /
                                         result['torch']['ms_per_step'])
    if 'hip' in result and 'autograd' in result:
        result['autograd_over_hip_time'] = (result['autograd']['ms_per_step'] /
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
