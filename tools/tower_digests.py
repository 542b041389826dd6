"""Digests of what the three transformer towers compute, for a bit-for-bit comparison of two
builds of libmilan_hip.  One line per case: the first 16 hex digits of the sha256
of each result tensor's bytes, and the workspace byte counts.  Fixed seeds, small shapes: the
ones at which the shared parts (LDS attention, LayerNorm rows, L2 norm, the weight arena) take
each of their paths.

    MILAN_LIB=<one build>     python tools/tower_digests.py > a.txt
    MILAN_LIB=<another build> python tools/tower_digests.py > b.txt
    diff a.txt b.txt

One library per process.  The record of the refactor that introduced csrc/tower.hip is
profiles/tower_refactor.txt.
"""
import hashlib
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO), str(REPO / 'tests'),
                str(REPO / 'tests' / 'golden')]

import bert_standin  # noqa: E402
import clip_standin  # noqa: E402
import vitref  # noqa: E402
from milan_amd import bertscore, hip, rerankers  # noqa: E402
from test_gpu_clip import FUZZ, random_tokens  # noqa: E402
from test_gpu_vit import CASES  # noqa: E402

DEVICE = torch.device('cuda:0')


def dg(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def bert_cases():
    lengths = (3, 4, 17, 64)
    for kind in ('bert', 'roberta'):
        for hd in (20, 72):
            cfg = dict(bert_standin.CONFIGS[kind], width=2 * hd, heads=2, layers=2, num_layers=2,
                       max_positions=70)
            sd = bert_standin.state_dict(cfg, 31 + hd)
            pad = bert_standin.ids_of(cfg)['pad_id']
            dims = bertscore.infer_dims(sd, 2, 2, None, pad, cfg['eps'])
            weights = {k: v for k, v in bertscore.strip_prefix(sd)[0].items()
                       if k.startswith('embeddings.') or k.startswith('encoder.')}
            ctx = hip.BertContext(hip.BertDims(**dims), weights, DEVICE)
            g = torch.Generator().manual_seed(7)
            ids = torch.randint(0, dims['vocab_size'], (sum(lengths),), generator=g).to(DEVICE)
            bounds = [0]
            for n in lengths:
                bounds.append(bounds[-1] + n)
            offsets = torch.tensor(bounds, dtype=torch.int32, device=DEVICE)
            idf = (.5 + torch.rand(sum(lengths), generator=g)).to(DEVICE)
            cand = torch.tensor([0, 1, 2, 3, 3, 2], dtype=torch.int32)
            ref = torch.tensor([1, 2, 3, 0, 3, 0], dtype=torch.int32)
            tag = f'bert.{kind}.hd{hd} offset={dims["position_offset"]}'
            for normalize in (0, 1):
                batch = ctx.encode(ids, offsets, max(lengths), bool(normalize))
                single = []
                for a, b in zip(bounds, bounds[1:]):
                    one = torch.tensor([0, b - a], dtype=torch.int32, device=DEVICE)
                    single.append(ctx.encode(ids[a:b].contiguous(), one, b - a, bool(normalize)))
                pairs = ctx.score_pairs(batch, offsets, idf, cand, ref)
                print(tag, f'normalize={normalize} batch', dg(batch), 'single',
                      ' '.join(dg(s) for s in single), 'pairs', dg(pairs))
            ws = [int(ctx.lib.milan_bert_encode_workspace_bytes(ctx._h, n, total))
                  for n, total in ((1, 3), (4, 88), (200, 6000))]
            print(tag, 'workspace', *ws)
            ctx.close()


def clip_cases():
    for index in (0, 3):
        fuzz = FUZZ[index]
        clip_standin.configure(seed=100 + index, **fuzz)
        sd = {k: v for k, v in clip_standin.load()[0].state_dict().items()
              if v.dtype.is_floating_point}
        dims = rerankers.infer_dims(sd, fuzz['vision_heads'], fuzz['text_heads'])
        ctx = hip.ClipContext(hip.ClipDims(**dims), sd, DEVICE)
        g = torch.Generator().manual_seed(300 + index)
        res, layers, context = dims['resolution'], dims['vision_layers'], dims['context_length']
        images = torch.randn(4, 3, res, res, generator=g)
        masks = torch.rand(4, 1, res, res, generator=g)
        tokens = random_tokens(g, 6, dims, longest=3)
        mul_add = (1.1, .9, 1.05, -.1, .2, .05)
        tag = f'clip.fuzz{index}'
        both = {}
        for bits in (0b01, (1 << layers) - 1):
            for ma in (mul_add, None):
                both[bits, ma] = ctx.encode_images(images, masks, bits, True, ma)
                print(tag, f'images both mask_layers={bits:#b} mul_add={ma is not None}',
                      dg(both[bits, ma]))
        print(tag, 'images masked alone', dg(ctx.encode_images(images, masks, 0b01, False, None)))
        print(tag, 'images no masks', dg(ctx.encode_images(images)),
              dg(ctx.encode_images(images, mul_add=mul_add)))
        texts = ctx.encode_texts(tokens, context)
        print(tag, f'texts positions={context}', dg(texts), 'positions=5',
              dg(ctx.encode_texts(tokens, 5)))
        em, eu = (t.reshape(2, 2, -1) for t in both[0b01, None])
        neuron_of = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32)
        print(tag, 'rerank neuron_of', dg(ctx.rerank_scores(em, eu, texts, neuron_of, 0, .3)),
              'candidates=3', dg(ctx.rerank_scores(em, eu, texts, None, 3, .3)))
        ws = [int(ctx.lib.milan_clip_image_workspace_bytes(ctx._h, n, b))
              for n in (1, 7, 200) for b in (0, 1)]
        ws += [int(ctx.lib.milan_clip_text_workspace_bytes(ctx._h, rows, p))
               for rows in (1, 7, 200) for p in (context, 5)]
        print(tag, 'workspace', *ws)
        ctx.close()


def vit_cases():
    for index in (0, 1):
        *shape, _ = CASES[index]
        d = vitref.make_dims(*shape)
        sd = vitref.cast(vitref.weights(d, seed=100 + index), torch.float32)
        dims = hip.VitDims(resolution=d['res'], patch=d['patch'], width=d['width'],
                           layers=d['depth'], heads=d['heads'], hidden=d['hidden'],
                           eps=vitref.EPS)
        ctx = hip.VitContext(dims, sd, DEVICE)
        tag = f'vit.case{index}'
        for n in (1, 3):
            x = vitref.images(d, n, seed=200 + index).float()
            taps, cls = ctx.run(x, range(d['depth']), True)
            deepest, _ = ctx.run(x, [d['depth'] - 1])
            print(tag, f'n={n} taps', ' '.join(dg(taps[t]) for t in sorted(taps)), 'cls', dg(cls),
                  'deepest alone', dg(deepest[d['depth'] - 1]))
        print(tag, 'workspace',
              *[int(ctx.lib.milan_vit_workspace_bytes(ctx._h, n)) for n in (1, 3, 200)])
        ctx.close()
    for seqs, T, heads, hd in ((2, 1, 2, 16), (2, 33, 1, 48), (1, 130, 2, 64)):
        g = torch.Generator().manual_seed(T)
        qkv = torch.randn(seqs, T, 3 * heads * hd, generator=g).to(DEVICE)
        print(f'attention seqs={seqs} T={T} heads={heads} hd={hd}', dg(hip.attention(qkv, heads)))


def main():
    hip.require_device(DEVICE)
    bert_cases()
    clip_cases()
    vit_cases()
    torch.cuda.synchronize()
    print('done')


if __name__ == '__main__':
    main()
