"""Throughput of the CLIP reranker at ViT-B/32 dims with seeded random weights:
neurons per second of the rerank alone (k = 15 images of 224 x 224, `beam`
captions per neuron), with the causal truncation on and off, against the same
model (tests/golden/clip_standin.py) run by PyTorch on the same GPU.

    python tools/bench_clip_rerank.py [--neurons 8] [--beam 50 100] [--steps 5]

`decoder_with_clip_neurons_per_s` times `DecoderWithCLIP.forward` (resnet101 pyramid encoder,
vocabulary 5004, random weights, uint8 exemplars: encode + beam search + tokenise + rerank)
and `decoder_beam_neurons_per_s` the same call without the reranker.  The PyTorch baseline
runs the stand-in's unmasked image tower twice (it has no masked variant) and its text
tower over all 77 positions, in fp32 through torch's default GEMM library.

Prints one JSON line per configuration.  Medians over `--steps` timed calls after
`--warmup` untimed ones, timed with device events on the stream of the work.
"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO / 'tests'),
                str(REPO / 'tests' / 'golden')]

import clip_standin  # noqa: E402
from milan_amd import decoders, encoders, lang, rerankers, synthetic  # noqa: E402

DIMS = dict(resolution=224, patch=32, vision_width=768, vision_layers=12, vision_heads=12,
            embed_dim=512, context_length=77, vocab_size=49408, text_width=512, text_layers=12,
            text_heads=8)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        start, stop = torch.cuda.Event(True), torch.cuda.Event(True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--neurons', type=int, default=8)
    ap.add_argument('--k', type=int, default=15)
    ap.add_argument('--beam', type=int, nargs='+', default=[50, 100])
    ap.add_argument('--length', type=int, default=15)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    clip_standin.configure(seed=0, **DIMS)
    model = clip_standin.load()[0]
    g = torch.Generator().manual_seed(0)
    n, k = args.neurons, args.k
    images = torch.randn(n, k, 3, 224, 224, generator=g).cuda()
    masks = torch.rand(n, k, 1, 224, 224, generator=g).cuda()
    r = rerankers.reranker(lam=.5, weights=model.state_dict())
    indexer = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(5000)), None, True, True, True,
                           True, args.length)
    full = decoders.DecoderWithCLIP(
        indexer, encoders.PyramidConvEncoder('resnet101', pretrained=False),
        length=args.length,
        reranker_kwargs=dict(weights=model.state_dict(), tokenize=clip_standin.tokenize, lam=.5))
    full.reset_parameters()
    full = full.to('cuda')
    u8_images, u8_masks = synthetic.exemplars(n, k=k, size=224, seed=1)
    u8_images, u8_masks = u8_images.cuda(), u8_masks.cuda()
    torch_model = None if args.no_torch else model.cuda()
    for beam in args.beam:
        tokens = torch.zeros(n, beam, 77, dtype=torch.long)
        lengths = torch.randint(3, args.length + 1, (n, beam), generator=g)
        for i in range(n):
            for j in range(beam):
                m = int(lengths[i, j])
                tokens[i, j, 0] = 49406
                tokens[i, j, 1:1 + m] = torch.randint(1, 49000, (m,), generator=g)
                tokens[i, j, 1 + m] = 49407
        ids = [t.cuda() for t in tokens]
        row = dict(neurons=n, k=k, beam=beam, device=torch.cuda.get_device_name(0))
        for name, truncate in (('hip', True), ('hip_full_context', False)):
            r.clip_with_masks.truncate_text = truncate
            t = timed(lambda: r.similarities(images, masks, ids), args.steps, args.warmup)
            row[name + '_neurons_per_s'] = n / t
        r.clip_with_masks.truncate_text = True
        t = timed(lambda: full(u8_images, u8_masks, beam_size=beam), args.steps, args.warmup)
        row['decoder_with_clip_neurons_per_s'] = n / t
        t = timed(lambda: decoders.Decoder.forward(full, u8_images, u8_masks, strategy='beam',
                                                   beam_size=beam), args.steps, args.warmup)
        row['decoder_beam_neurons_per_s'] = n / t
        if torch_model is not None:
            flat = images.view(n * k, 3, 224, 224)

            def eager():
                with torch.no_grad():
                    # the unmasked pass twice stands in for masked + unmasked
                    a = torch_model.encode_image(flat)
                    b = torch_model.encode_image(flat)
                    t = torch_model.encode_text(tokens.view(-1, 77).cuda())
                    return a, b, t

            row['torch_standin_neurons_per_s'] = n / timed(eager, args.steps, args.warmup)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
