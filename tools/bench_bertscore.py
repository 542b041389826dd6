"""Throughput of BERTScore at the true roberta-large dims (24 layers of which 17
run, width 1024, 16 heads, intermediate 4096, vocabulary 50265) with seeded
random weights, on a MILAN-shaped workload: one caption of 3 to 15 words and 3
annotations per neuron.  Sentence pairs per second of

  (a) `milan_amd.bertscore.BERTScorer.score` (csrc/bert.hip: ragged rows, every
      distinct sentence encoded once), and
  (b) the same `transformers.RobertaModel`, cut to 17 layers, run by PyTorch in
      fp32 on the same GPU with bert_score's batching: the distinct sentences
      sorted by length, padded to the longest of each batch of `--batch`, then
      the padded greedy matching (bmm, masked maxima, idf-weighted sums) in
      batches of pairs.

    python tools/bench_bertscore.py [--neurons 2000] [--batch 64] [--steps 5]

Prints the device clocks read before the run and one JSON line.  Medians over
`--steps` timed calls after `--warmup` untimed ones, wall clock around a
synchronised call (both sides include their host work: tokenising, batching).
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO / 'tests'),
                str(REPO / 'tests' / 'golden')]

import bert_standin  # noqa: E402
from milan_amd import bertscore  # noqa: E402

CFG = dict(bert_standin.CONFIGS['roberta'], width=1024, heads=16, layers=24, num_layers=17,
           intermediate=4096, max_positions=514, type_vocab=1)
VOCAB = 50265


def clocks():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True,
                             timeout=30).stdout
    except (OSError, subprocess.TimeoutExpired):
        return 'rocm-smi not available'
    lines = [l.split(':', 1)[-1].strip() for l in out.splitlines()
             if 'GPU[0]' in l and ('sclk' in l or 'mclk' in l)]
    return '; '.join(lines) or 'no clock lines'


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - start)
    return statistics.median(times)


def torch_scorer(model, tok, special, weight_of, batch):
    """bert_score's padded batching on torch: -> fn(cands, refs) -> (pairs, 3)."""

    def encode(sentences):
        ids = {s: tok.encode(s).ids for s in sentences}
        order = sorted(sentences, key=lambda s: -len(ids[s]))
        table = {}
        for lo in range(0, len(order), batch):
            chunk = order[lo:lo + batch]
            longest = len(ids[chunk[0]])
            padded = torch.full((len(chunk), longest), special['pad_id'], dtype=torch.long)
            mask = torch.zeros(len(chunk), longest, dtype=torch.long)
            for row, s in enumerate(chunk):
                padded[row, :len(ids[s])] = torch.tensor(ids[s])
                mask[row, :len(ids[s])] = 1
            with torch.no_grad():
                out = model(input_ids=padded.cuda(),
                            attention_mask=mask.cuda()).last_hidden_state
            for row, s in enumerate(chunk):
                emb = out[row, :len(ids[s])]
                table[s] = (emb / emb.norm(dim=-1, keepdim=True),
                            torch.tensor([weight_of(t) for t in ids[s]]).cuda())
        return table

    def score(cands, refs):
        pairs = [(c, r) for c, rs in zip(cands, refs) for r in rs]
        table = encode(list(dict.fromkeys([c for c, _ in pairs] + [r for _, r in pairs])))
        pad = torch.nn.utils.rnn.pad_sequence
        out = []
        for lo in range(0, len(pairs), batch):
            chunk = pairs[lo:lo + batch]
            c = pad([table[a][0] for a, _ in chunk], batch_first=True)
            r = pad([table[b][0] for _, b in chunk], batch_first=True)
            wc = pad([table[a][1] for a, _ in chunk], batch_first=True)
            wr = pad([table[b][1] for _, b in chunk], batch_first=True)
            mc = pad([torch.ones(len(table[a][1])) for a, _ in chunk], batch_first=True).cuda()
            mr = pad([torch.ones(len(table[b][1])) for _, b in chunk], batch_first=True).cuda()
            sim = torch.bmm(c, r.transpose(1, 2)) * (mc[:, :, None] * mr[:, None, :])
            p = (sim.max(dim=2).values * wc / wc.sum(1, keepdim=True)).sum(1)
            rr = (sim.max(dim=1).values * wr / wr.sum(1, keepdim=True)).sum(1)
            out.append(torch.stack([p, rr, 2 * p * rr / (p + rr)], 1))
        return torch.cat(out).cpu()

    return score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--neurons', type=int, default=2000)
    ap.add_argument('--annotations', type=int, default=3)
    ap.add_argument('--words', type=int, default=2000)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    print('clocks before the run:', clocks(), flush=True)
    words = tuple(f'w{i}' for i in range(args.words))
    g = torch.Generator().manual_seed(0)
    cands = bert_standin.sentences(g, args.neurons, 15, words, shortest=3)
    refs = [bert_standin.sentences(g, args.annotations, 15, words, shortest=3)
            for _ in cands]
    flat = [r for rs in refs for r in rs]
    sd = bert_standin.state_dict(CFG, 0, vocab_size=VOCAB, std=.02)
    tok = bert_standin.tokenizer(CFG, words)
    special = bert_standin.ids_of(CFG, words)
    scorer = bertscore.BERTScorer(sd, tok, num_layers=CFG['num_layers'], heads=CFG['heads'],
                                  idf=True, idf_sents=flat, device='cuda', **special)
    pairs = len(flat)
    unique = len(set(cands + flat))
    tokens = sum(len(scorer.tokens(s)) for s in set(cands + flat))
    result = dict(neurons=args.neurons, pairs=pairs, distinct_sentences=unique,
                  distinct_tokens=tokens, batch=args.batch)
    hip_s = timed(lambda: scorer.score(cands, refs, batch_size=args.batch), args.steps,
                  args.warmup)
    result.update(hip_seconds=hip_s, hip_pairs_per_s=pairs / hip_s)
    if not args.no_torch:
        import transformers
        config = transformers.RobertaConfig(
            vocab_size=VOCAB, hidden_size=CFG['width'], num_hidden_layers=CFG['layers'],
            num_attention_heads=CFG['heads'], intermediate_size=CFG['intermediate'],
            max_position_embeddings=CFG['max_positions'], type_vocab_size=CFG['type_vocab'],
            layer_norm_eps=CFG['eps'], hidden_dropout_prob=0., attention_probs_dropout_prob=0.,
            pad_token_id=special['pad_id'])
        model = transformers.RobertaModel(config, add_pooling_layer=False)
        own = {k: v for k, v in bert_standin.strip(sd).items() if not k.startswith('pooler.')}
        model.load_state_dict(own, strict=False)
        model.encoder.layer = model.encoder.layer[:CFG['num_layers']]
        model = model.eval().cuda()
        fn = torch_scorer(model, tok, special, scorer.token_weight, args.batch)
        torch_s = timed(lambda: fn(cands, refs), args.steps, args.warmup)
        # the two sides agree (per pair, before the maximum over references)
        mine = torch.stack(scorer.score([c for c, rs in zip(cands[:50], refs) for _ in rs],
                                        [r for rs in refs[:50] for r in rs],
                                        batch_size=args.batch), 1)
        theirs = fn(cands[:50], refs[:50])
        result.update(torch_seconds=torch_s, torch_pairs_per_s=pairs / torch_s,
                      hip_over_torch=torch_s / hip_s,
                      max_abs_difference=(mine - theirs).abs().max().item())
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
