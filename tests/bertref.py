"""A BERT-family encoder over ragged sentences and the BERTScore matching of
bert_score 0.3.11 as plain functions of a HuggingFace state dict (model prefix
stripped), in whatever dtype the state dict has: float64 gives the yardstick
the GPU tests measure errors against, float32 the error that sets their bound
(the clipref.py pattern).  The tower is pinned to `transformers` by
tests/test_bertscore_ref_vs_transformers.py.  Written from the algorithm's
description, independently of milan_amd/bertscore.py; sentences are lists of
token ids with the specials in place.
"""
import math

import torch
from torch.nn import functional as F


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}


def _linear(x, sd, name):
    return x @ sd[name + '.weight'].T + sd[name + '.bias']


def _ln(x, sd, name, eps):
    return F.layer_norm(x, x.shape[-1:], sd[name + '.weight'], sd[name + '.bias'], eps)


def encode_one(sd, ids, heads, num_layers, position_offset, eps):
    """(T, W) last hidden state of the first `num_layers` layers for one sentence."""
    ids = torch.as_tensor(ids, dtype=torch.long)
    t = len(ids)
    x = sd['embeddings.word_embeddings.weight'][ids]
    x = x + sd['embeddings.token_type_embeddings.weight'][0]
    x = x + sd['embeddings.position_embeddings.weight'][position_offset:position_offset + t]
    x = _ln(x, sd, 'embeddings.LayerNorm', eps)
    w = x.shape[-1]
    hd = w // heads
    for layer in range(num_layers):
        p = f'encoder.layer.{layer}.'
        q, k, v = (_linear(x, sd, p + 'attention.self.' + n).view(t, heads, hd).transpose(0, 1)
                   for n in ('query', 'key', 'value'))
        att = (q @ k.transpose(-2, -1) / math.sqrt(hd)).softmax(dim=-1)
        ctx = (att @ v).transpose(0, 1).reshape(t, w)
        x = _ln(_linear(ctx, sd, p + 'attention.output.dense') + x, sd,
                p + 'attention.output.LayerNorm', eps)
        h = _linear(x, sd, p + 'intermediate.dense')
        h = h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = _ln(_linear(h, sd, p + 'output.dense') + x, sd, p + 'output.LayerNorm', eps)
    return x


def encode(sd, sentences, **cfg):
    return [encode_one(sd, ids, **cfg) for ids in sentences]


def idf_weights(reference_sentences, cls, sep, idf=True):
    """-> function id -> weight.  idf: log((N + 1) / (df + 1)) with df over the id SETS of the
    N reference sentences (specials included, so cls and sep get 0), log(N + 1) for unseen
    ids; not idf: 1, and 0 for cls and sep."""
    if not idf:
        return lambda t: 0. if t in (cls, sep) else 1.
    n = len(reference_sentences)
    df = {}
    for ids in reference_sentences:
        for t in set(int(i) for i in ids):
            df[t] = df.get(t, 0) + 1
    return lambda t: math.log((n + 1) / (df.get(int(t), 0) + 1))


def pair(c, r, wc, wr):
    """P, R, F and the smallest best-match cosine of one (candidate, reference) pair.  c, r:
    (T, W) embeddings; wc, wr: (T,) weights."""
    if len(c) <= 2 or len(r) <= 2:
        z = torch.zeros((), dtype=c.dtype)
        return z, z, z, None
    c = c / c.norm(dim=-1, keepdim=True)
    r = r / r.norm(dim=-1, keepdim=True)
    sim = c @ r.T
    p_i, r_j = sim.max(dim=1).values, sim.max(dim=0).values
    wc, wr = wc / wc.sum(), wr / wr.sum()
    p, rr = (wc * p_i).sum(), (wr * r_j).sum()
    f = 2 * p * rr / (p + rr)
    if torch.isnan(f):
        f = torch.zeros((), dtype=c.dtype)
    return p, rr, f, min(float(p_i.min()), float(r_j.min()))


def bert_score(sd, cands, refs, weight_of, baseline=None, **cfg):
    """cands: token-id lists; refs: per candidate a list of token-id lists.  -> (P, R, F)
    tensors of len(cands) in sd's dtype, and the smallest best-match cosine met (None when
    every pair had an empty side)."""
    dtype = sd['embeddings.LayerNorm.weight'].dtype
    cache = {}

    def emb(ids):
        key = tuple(int(i) for i in ids)
        if key not in cache:
            cache[key] = (encode_one(sd, key, **cfg),
                          torch.tensor([weight_of(t) for t in key], dtype=dtype))
        return cache[key]

    out, lowest = [], None
    for cand, cand_refs in zip(cands, refs):
        c, wc = emb(cand)
        best = None
        for ref in cand_refs:
            r, wr = emb(ref)
            p, rr, f, low = pair(c, r, wc, wr)
            prf = torch.stack([p, rr, f])
            best = prf if best is None else torch.maximum(best, prf)
            if low is not None:
                lowest = low if lowest is None else min(lowest, low)
        out.append(best)
    out = torch.stack(out)
    if baseline is not None:
        b = torch.tensor(baseline, dtype=dtype)
        out = (out - b) / (1 - b)
    return out[:, 0], out[:, 1], out[:, 2], lowest
