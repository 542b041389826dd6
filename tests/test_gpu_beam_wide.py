"""Wide beam search (125 <= beam_size <= 1024).

A  the merge kernel alone, bit for bit against a stable CPU sort;
B  the wide kernels forced at narrow beams against the shipped path, end to end,
   bit for bit (the shipped path is pinned by goldens G14);
C  wide beams against the oracle: the SET of beams, the sorted scores, every beam
   re-scored by teacher forcing, distinctness, T';
D  ties by construction; E rerank at a wide beam; F DecoderWithCLIP at its default
   beam_size=1000; G limits; H graph replay.

C takes no near-tie excuses, so its inputs are admitted by a rule that looks at the
oracle alone: the fp32 oracle's smallest selection margin must be at least ten times
the largest difference between the fp32 and the float64 oracle's beam scores on
that case.  Both numbers are computed here; a (case, seed) that fails the rule is
an assertion error, not a skip.
"""
import functools
import json
import pathlib
import sys

import pytest
import torch

import beamcheck
from milan_amd import hip, synthetic
from oracle import milan_oracle as O

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min
RTOL, ATOL = 1e-4, beamcheck.ATOL


def state_dict(nv, seed):
    return synthetic.decoder_state_dict(nv + 4, feature_size=244, hidden_size=64,
                                        embedding_size=16, lm_hidden_size=64,
                                        lm_embedding_size=16, seed=seed)


def context(sd, nv):
    return hip.Context(hip.make_dims(sd, nv), sd, 'cuda')


# ---- A: the merge alone -------------------------------------------------------
def merge_inputs(kind, n, beam_prev, beam, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (n, beam_prev, beam)
    cand_i = torch.randint(0, 5000, shape, generator=g, dtype=torch.int32)
    if kind == 'random':
        cand_v = 0. - torch.rand(shape, generator=g).cumsum(-1)
        last_lp = 0. - 8 * torch.rand(n, beam_prev, generator=g)
    elif kind == 'quantised':  # multiples of 0.25: sums tie exactly, across the k-th value too
        cand_v = 0. - torch.randint(0, 3, shape, generator=g).cumsum(-1) * .25
        last_lp = 0. - torch.randint(0, 8, (n, beam_prev), generator=g) * .25
    elif kind == 'finished':   # allennlp's forced lists of finished parents among live ones
        cand_v = 0. - torch.rand(shape, generator=g).cumsum(-1)
        done = torch.rand(n, beam_prev, generator=g) < .5
        done[0] = True         # one neuron whose beams have all finished
        forced = torch.full((beam,), FMIN)
        forced[0] = 0.
        cand_v[done] = forced
        last_lp = 0. - 8 * torch.rand(n, beam_prev, generator=g)
    else:                      # everything equal
        cand_v = torch.full(shape, -1.5)
        last_lp = torch.full((n, beam_prev), -2.)
    assert bool((cand_v[..., :-1] >= cand_v[..., 1:]).all())
    return cand_v.float(), cand_i, last_lp.float()


def merge_expected(cand_v, cand_i, last_lp):
    n, beam_prev, beam = cand_v.shape
    summed = (cand_v + last_lp[:, :, None]).reshape(n, -1)  # the kernel's fp32 addition
    values, index = torch.sort(summed, dim=1, descending=True, stable=True)
    values, index = values[:, :beam], index[:, :beam]
    tok = cand_i.reshape(n, -1).gather(1, index)
    return values, tok, (index // beam).int()


KINDS = ('random', 'quantised', 'finished', 'equal')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,beam_prev,beam', [(3, 1, 126), (3, 1, 1000), (2, 126, 126),
                                              (2, 257, 257), (1, 1000, 1000),
                                              (1, 1024, 1024)])
def test_merge_is_bit_exact(n, beam_prev, beam, kind):
    cand_v, cand_i, last_lp = merge_inputs(kind, n, beam_prev, beam, seed=beam + beam_prev)
    want = merge_expected(cand_v, cand_i, last_lp)
    got = hip.beam_merge(cand_v.cuda(), cand_i.cuda(), last_lp.cuda())
    for name, g, w in zip(('new_lp', 'new_tok', 'new_bp'), got, want):
        assert torch.equal(g.cpu(), w), (name, kind)
    if beam_prev == 1:  # the first step of a search passes no running scores
        zero = torch.zeros_like(last_lp)
        want = merge_expected(cand_v, cand_i, zero)
        got = hip.beam_merge(cand_v.cuda(), cand_i.cuda(), None)
        for g, w in zip(got, want):
            assert torch.equal(g.cpu(), w), kind


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,beam_prev,beam', [(4, 50, 50), (4, 124, 124), (4, 125, 125),
                                              (4, 1, 7)])
def test_forced_wide_merge_equals_the_narrow_kernel(n, beam_prev, beam, kind):
    # (124 is the widest beam whose candidates fit the narrow kernel's LDS; at 125 `wide=0`
    # already picks the wide kernel, and both are held to the CPU sort)
    cand_v, cand_i, last_lp = merge_inputs(kind, n, beam_prev, beam, seed=beam)
    args = (cand_v.cuda(), cand_i.cuda(), last_lp.cuda())
    narrow, wide = hip.beam_merge(*args, wide=False), hip.beam_merge(*args, wide=True)
    for g, w, e in zip(wide, narrow, merge_expected(cand_v, cand_i, last_lp)):
        assert torch.equal(g, w) and torch.equal(g.cpu(), e), kind


def test_merge_rejects_beams_above_the_limit():
    cand_v, cand_i, last_lp = merge_inputs('random', 1, 1, 1025, seed=1)
    with pytest.raises(ValueError, match='beam_size='):
        hip.beam_merge(cand_v.cuda(), cand_i.cuda(), last_lp.cuda())


# ---- B: forced-wide equals the shipped path -------------------------------------
OUTPUTS = ('beam_tokens', 'beam_scores', 'tokens', 'scores', 'out_len')


@functools.lru_cache(maxsize=None)
def narrow_case(nv):
    sd = state_dict(nv, seed=nv)
    feats = torch.rand(3, 5, 244, generator=torch.Generator().manual_seed(nv + 1))
    return sd, feats.cuda()


@pytest.mark.parametrize('beam', [2, 7, 50, 124, 125])
@pytest.mark.parametrize('nv', [40, 1000])
def test_forced_wide_path_equals_the_shipped_path_bitwise(nv, beam):
    sd, feats = narrow_case(nv)
    ctx = context(sd, nv)
    assert ctx.beam_path == 0
    runs = 0
    for precision in ('f32', 'split_f16'):
        ctx.set_precision(precision)
        for strategy, mi in ((hip.BEAM, False), (hip.BEAM, True), (hip.RERANK, False)):
            outs = []
            for path in (0, 1):
                ctx.set_beam_path(path)
                assert ctx.beam_path == path
                if beam > nv + 4:  # no such search exists: both paths say so
                    with pytest.raises(ValueError, match='beam_size='):
                        ctx.decode(feats, strategy, 5, beam, mi, 0.2)
                    continue
                outs.append(ctx.decode(feats, strategy, 5, beam, mi, 0.2))
            if outs:
                runs += 1
                for key in OUTPUTS:
                    assert torch.equal(outs[0][key], outs[1][key]), (key, precision, strategy, mi)
    assert runs == (6 if beam <= nv + 4 else 0)
    ctx.close()


# ---- C: wide beams against the oracle --------------------------------------------
def stop_biased(sd, nv, bias):
    sd = {k: v.clone() for k, v in sd.items()}
    sd['output.1.bias'][nv + 1] += bias
    return sd


@functools.lru_cache(maxsize=None)
def oracle_case(nv, beam, length, mi, seed, stop_bias=0.):
    """The fp32 oracle's search, its smallest selection margin and the largest beam-score
    difference to the float64 oracle; computed once per case."""
    sd = state_dict(nv, seed)
    if stop_bias:
        sd = stop_biased(sd, nv, stop_bias)
    feats = torch.rand(3, 5, 244, generator=torch.Generator().manual_seed(seed))
    margins = []
    tokens, scores = O.beam_search(feats, sd, nv, nv + 1, length, beam, mi, 0.2,
                                   margins=margins)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, scores64 = O.beam_search(feats.double(), sd64, nv, nv + 1, length, beam, mi, 0.2)
    margin = float(margins[0].min())
    diff = float((scores.double() - scores64).abs().max())
    return sd, feats, tokens, scores, margin, diff


def rescore(feats, sd, nv, tokens, mi):
    """Score of every beam under teacher forcing, with allennlp's rule for finished
    beams: nothing is added after the first <stop>."""
    n, beam, length = tokens.shape
    rows = tokens.reshape(n * beam, length)
    out = O.teacher_forced(feats.repeat_interleave(beam, 0), sd, nv, rows, mi=mi,
                           temperature=0.2)
    picked = out.predictions.gather(2, rows.unsqueeze(-1)).squeeze(-1)
    stopped = (rows == nv + 1).long().cumsum(1) - (rows == nv + 1).long()  # stops before t
    return (picked * (stopped == 0)).sum(1).reshape(n, beam)


def check_against_oracle(nv, beam, length, mi, seed, stop_bias=0., precision='f32',
                         min_finished=0.):
    sd, feats, want_t, want_s, margin, diff = oracle_case(nv, beam, length, mi, seed,
                                                          stop_bias)
    print(f'nv={nv} beam={beam} length={length} mi={mi} seed={seed}: oracle margin '
          f'{margin:.3g}, fp32-vs-float64 oracle score difference {diff:.3g}')
    assert margin >= 10 * diff, (
        f'seed {seed} is too close to a tie for a test without excuses (margin '
        f'{margin:.3g} < 10 x {diff:.3g}): pick another seed')
    stop = nv + 1
    finished = float((want_t == stop).any(-1).float().mean())
    assert finished >= min_finished, f'only {finished:.2f} of the beams finish'
    ctx = context(sd, nv)
    ctx.set_precision(precision)
    out = ctx.decode(feats.cuda(), hip.BEAM, length, beam, mi, 0.2)
    ctx.close()
    tp = want_t.shape[2]
    bt, bs = out['beam_tokens'].cpu(), out['beam_scores'].cpu()
    assert int(out['out_len'][0]) == tp                                    # 6
    assert bool((bt[:, :, tp:] == stop).all())
    bt = bt[:, :, :tp]
    assert bool((bs[:, :-1] >= bs[:, 1:]).all())                           # 1
    print('  max |sorted score - oracle|', float((bs - want_s).abs().max()))
    for i in range(len(bt)):
        got = {tuple(r.tolist()) for r in bt[i]}
        assert len(got) == beam, f'neuron {i}: beams repeat'               # 5
        want = {tuple(r.tolist()) for r in want_t[i]}
        assert got == want, (                                              # 2
            f'neuron {i}: {len(want - got)} beams of the oracle are missing '
            f'(margin {margin:.3g}, oracle difference {diff:.3g})')
    torch.testing.assert_close(bs, want_s, rtol=RTOL, atol=ATOL)           # 3
    torch.testing.assert_close(bs, rescore(feats, sd, nv, bt, mi), rtol=RTOL,
                               atol=ATOL)                                  # 4


WIDE_CASES = [
    # nv, beam, length, mi, seed
    (1100, 1000, 3, False, 3), (1100, 1000, 3, False, 5),
    (1100, 1024, 3, False, 5),
    (1100, 1000, 3, True, 3),
    (300, 257, 4, False, 1), (300, 257, 4, False, 3), (300, 257, 4, False, 5),
    (300, 257, 4, False, 6),
    (300, 256, 4, True, 1), (300, 256, 4, True, 2), (300, 256, 4, True, 4),
    (300, 256, 4, True, 5), (300, 256, 4, True, 6),
    (200, 126, 5, False, 1), (200, 126, 5, False, 2), (200, 126, 5, False, 3),
    (200, 126, 5, False, 4), (200, 126, 5, False, 5), (200, 126, 5, False, 6),
    (600, 600, 3, False, 3), (600, 600, 3, False, 4),   # beam nearly the vocabulary
]


@pytest.mark.parametrize('nv,beam,length,mi,seed', WIDE_CASES)
def test_wide_beam_matches_the_oracle(nv, beam, length, mi, seed):
    check_against_oracle(nv, beam, length, mi, seed)


# a positive bias on <stop>: a third or more of the beams finish inside the search
# (chosen by the rule above among seeds 1-8 and biases 0.5-4: oracle margin 9.9e-5, oracle
# difference 3.0e-6, half of the beams finished and T' still 4)
STOP_CASE = dict(nv=300, beam=257, length=4, mi=False, seed=5, stop_bias=1.5)


def test_wide_beam_with_many_finished_beams_matches_the_oracle():
    check_against_oracle(min_finished=1 / 3, **STOP_CASE)


def test_wide_beam_in_split_f16_matches_the_oracle():
    check_against_oracle(300, 257, 4, False, 1, precision='split_f16')


# ---- D: ties by construction -----------------------------------------------------
@pytest.mark.parametrize('beam', [300, 1000])
def test_all_equal_logits_pick_lowest_indices_at_wide_beams(beam):
    nv = 1100
    sd = state_dict(nv, seed=3)
    sd['output.1.weight'].zero_()
    sd['output.1.bias'].zero_()
    ctx = context(sd, nv)
    out = ctx.decode(torch.rand(3, 5, 244).cuda(), hip.BEAM, 3, beam, False, 0.2)
    ctx.close()
    # every candidate ties at every step: step 0 keeps classes 0..beam-1, then each merge
    # keeps the candidates of beam 0 => beam j reads [0, 0, j]
    bt = out['beam_tokens'].cpu()
    assert bt[:, :, 0].eq(0).all() and bt[:, :, 1].eq(0).all()
    assert bt[:, :, 2].eq(torch.arange(beam)).all()


@pytest.mark.parametrize('nv', [5000, 6200])   # register kernel, LDS kernel (V > 6144)
@pytest.mark.parametrize('group,k', [(30, 300), (7, 1000), (700, 1000)])
def test_runs_of_equal_logits_straddling_the_kth_value_at_wide_k(group, k, nv):
    """Row-independent logits in runs of `group` equal values: the top-k is exactly
    token ids 0..k-1 in order -- the k-th value's run is cut at its lowest indices."""
    sd = state_dict(nv, seed=9)
    sd['output.1.weight'].zero_()
    sd['output.1.bias'].copy_(-(torch.arange(nv + 4) // group).float() * 0.25)
    ctx = context(sd, nv)
    feats = torch.rand(2, 5, 244).cuda()
    for precision in ('f32', 'split_f16'):
        ctx.set_precision(precision)
        out = ctx.decode(feats, hip.BEAM, 1, k, False, 0.2)
        bt = out['beam_tokens'].cpu()[:, :, 0]
        assert bt.eq(torch.arange(k)).all(), (precision, bt[0])
        want = torch.log_softmax(sd['output.1.bias'], 0)[:k]
        torch.testing.assert_close(out['beam_scores'].cpu(), want.expand(2, k),
                                   rtol=1e-5, atol=1e-5)
    ctx.close()


# ---- E: rerank at a wide beam ------------------------------------------------------
def test_rerank_at_a_wide_beam_matches_the_oracle_on_the_gpu_beams():
    nv, beam, length = 600, 300, 3
    sd = state_dict(nv, seed=4)
    feats = torch.rand(3, 5, 244, generator=torch.Generator().manual_seed(4))
    ctx = context(sd, nv)
    out = ctx.decode(feats.cuda(), hip.RERANK, length, beam, False, 0.2)
    ctx.close()
    tp = int(out['out_len'][0])
    bt, bs = out['beam_tokens'].cpu()[:, :, :tp], out['beam_scores'].cpu()
    want_t, want_s, choice = O.rerank(bt, bs, sd, nv, nv + 1, 0.2)
    seqs = torch.cat([bt.new_full((3, beam, 1), nv), bt], -1).view(3 * beam, -1)
    pmi = bs - 0.2 * O.lm_score(seqs, sd, nv + 1).view(3, beam)
    top2 = pmi.topk(2, dim=-1).values
    tokens, scores = out['tokens'].cpu()[:, :tp], out['scores'].cpu()
    excuses = 0
    for i in range(3):
        row = [j for j in range(beam) if torch.equal(bt[i, j], tokens[i])]
        assert len(row) == 1, f'neuron {i}: tokens are not one of its beams'
        torch.testing.assert_close(scores[i], pmi[i, row[0]], rtol=RTOL, atol=ATOL + 1e-3)
        if row[0] != int(choice[i]):
            assert float(top2[i, 0] - top2[i, 1]) < beamcheck.TIE, (
                f'neuron {i}: chose beam {row[0]}, the oracle {int(choice[i])}')
            excuses += 1
    assert excuses <= 1


# ---- F: DecoderWithCLIP at its default beam_size -------------------------------------
def test_decoder_with_clip_runs_at_its_default_beam_size():
    import clipref
    from milan_amd import decoders, encoders, lang
    golden = pathlib.Path(__file__).resolve().parent / 'golden'
    sys.path.insert(0, str(golden))
    import clip_standin
    meta = json.loads((golden / 'reference_goldens_clip.json').read_text())
    tensors = torch.load(golden / 'reference_goldens_clip.pt', weights_only=True)
    case = meta['decoder']
    dims = meta['configs'][case['config']]
    clip_standin.configure(**dims)

    class PoolEncoder(encoders.Encoder):

        def __init__(self):
            super().__init__()
            self.feature_shape = (clipref.POOL_FEATURES,)

        def forward(self, images, masks=None, **_):
            return clipref.pool_features(images, masks)

        def properties(self):
            return {}

    nvocab, length = 1000, 3
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(nvocab)), None, True, True, True,
                       True, length)
    model = decoders.DecoderWithCLIP(
        idx, PoolEncoder(), embedding_size=case['emb'], hidden_size=case['hidden'],
        length=length,
        reranker_kwargs=dict(weights=tensors['weights/' + case['config']],
                             tokenize=clip_standin.tokenize, lam=case['lam'],
                             vision_heads=dims['vision_heads'],
                             text_heads=dims['text_heads']))
    assert model.beam_size == 1000 and model.properties()['beam_size'] == 1000
    sd = synthetic.decoder_state_dict(len(idx), feature_size=clipref.POOL_FEATURES,
                                      hidden_size=case['hidden'],
                                      embedding_size=case['emb'], lm=False, seed=7)
    result = model.load_state_dict(sd, strict=False)
    assert not result.unexpected_keys and not result.missing_keys, result
    model.precision = 'f32'
    model = model.to('cuda')
    images, masks, _ = clipref.synthetic_inputs(dims, 2, case['k'], [1, 1], 'random', 5)
    images, masks = images.cuda(), masks.cuda()
    out = model(images, masks)
    assert out.beam_tokens.shape == (2, 1000, length)
    plain = decoders.Decoder.forward(model, images, masks=masks, strategy='beam',
                                     beam_size=1000)
    assert torch.equal(plain.beam_tokens, out.beam_tokens)
    assert torch.equal(plain.beam_scores, out.beam_scores)
    ranked = model.reranker(images, masks, [list(c) for c in plain.beam_captions])
    assert out.captions == tuple(r[0] for r in ranked.texts)
    for n, order in enumerate(ranked.orders):
        assert torch.equal(out.scores[n], plain.beam_scores[n, order[0]])
        assert torch.equal(out.tokens[n], plain.beam_tokens[n, order[0]])


# ---- G: limits -----------------------------------------------------------------------
def test_beam_size_limits():
    sd = state_dict(1100, seed=2)
    ctx = context(sd, 1100)
    feats = torch.rand(2, 5, 244).cuda()
    with pytest.raises(ValueError, match='beam_size='):
        ctx.decode(feats, hip.BEAM, 3, 1025, False, 0.2)
    ctx.decode(feats, hip.BEAM, 2, 1024, False, 0.2)
    ctx.close()
    sd = state_dict(40, seed=2)
    ctx = context(sd, 40)
    with pytest.raises(ValueError, match=r'beam_size=1000 must be in 1\.\.vocab_size \(44\)'):
        ctx.decode(feats, hip.BEAM, 3, 1000, False, 0.2)
    with pytest.raises(ValueError, match=r'beam_size=45 must be in 1\.\.vocab_size \(44\)'):
        ctx.decode(feats, hip.BEAM, 3, 45, False, 0.2)
    ctx.close()


def test_unknown_beam_path_mode_is_rejected():
    ctx = context(state_dict(40, seed=2), 40)
    with pytest.raises(ValueError, match='beam path'):
        ctx.set_beam_path(2)
    assert ctx.beam_path == 0
    ctx.close()


def test_more_than_256_beams_need_a_vocabulary_the_wide_row_select_holds():
    """Above 36864 logits a row does not fit the wide per-row top-k's LDS; the k-rounds
    block argmax is no path to fall back to, so the call is refused."""
    nv = 37000
    ctx = context(state_dict(nv, seed=2), nv)
    with pytest.raises(ValueError, match=r'beam_size=300 above 256 needs vocab_size <= 36864'):
        ctx.decode(torch.rand(2, 5, 244).cuda(), hip.BEAM, 2, 300, False, 0.2)
    ctx.close()


@pytest.mark.parametrize('n,length', [(1 << 21, 3),      # n * beam_size = 2^31 rows
                                      (1 << 19, 1100)])  # rows * (length + 1) > 2^31 * 256
def test_row_counts_past_the_32_bit_limits_are_refused_before_any_launch(n, length):
    """The requirement comes before the workspace is planned or anything is launched, so
    the call can be made with token-sized buffers."""
    ctx = context(state_dict(1100, seed=2), 1100)
    buf = torch.zeros(4096, dtype=torch.int64, device='cuda')
    ws = torch.empty(1 << 16, dtype=torch.uint8, device='cuda')
    ptr = buf.data_ptr()
    with pytest.raises(ValueError, match='lower chunk_size or beam_size'):
        hip._check(ctx.lib.milan_decode(ctx._h, ptr, n, 5, hip.BEAM, length, 1024, 0, 0.2, 0,
                                        ptr, ptr, None, None, ptr, ptr, ptr, ws.data_ptr(),
                                        ws.numel(), hip._stream(ctx.device)))
    ctx.close()


def test_rows_past_16384_blocks_are_all_written():
    """The kernels that handle one element per thread (the LM input sequences, the
    back-trace, the column gathers) get a grid that covers every element:
    rows * (length + 1) = 4.23 M here, more than 16384 blocks of 256 threads.  A decode of
    all neurons equals the decodes of its two halves, bit for bit."""
    nv, beam, length, n = 40, 32, 31, 4128
    assert n * beam * (length + 1) > 16384 * 256
    ctx = context(state_dict(nv, seed=6), nv)
    feats = torch.rand(n, 1, 244, generator=torch.Generator().manual_seed(6)).cuda()
    run = lambda f: ctx.decode(f, hip.RERANK, length, beam, False, 0.2, group_size=16)  # noqa: E731
    whole = run(feats)
    parts = [run(feats[i:i + n // 2]) for i in (0, n // 2)]
    ctx.close()
    for key in OUTPUTS:
        assert torch.equal(whole[key], torch.cat([p[key] for p in parts])), key


# ---- H: graph replay -------------------------------------------------------------------
def test_wide_beam_graph_replay_is_bit_identical():
    nv, beam = 600, 300
    sd = state_dict(nv, seed=5)
    ctx = context(sd, nv)
    feats = torch.rand(2, 5, 244, generator=torch.Generator().manual_seed(5)).cuda()
    want = ctx.decode(feats, hip.RERANK, 4, beam, False, 0.2)
    ctx.enable_graphs(True)
    # call 1: direct, call 2: capture + launch, call 3: replay
    outs = [ctx.decode(feats, hip.RERANK, 4, beam, False, 0.2) for _ in range(3)]
    torch.cuda.synchronize()
    assert ctx.graph_stats() == (1, 2)
    for got in outs:
        for key in OUTPUTS:
            assert torch.equal(got[key], want[key]), key
    ctx.close()
