"""CPU: what tests/test_gpu_full_decoder.py relies on, shown without a GPU.

  1. decref's float64 reference, run in float32, is the oracle (`oracle/milan_oracle.py`).
  2. decref's case table reaches the tiles, epilogues and kernels it names.
  3. Conditioning: on every case the fp32 CPU oracle's error against float64 is at most a
     quarter of the bound, per quantity; the figures the bound was taken from are printed.
  4. The bound resolves the mutants: each, applied to the float64 reference through its
     hook, exceeds the bound at least tenfold.
  5. The beam cases: seeds with no near-tie at n <= 7, and the fp32 oracle itself within
     the excuse cap above.
  6. Off the unit operand scale (tests/test_gpu_decoder_range.py): `decref.rescaled` is
     exact under the fp32 oracle and under float64 at every scale used, so the bounds hold
     unchanged there; and a feature operand left with the absolute resolution of a
     subnormal `lo` exceeds them.
DESIGN.md sections 4.19 and 4.21."""
import functools

import pytest
import torch

import decref as D
from beamcheck import TIE
from oracle import milan_oracle as O

IDS = [D.case_id(c) for c in D.CASES]
SMALL = [c for c in D.CASES if c.geom != 'prod' and c.n <= 257]


def inputs(case):
    d = case.dims
    sd = D.weights(case.geom)
    feats = D.features(d, case.n, case.k)
    targets = D.forced_targets(d, case.n, D.forced_length(case))
    return d, sd, feats, targets


# ---- 1. the reference is the oracle -------------------------------------------------------
@pytest.mark.parametrize('case', SMALL, ids=[D.case_id(c) for c in SMALL])
def test_float32_reference_is_the_oracle(case):
    d, sd, feats, targets = inputs(case)
    start, _ = D.specials(d)
    for lm in (False, True):
        got, want = D.init_state(feats, sd, lm), O.init_state(feats, sd, lm)
        for g, w in zip(got, want):
            assert (g is None and w is None) or torch.equal(g, w)
        keys = D.project_keys(feats, sd)
        assert torch.equal(keys, O.project_keys(feats, sd))
        tok = D.edge_tokens(d, case.n)
        p, a, st = D.step(feats, keys, tok, got, sd)
        wp, wa, wst = O.step(feats, keys, tok, want, sd)
        assert torch.equal(p, wp) and torch.equal(a, wa)
        for g, w in zip(st, wst):
            assert (g is None and w is None) or torch.equal(g, w)
        # the hooked path (stages observed, nothing replaced) computes the same
        seen = []
        hp, ha, _ = D.step(feats, keys, tok, got, sd, hook=lambda n, v, e: seen.append(n))
        assert torch.equal(hp, p) and torch.equal(ha, a)
        assert seen[:4] == ['q', 'att', 'ctx', 'x'] and 'lse' in seen and seen[-1] == 'pred'
    for mi in (False, True):
        got = D.teacher_forced(feats, sd, start, targets, mi=mi)
        want = O.teacher_forced(feats, sd, start, targets, mi=mi)
        assert torch.equal(got.predictions, want.predictions)
        assert torch.equal(got.attentions, want.attentions)
        assert torch.equal(got.scores, want.scores)


@pytest.mark.parametrize('mi', [False, True])
@pytest.mark.parametrize('n,beam,length', [(7, 5, 4), (3, 1, 3), (5, 16, 6)])
def test_float32_search_is_the_oracle(n, beam, length, mi):
    d = D.GEOMETRIES['small']
    sd = D.weights('small')
    feats = D.features(d, n, 15, seed=3)
    start, stop = D.specials(d)
    margins = []
    wt, ws = O.beam_search(feats, sd, start, stop, length, beam, mi, D.TEMPERATURE, margins)
    got = D.beam_search(feats, sd, start, stop, length, beam, mi)
    assert torch.equal(got.tokens, wt) and torch.equal(got.scores, ws)
    assert torch.equal(got.margins, margins[0])
    # rescore, pinned to the search's own scores: in float64 both are the same sums
    sd64 = D.promote(sd)
    s64 = D.beam_search(feats.double(), sd64, start, stop, length, beam, mi)
    re = D.rescore(feats.double(), s64.tokens, sd64, start, stop, mi)
    assert float((re - s64.scores).abs().max()) < 1e-11
    # and in float32 against the oracle's beam scores, within the oracle's own error
    re32 = D.rescore(feats, wt, sd, start, stop, mi)
    assert float((re32 - ws).abs().max()) <= length * D.LOGP_CLASS / 4
    # lm_score, float32: the oracle's
    seqs = torch.cat([torch.full((n * beam, 1), start), wt.reshape(n * beam, -1)], 1)
    assert torch.equal(D.lm_score(seqs, sd, stop), O.lm_score(seqs, sd, stop))


def test_rescore_stops_at_stop():
    """Nothing is added after the first <stop>, whatever follows it."""
    d = D.GEOMETRIES['small']
    sd = D.promote(D.weights('small'))
    feats = D.features(d, 2, 15).double()
    start, stop = D.specials(d)
    toks = torch.tensor([[[5, stop, stop, stop], [5, stop, 9, 11]],
                         [[7, 8, 9, stop], [7, 8, 9, 10]]])
    re = D.rescore(feats, toks, sd, start, stop)
    assert float(re[0, 0]) == float(re[0, 1])
    short = D.rescore(feats, toks[:, :, :2], sd, start, stop)
    assert float(short[0, 0]) == float(re[0, 0])
    assert float(re[1, 0]) != float(re[1, 1])


# ---- 2. the table is what it says -----------------------------------------------------------
def test_case_table_reaches_what_it_names():
    G = D.GEOMETRIES
    rows = 257

    def tiles(geom, precision='split_f16'):
        return {g[0]: g for g in D.step_gemms(G[geom], rows, precision)}

    # prod: fused, every real tile
    assert D.fused(G['prod'])
    p = tiles('prod')
    assert p['lstm'][1:] == (rows, 2048, 4032 + 512, 4032, 'pp32_256', 'lstm')
    assert p['vocab'][5] == 'pp32_256' and D.padded_columns(5004, p['vocab'][5]) == 116
    assert p['gate'][2] == 3904 and p['gate'][5:] == ('pp32_128', 'bias_sigmul_split')
    assert p['q'][5] == 'pp32_256'
    assert D.attend_path(15, 512) == 'attend16' and D.context_path(15, 3904) == (True, 4)
    assert D.lm_split_ok(G['prod'], 'split_f16') and not D.lm_split_ok(G['prod'], 'f32')
    # small: 4H = 256 and the ragged V on the 256 tile, F = 160 on the 128 tile
    s = tiles('small')
    assert D.fused(G['small'])
    assert s['lstm'][2] == 256 and s['lstm'][5:] == ('pp32_256', 'lstm')
    assert s['vocab'][5] == 'pp32_256' and D.padded_columns(2300, 'pp32_256') == 4
    assert s['gate'][5] == 'pp32_128' and s['q'][5] == 'split_256x64'
    # h96: EPI_LSTM at N = 384 on the 128 tile, A % 64 != 0, two context slices, V on 128
    h = tiles('h96')
    assert D.fused(G['h96']) and h['lstm'][2] == 384 and h['lstm'][5:] == ('pp32_128', 'lstm')
    assert G['h96'].A % 64 != 0 and D.context_path(15, 1056) == (True, 2)
    assert h['vocab'][5] == 'pp32_128'
    # k32: K = 32, one 32-wide k-tile in the vocabulary product (the ring has 5 stages)
    k = tiles('k32')
    assert D.fused(G['k32']) and k['vocab'][3] == 32 and k['vocab'][5] == 'pp32_256'
    # kK: 17 leaves both resident kernels, 16 is the last that stays
    assert D.attend_path(16, 64) == 'attend16' and D.context_path(16, 160)[0]
    assert D.attend_path(17, 64) == 'attend' and not D.context_path(17, 160)[0]
    assert D.attend_path(1, 64) == 'attend16'
    # a512 / a520
    assert D.attend_path(15, 512) == 'attend16' and D.attend_path(15, 520) == 'attend'
    assert tiles('a520')['q'][5] == 'pp32_128' and tiles('a512')['q'][5] == 'pp32_256'
    # unfused: two products for the cell, the first without a split copy
    u = tiles('unfused')
    assert not D.fused(G['unfused'])
    assert 'lstm' not in u and u['lstm_ih'][5] == 'f32_128x128' and u['lstm_hh'][6] == 'bias_add'
    assert u['lstm_hh'][5] == 'pp32_256' and u['gate'][6] == 'bias_sigmul'
    # f32: nothing on a split tile
    for geom in G:
        for g in D.step_gemms(G[geom], rows, 'f32', k=15):
            assert g[5].startswith('f32') and D.TILE_FAMILY[g[5]] == 'f32'
    # every case of the table: the log-prob kernel, and a second row tile where n > 256
    for case in D.CASES:
        assert D.row_select_path(case.dims.V, 0) == 'reg'
    assert sum(c.n > 256 for c in D.CASES) >= 8
    # the beam case (90, 50): fewer wave slots than rows, so a wave walks two rows
    rs, walks = D.attend_grid(90, 50)
    assert (rs, walks) == (12, True) and rs < -(-50 // 4)
    assert D.attend_grid(64, 16) == (4, False) and D.attend_grid(257, 1) == (1, False)
    for geom, n, beam in D.BEAM_CASES:
        assert D.row_select_path(G[geom].V, beam) == 'reg'


def test_edge_tokens():
    for case in D.CASES:
        d = case.dims
        tok = D.edge_tokens(d, case.n)
        _, stop = D.specials(d)
        assert stop in tok.tolist() and 0 <= int(tok.min()) and int(tok.max()) < d.V
        assert case.n in (256, 257) or tok[-1] == stop
        if case.n >= 257:
            assert tok[0] == 0 and tok[255] == d.V - 1 and tok[256] == D.ragged_id(d)
        if case.n > 4:
            assert {0, d.V - 1, D.ragged_id(d), stop} <= set(tok.tolist())


# ---- 3. conditioning: the oracle's own error, per case ---------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_errors(case):
    """Worst |fp32 CPU oracle - float64| per quantity: init_state, the single step of the GPU
    test, teacher forcing with and without MI."""
    d, sd, feats, targets = inputs(case)
    sd64, f64 = D.promote(sd), feats.double()
    start, _ = D.specials(d)
    e = dict(state=0., att=0., logp=0., score=0.)

    def worst(key, a, b):
        e[key] = max(e[key], float((a.double() - b).abs().max()))

    st32, st64 = O.init_state(feats, sd), D.init_state(f64, sd64)
    worst('state', st32.h, st64.h)
    worst('state', st32.c, st64.c)
    keys64 = D.project_keys(f64, sd64)
    _, _, st1 = D.step(f64, keys64, torch.full((case.n,), start), st64, sd64)
    h1, c1 = st1.h.float(), st1.c.float()
    tok = D.edge_tokens(d, case.n)
    p64, a64, s64 = D.step(f64, keys64, tok, D.State(h1.double(), c1.double(), None, None), sd64)
    p32, a32, s32 = O.step(feats, O.project_keys(feats, sd), tok, O.State(h1, c1, None, None), sd)
    worst('logp', p32, p64)
    worst('att', a32, a64)
    worst('state', s32.h, s64.h)
    worst('state', s32.c, s64.c)
    for mi in (False, True):
        o = O.teacher_forced(feats, sd, start, targets, mi=mi)
        r = D.teacher_forced(f64, sd64, start, targets, mi=mi)
        worst('logp', o.predictions, r.predictions)
        worst('att', o.attentions, r.attentions)
        worst('score', o.scores, r.scores)
    return e


@pytest.mark.parametrize('case', D.CASES, ids=IDS)
def test_oracle_is_well_inside_the_bound(case):
    e = oracle_errors(case)
    length = D.forced_length(case)
    print(f'{D.case_id(case)}: fp32 oracle vs float64: h/c {e["state"]:.2e}  att {e["att"]:.2e}  '
          f'log-probs {e["logp"]:.2e}  scores({length}) {e["score"]:.2e}')
    assert e['state'] <= D.STATE_CLASS / 4
    assert e['att'] <= D.ATT_CLASS / 4
    assert e['logp'] <= D.LOGP_CLASS / 4
    assert e['score'] <= length * D.LOGP_CLASS / 4


def test_constants_are_the_table_worst_times_nine():
    """Each constant IS 9 x the oracle's worst over the table, rounded to one significant
    digit."""
    worst = {k: max(oracle_errors(c)[k] for c in D.CASES) for k in ('state', 'att', 'logp')}
    print('fp32 oracle vs float64, worst over the table: ' +
          '  '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    print(f'x {D.ORACLE_RATIO:g}: ' +
          '  '.join(f'{k} {D.ORACLE_RATIO * v:.3g}' for k, v in worst.items()))
    print(f'constants: STATE_CLASS {D.STATE_CLASS:g}  ATT_CLASS {D.ATT_CLASS:g}  '
          f'LOGP_CLASS {D.LOGP_CLASS:g}')
    for const, key in ((D.STATE_CLASS, 'state'), (D.ATT_CLASS, 'att'), (D.LOGP_CLASS, 'logp')):
        assert float(f'{D.ORACLE_RATIO * worst[key]:.0e}') == const, (key, worst[key], const)


@pytest.mark.parametrize('seed', range(D.FUZZ_SEEDS))
def test_fuzz_geometries_are_fused_and_conditioned(seed):
    """Every geometry of the GPU fuzz takes the fused branch on split tiles only, and the
    oracle is well inside the bound there too: no seed is skipped."""
    d, k, n = D.fuzz_geometry(seed)
    assert D.fused(d) and d.F <= 1200 and 1 <= k <= 16 and 1 <= n <= 300
    gemms = D.step_gemms(d, n, 'split_f16')
    assert [g[0] for g in gemms] == ['q', 'gate', 'lstm', 'vocab']
    assert all(not g[5].startswith('f32') for g in gemms) and D.gemm(gemms, 'lstm')[4] == d.E + d.F
    sd = D.weights('fuzz', seed, d)
    feats = D.features(d, n, k, seed)
    targets = D.forced_targets(d, n, 3, seed)
    mi = bool(seed % 2)
    start, _ = D.specials(d)
    o = O.teacher_forced(feats, sd, start, targets, mi=mi)
    r = D.teacher_forced(feats.double(), D.promote(sd), start, targets, mi=mi)
    e = (float((o.predictions - r.predictions).abs().max()),
         float((o.attentions - r.attentions).abs().max()))
    print(f'fuzz {seed} {tuple(d)} k={k} n={n}: fp32 oracle vs float64: log-probs {e[0]:.2e}  '
          f'att {e[1]:.2e}')
    assert e[0] <= D.LOGP_CLASS / 4 and e[1] <= D.ATT_CLASS / 4


# ---- 4. what the bound resolves ---------------------------------------------------------------
def step_setup(geom, n, k, lm=False):
    d = D.GEOMETRIES[geom]
    sd = D.promote(D.weights(geom))
    feats = D.features(d, n, k).double()
    keys = D.project_keys(feats, sd)
    st0 = D.init_state(feats, sd, lm)
    start, _ = D.specials(d)
    _, _, st1 = D.step(feats, keys, torch.full((n,), start), st0, sd)
    tok = D.edge_tokens(d, n)
    return d, sd, feats, keys, tok, st1


def step_ratio(geom, n, k, hook, lm=False):
    """Worst error / bound over pred, att, h2, c2 of one mutated step."""
    d, sd, feats, keys, tok, st1 = step_setup(geom, n, k, lm)
    want = D.step(feats, keys, tok, st1, sd)
    got = D.step(feats, keys, tok, st1, sd, hook=hook)
    ratios = dict(pred=float((got[0] - want[0]).abs().max()) / D.LOGP_CLASS,
                  att=float((got[1] - want[1]).abs().max()) / D.ATT_CLASS,
                  h2=float((got[2].h - want[2].h).abs().max()) / D.STATE_CLASS,
                  c2=float((got[2].c - want[2].c).abs().max()) / D.STATE_CLASS)
    return ratios


def replace(stage, fn):
    def hook(name, value, env):
        if name == stage:
            return fn(value.clone(), env)
    return hook


def to_f16(v, env):
    return v.to(torch.float16).double()


def swap_att(v, env):
    v[3, [4, 5]] = v[3, [5, 4]]
    return v


def c_in_255(v, env):
    v[256] = v[255]
    return v


def swap_i_f(v, env):
    hsz = v.shape[1] // 4
    v[:, 16:32], v[:, hsz + 16:hsz + 32] = v[:, hsz + 16:hsz + 32].clone(), v[:, 16:32].clone()
    return v


def lse_without_tail(v, env):
    logits = env['logits']
    return logits[:, :logits.shape[1] - logits.shape[1] % 64].logsumexp(dim=-1, keepdim=True)


def lm_previous_row(v, env):
    return v.roll(1, dims=0)


STEP_MUTANTS = {
    'a-vocab-f16': ('small', 257, 15, replace('vocab_a', to_f16), False),
    'a-lstm-f16': ('small', 257, 15, replace('lstm_a', to_f16), False),
    'a-vocab-f16-prod': ('prod', 257, 15, replace('vocab_a', to_f16), False),
    'a-lstm-f16-prod': ('prod', 257, 15, replace('lstm_a', to_f16), False),
    'b-att-swap': ('small', 257, 15, replace('att', swap_att), False),
    'd-c_in-row-256': ('small', 257, 15, replace('c_in', c_in_255), False),
    'e-gates-i-f': ('small', 257, 15, replace('gates', swap_i_f), False),
    'f-lse-tail': ('small', 257, 15, replace('lse', lse_without_tail), False),
    'f-lse-tail-prod': ('prod', 3, 15, replace('lse', lse_without_tail), False),
    'h-lm-row': ('small', 257, 15, replace('lm_logp', lm_previous_row), True),
}


@pytest.mark.parametrize('name', sorted(STEP_MUTANTS))
def test_step_mutant_exceeds_the_bound(name):
    geom, n, k, hook, lm = STEP_MUTANTS[name]
    ratios = step_ratio(geom, n, k, hook, lm)
    print(f'mutant {name} on {geom} n={n}: error / bound: ' +
          '  '.join(f'{q} {r:.3g}' for q, r in ratios.items()))
    assert max(ratios.values()) >= 10, ratios


def wrong_neuron(value, env):
    """The first beam row of neuron 1 pooled with neuron 0's features."""
    if env['rpn'] == 1:
        return None
    r = env['rpn']
    value[r] = env['att'][r] @ env['feats'][0]
    return value


def wrong_backpointer(value, env):
    """One beam's state follows another parent (the back-trace keeps the right one)."""
    beam = env['beam']
    value[1] = value[0] if value[1] != value[0] else value[0] - value[0] % beam + (
        value[0] % beam + 1) % beam
    return value


SEARCH_MUTANTS = {
    'c-neuron-features': replace('ctx', wrong_neuron),
    'g-backpointer': replace('rows', wrong_backpointer),
}


@pytest.mark.parametrize('name', sorted(SEARCH_MUTANTS))
def test_search_mutant_is_caught_by_rescore(name):
    geom, n, beam = 'small', 7, 5
    d = D.GEOMETRIES[geom]
    sd = D.promote(D.weights(geom))
    feats = D.features(d, n, D.BEAM_K, D.BEAM_SEEDS[(geom, n, beam)]).double()
    start, stop = D.specials(d)
    clean = D.beam_search(feats, sd, start, stop, D.BEAM_LENGTH, beam)
    assert float((D.rescore(feats, clean.tokens, sd, start, stop) -
                  clean.scores).abs().max()) < 1e-11
    got = D.beam_search(feats, sd, start, stop, D.BEAM_LENGTH, beam, hook=SEARCH_MUTANTS[name])
    re = D.rescore(feats, got.tokens, sd, start, stop)
    ratio = float((re - got.scores).abs().max()) / (D.BEAM_LENGTH * D.LOGP_CLASS)
    print(f'mutant {name} on {geom} n={n} beam={beam}: |scores - rescore| / bound {ratio:.3g}')
    assert ratio >= 10


# ---- 5. the beam cases ------------------------------------------------------------------------
@pytest.mark.parametrize('mi', [True, False], ids=['beam-mi', 'rerank-lik'])
@pytest.mark.parametrize('geom,n,beam', D.BEAM_CASES,
                         ids=[f'{g}-n{n}-b{b}' for g, n, b in D.BEAM_CASES])
def test_beam_seeds(geom, n, beam, mi):
    """n <= 7: every float64 select margin is at least TIE (so the GPU test allows no
    excuse).  Larger cases: the fp32 oracle itself differs from the float64 search in at
    most 2 neurons, each on a near-tie."""
    d = D.GEOMETRIES[geom]
    sd = D.weights(geom)
    feats = D.features(d, n, D.BEAM_K, D.BEAM_SEEDS[(geom, n, beam)])
    start, stop = D.specials(d)
    want = D.beam_search(feats.double(), D.promote(sd), start, stop, D.BEAM_LENGTH, beam, mi)
    near = int((want.margins < TIE).sum())
    print(f'{geom} n={n} beam={beam} mi={int(mi)}: smallest float64 margin '
          f'{float(want.margins.min()):.3g}, {near} neurons below TIE')
    assert want.tokens.shape[2] == D.BEAM_LENGTH
    if n <= 7:
        assert near == 0
    got = D.beam_search(feats, sd, start, stop, D.BEAM_LENGTH, beam, mi)
    excuses = D.beam_set_excuses(got.tokens, want.tokens, want.margins, TIE, 'fp32 oracle')
    print(f'fp32 oracle: {excuses} excuses')
    assert excuses <= (0 if n <= 7 else 2)
    assert float((got.scores.double() - D.rescore(feats.double(), got.tokens, D.promote(sd),
                                                  start, stop, mi)).abs().max()) \
        <= D.BEAM_LENGTH * D.LOGP_CLASS / 4


# ---- 6. off the unit operand scale --------------------------------------------------------------
def _everything(feats, sd, case):
    """init_state, the single step of the GPU test and teacher forcing (both MI settings) in
    the dtype of `sd`, as one flat list of tensors."""
    d = case.dims
    start, _ = D.specials(d)
    out = []
    st0 = D.init_state(feats, sd, lm=True)
    out += [st0.h, st0.c]
    keys = D.project_keys(feats, sd)
    _, _, st1 = D.step(feats, keys, torch.full((case.n,), start), st0, sd)
    p, a, st2 = D.step(feats, keys, D.edge_tokens(d, case.n), st1, sd)
    out += [p, a, st2.h, st2.c, st2.h_lm, st2.c_lm]
    targets = D.forced_targets(d, case.n, D.forced_length(case))
    for mi in (False, True):
        f = D.teacher_forced(feats, sd, start, targets, mi=mi)
        out += [f.predictions, f.attentions, f.scores]
    return out


@functools.lru_cache(maxsize=None)
def _unscaled(case, double):
    sd = D.weights(case.geom)
    feats = D.features(case.dims, case.n, case.k)
    if double:
        sd, feats = D.promote(sd), feats.double()
    return _everything(feats, sd, case)


@pytest.mark.parametrize('log2_feat,log2_emb', D.SCALES,
                         ids=[f'f{f}-e{e}' for f, e in D.SCALES])
@pytest.mark.parametrize('case', D.RANGE_CASES, ids=[D.case_id(c) for c in D.RANGE_CASES])
def test_rescaled_is_exact(case, log2_feat, log2_emb):
    """The rescaled case under the fp32 oracle's arithmetic, and under float64, gives the
    bits of the unscaled one: nothing underflows or overflows and the transform is right.
    Hence the oracle's error against float64 is one figure for every scale, and the GPU test
    keeps STATE_CLASS / ATT_CLASS / LOGP_CLASS unchanged."""
    sd, feats = D.rescaled(D.weights(case.geom), D.features(case.dims, case.n, case.k),
                           log2_feat, log2_emb)
    assert torch.equal(feats, D.features(case.dims, case.n, case.k) * 2.0 ** log2_feat)
    assert torch.isfinite(feats).all() and float(feats[feats > 0].min()) > 2.0 ** -100
    worst = 0.0
    for double in (False, True):
        got = _everything(feats.double(), D.promote(sd), case) if double else \
            _everything(feats, sd, case)
        for g, w in zip(got, _unscaled(case, double)):
            assert torch.equal(g, w)
    for g32, g64 in zip(_unscaled(case, False), _unscaled(case, True)):
        worst = max(worst, float((g32.double() - g64).abs().max()))
    print(f'{D.case_id(case)} f={log2_feat} e={log2_emb}: bit-exact in fp32 and float64; '
          f'fp32 oracle vs float64 (any quantity) {worst:.2e} at every scale')


def test_range_cases_are_table_cases():
    """The sweep's two cases are rows of the 4.19 table (so the constants cover them), and
    at 2^10 the largest feature is far below the clamp."""
    for case in D.RANGE_CASES:
        assert case in D.CASES and D.fused(case.dims)
        top = float(D.features(case.dims, case.n, case.k).max()) * 2.0 ** max(D.FEATURE_SCALES)
        assert top < 65504 / 8, top
    assert set(D.SCALES) >= {(f, 0) for f in D.FEATURE_SCALES} | {(-10, 6)}
    # the extra geometry of test_feature_scale_is_undone_exactly: not fused, but the cell's
    # product has a concatenated split copy (decoder.hip, cat_linear / lstm_layer)
    c = D.CAT_DIMS
    assert not D.fused(c) and (c.E + c.F) % 32 == 0 and c.H % 32 == 0 and c.E % 16 != 0
    assert [g[0] for g in D.step_gemms(c, D.CAT_CASE.n, 'split_f16')] == \
        ['q', 'gate', 'lstm', 'vocab']


def test_subnormal_lo_exceeds_the_bound():
    """Resolution: at feature scale 2^-14 on `prod`, the feature operands of the float64
    reference (the features the keys are projected from, the context vector) rounded to an
    absolute grid of 2^-24 -- what a `lo` half in the f16 subnormals leaves of them -- move a
    step by at least 10 x the bound.  The sweep sees the defect it exists for."""
    case = D.RANGE_CASES[1]
    assert case.geom == 'prod'
    d = case.dims
    sd, feats = D.rescaled(D.promote(D.weights(case.geom)),
                           D.features(d, case.n, case.k).double(), -14, 0)
    start, _ = D.specials(d)
    keys = D.project_keys(feats, sd)
    st0 = D.init_state(feats, sd)
    _, _, st1 = D.step(feats, keys, torch.full((case.n,), start), st0, sd)
    tok = D.edge_tokens(d, case.n)
    want = D.step(feats, keys, tok, st1, sd)
    grid = 2.0 ** -24
    coarse = torch.round(feats / grid) * grid
    got = D.step(feats, D.project_keys(coarse, sd), tok, st1, sd, hook=D.resolution_hook(grid))
    ratios = dict(pred=float((got[0] - want[0]).abs().max()) / D.LOGP_CLASS,
                  att=float((got[1] - want[1]).abs().max()) / D.ATT_CLASS,
                  h2=float((got[2].h - want[2].h).abs().max()) / D.STATE_CLASS,
                  c2=float((got[2].c - want[2].c).abs().max()) / D.STATE_CLASS)
    print('2^-24 grid on the feature operands at 2^-14, prod: error / bound: ' +
          '  '.join(f'{q} {r:.3g}' for q, r in ratios.items()))
    assert max(ratios.values()) >= 10, ratios
