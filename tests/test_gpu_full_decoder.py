"""GPU: the inference decoder -- `init_state`, one `step`, teacher forcing, beam search and
rerank -- against the float64 reference of tests/decref.py, over decref's case table (the
production width and the tile / kernel boundaries of the step's dispatch) in both precision
modes, within decref's fp32-class bounds.  DESIGN.md section 4.19 has the table, the bound
and the measured figures; tests/test_decoder_ref_host.py shows on the CPU that the table
reaches what it names and that the bound resolves the mutants it should.

Every test prints its figures before it asserts."""
import functools

import pytest
import torch

import decref as D
from beamcheck import TIE
from milan_amd import hip

pytestmark = pytest.mark.gpu

IDS = [D.case_id(c) for c in D.CASES]


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


@pytest.fixture(scope='module')
def contexts(dev):
    """One hip.Context per geometry, made on first use."""
    made = {}

    def get(geom, precision):
        if geom not in made:
            sd = D.weights(geom)
            made[geom] = hip.Context(hip.make_dims(sd, D.GEOMETRIES[geom].V - 4), sd, dev)
        made[geom].set_precision(precision)
        return made[geom]

    yield get
    for ctx in made.values():
        ctx.close()


def err(got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), 'non-finite result'
    return float((got - want).abs().max())


def report(what, figures, bounds):
    """Print `name err / bound` for every figure, then assert them all."""
    print(what + ': ' + '  '.join(f'{k} {v:.2e}/{bounds[k]:.0e}' for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= bounds[k], f'{what}: {k} error {v:.3g} exceeds the bound {bounds[k]:g}'


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """float64: the initial state, and one step from the state after step 1 rounded to fp32."""
    d = case.dims
    sd = D.promote(D.weights(case.geom))
    feats = D.features(d, case.n, case.k)
    f64 = feats.double()
    keys = D.project_keys(f64, sd)
    st0 = D.init_state(f64, sd)
    start, _ = D.specials(d)
    _, _, st1 = D.step(f64, keys, torch.full((case.n,), start), st0, sd)
    h1, c1 = st1.h.float(), st1.c.float()
    tok = D.edge_tokens(d, case.n)
    pred, att, st2 = D.step(f64, keys, tok, D.State(h1.double(), c1.double(), None, None), sd)
    return dict(feats=feats, st0=st0, h1=h1, c1=c1, tok=tok, pred=pred, att=att, st2=st2)


@functools.lru_cache(maxsize=None)
def forced_reference(case, mi):
    d = case.dims
    sd = D.promote(D.weights(case.geom))
    feats = D.features(d, case.n, case.k)
    targets = D.forced_targets(d, case.n, D.forced_length(case))
    want = D.teacher_forced(feats.double(), sd, D.specials(d)[0], targets, mi=mi)
    return feats, targets, want


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('case', D.CASES, ids=IDS)
def test_init_state_and_step(contexts, case, precision):
    """`init_state` on every case, and one `step` from the float64 reference's state after
    step 1 (rounded to fp32, fed to both sides) with the edge token ids 0, V - 1, V - V % 64
    and <stop> on rows 0, 255, 256 and the last (at n = 256 and 257, where two of those are
    one row, and below, an id moves to the nearest free row: `decref.edge_tokens`): pred, att,
    h2, c2.  (Should one exceed its bound: `decref.step` offers every stage
    of the reference to a hook -- q, att, ctx, x, gates, h2, c2, logits -- to find the first
    kernel that is off.)"""
    ctx = contexts(case.geom, precision)
    ref = step_reference(case)
    h0, c0 = ctx.init_state(ref['feats'])
    pred, att, h2, c2, _, _ = ctx.step(ref['feats'], ref['tok'], ref['h1'], ref['c1'], None,
                                       None, D.TEMPERATURE)
    figures = dict(h0=err(h0, ref['st0'].h), c0=err(c0, ref['st0'].c),
                   pred=err(pred, ref['pred']), att=err(att, ref['att']),
                   h2=err(h2, ref['st2'].h), c2=err(c2, ref['st2'].c))
    bounds = dict(h0=D.STATE_CLASS, c0=D.STATE_CLASS, pred=D.LOGP_CLASS, att=D.ATT_CLASS,
                  h2=D.STATE_CLASS, c2=D.STATE_CLASS)
    report(f'step {D.case_id(case)} {precision}', figures, bounds)
    assert ctx.status() == 0


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('mi', [False, True], ids=['lik', 'mi'])
@pytest.mark.parametrize('case', D.CASES, ids=IDS)
def test_teacher_forcing(contexts, case, mi, precision):
    ctx = contexts(case.geom, precision)
    feats, targets, want = forced_reference(case, mi)
    length = targets.shape[1]
    out = ctx.decode(feats, hip.FORCED, length, 1, mi, D.TEMPERATURE, forced=targets)
    assert torch.equal(out['tokens'].cpu(), targets)
    pred = out['predictions'].cpu()
    # scores are exactly the gathered predictions, accumulated in step order
    acc = torch.zeros(case.n)
    for t in range(length):
        acc = acc + pred[torch.arange(case.n), t, targets[:, t]]
    figures = dict(pred=err(pred, want.predictions), att=err(out['attentions'], want.attentions),
                   scores=err(out['scores'], want.scores))
    bounds = dict(pred=D.LOGP_CLASS, att=D.ATT_CLASS, scores=length * D.LOGP_CLASS)
    report(f'forced {D.case_id(case)} mi={int(mi)} {precision}', figures, bounds)
    assert torch.equal(acc, out['scores'].cpu())
    assert ctx.status() == 0


STRATEGIES = {'beam': (hip.BEAM, True), 'rerank': (hip.RERANK, False)}  # (strategy, mi)


@functools.lru_cache(maxsize=None)
def search_reference(geom, n, beam, mi, seed):
    d = D.GEOMETRIES[geom]
    sd = D.promote(D.weights(geom))
    feats = D.features(d, n, D.BEAM_K, seed)
    start, stop = D.specials(d)
    return feats, D.beam_search(feats.double(), sd, start, stop, D.BEAM_LENGTH, beam, mi=mi)


def check_search(ctx, geom, feats, beam, strategy, want, what, cap):
    """Everything the rows-per-neuron test asserts of one `decode`; returns the excuses."""
    d = D.GEOMETRIES[geom]
    sd = D.promote(D.weights(geom))
    start, stop = D.specials(d)
    n = len(feats)
    length = D.BEAM_LENGTH
    code, mi = STRATEGIES[strategy]
    out = ctx.decode(feats, code, length, beam, mi, D.TEMPERATURE)
    bt, bs = out['beam_tokens'].cpu(), out['beam_scores'].cpu()
    tp = int(out['out_len'].max())
    assert bt.shape == (n, beam, length) and (bt[:, :, tp:] == stop).all(), \
        f'{what}: tokens past out_len must be <stop>'
    assert (bs[:, :-1] >= bs[:, 1:]).all(), f'{what}: beam scores not sorted'
    # float64 teacher-forced rescoring of the GPU's own beams: no tie excuse needed
    re = D.rescore(feats.double(), bt[:, :, :tp], sd, start, stop, mi=mi)
    gap = float((bs.double() - re).abs().max())
    print(f'{what}: |beam_scores - rescore| {gap:.2e}/{length * D.LOGP_CLASS:.0e}', end='')
    assert gap <= length * D.LOGP_CLASS, (
        f'{what}: a returned beam score is {gap:.3g} off the float64 score of its own tokens')
    assert tp == want.tokens.shape[2], f'{what}: out_len {tp} != {want.tokens.shape[2]}'
    excuses = D.beam_set_excuses(bt, want.tokens, want.margins, TIE, what)
    print(f'  excuses {excuses}/{cap}')
    assert excuses <= cap, f'{what}: {excuses} near-tie excuses, at most {cap} allowed'
    if strategy == 'rerank':
        # the pick is one of the beams, and the best of them by the float64 PMI
        tok = out['tokens'].cpu()[:, :tp]
        starts = torch.full((n, beam, 1), start, dtype=torch.long)
        seqs = torch.cat([starts, bt[:, :, :tp]], dim=-1).view(n * beam, -1)
        pmi = re - D.TEMPERATURE * D.lm_score(seqs, sd, stop).view(n, beam)
        which = (bt[:, :, :tp] == tok.unsqueeze(1)).all(dim=-1)
        assert which.any(dim=1).all(), f'{what}: the reranked tokens are not one of the beams'
        picked = torch.where(which, pmi, pmi.new_full((), -1e30)).max(dim=1).values
        # tp decoder log-probs, minus temperature x tp LM log-probs of the same class
        bound = tp * (1 + D.TEMPERATURE) * D.LOGP_CLASS
        off = float((out['scores'].cpu().double() - picked).abs().max())
        print(f'{what}: |scores - float64 PMI of the pick| {off:.2e}/{bound:.1e}')
        assert off <= bound
        assert float((pmi.max(dim=1).values - picked).max()) <= 2 * bound, \
            f'{what}: rerank did not pick the best beam'
    return excuses


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('strategy', ['beam', 'rerank'])
@pytest.mark.parametrize('geom,n,beam', D.BEAM_CASES,
                         ids=[f'{g}-n{n}-b{b}' for g, n, b in D.BEAM_CASES])
def test_rows_per_neuron(contexts, geom, n, beam, strategy, precision):
    """Beam search and rerank with several rows per neuron (at (90, 50) attend16's waves walk
    two rows): every returned beam rescored in float64, the beam set against the float64
    search.  No excuse at n <= 7 (seeds chosen for margins >= TIE), at most 2 above."""
    ctx = contexts(geom, precision)
    seed = D.BEAM_SEEDS[(geom, n, beam)]
    feats, want = search_reference(geom, n, beam, STRATEGIES[strategy][1], seed)
    check_search(ctx, geom, feats, beam, strategy, want,
                 f'{strategy} {geom} n={n} beam={beam} {precision}', 0 if n <= 7 else 2)
    assert ctx.status() == 0


@pytest.mark.parametrize('precision', D.PRECISIONS)
def test_kernels_named_are_kernels_run(contexts, precision):
    """One `prod` step under the profiler: the products run in the kernel families decref's
    restated dispatch names."""
    case = D.CASES[0]
    assert case.geom == 'prod'
    ctx = contexts('prod', precision)
    ref = step_reference(case)
    ctx.step(ref['feats'], ref['tok'], ref['h1'], ref['c1'], None, None, D.TEMPERATURE)
    torch.cuda.synchronize()
    hip.profile_enable(True)
    try:
        ctx.step(ref['feats'], ref['tok'], ref['h1'], ref['c1'], None, None, D.TEMPERATURE)
        torch.cuda.synchronize()
        fam = hip.profile_read_kernels()
    finally:
        hip.profile_enable(False)
    launches = {k: int(v['launches']) for k, v in fam.items() if v['launches']}
    print(f'prod step {precision}: launches {launches}')
    want = {}
    for g in D.step_gemms(case.dims, case.n, precision, k=case.k):
        family = D.TILE_FAMILY[g[5]]
        want[family] = want.get(family, 0) + 1
    if precision == 'split_f16':
        assert want['pp32_256'] >= 1 and want['pp32_128'] >= 1 and 'f32' not in want
    else:
        assert set(want) == {'f32'}
    for family in ('pp32_256', 'pp32_128', 'f32'):
        assert launches.get(family, 0) == want.get(family, 0), (family, launches, want)


@pytest.mark.parametrize('seed', range(D.FUZZ_SEEDS))
def test_fuzz_fused(dev, seed):
    """Random geometries that always take step_core's fused branch: teacher forcing (MI on
    odd seeds) and a rescored beam search, split_f16."""
    d, k, n = D.fuzz_geometry(seed)
    assert D.fused(d)
    sd = D.weights('fuzz', seed, d)
    sd64 = D.promote(sd)
    start, stop = D.specials(d)
    mi = bool(seed % 2)
    feats = D.features(d, n, k, seed)
    targets = D.forced_targets(d, n, 3, seed)
    want = D.teacher_forced(feats.double(), sd64, start, targets, mi=mi)
    ctx = hip.Context(hip.make_dims(sd, d.V - 4), sd, dev)
    try:
        ctx.set_precision('split_f16')
        out = ctx.decode(feats, hip.FORCED, 3, 1, mi, D.TEMPERATURE, forced=targets)
        figures = dict(pred=err(out['predictions'], want.predictions),
                       att=err(out['attentions'], want.attentions),
                       scores=err(out['scores'], want.scores))
        what = f'fuzz {seed} {tuple(d)} k={k} n={n} mi={int(mi)}'
        report(what, figures, dict(pred=D.LOGP_CLASS, att=D.ATT_CLASS,
                                   scores=3 * D.LOGP_CLASS))
        nb = min(n, 40)
        beam = 2 + seed % 7
        out = ctx.decode(feats[:nb], hip.BEAM, 3, beam, mi, D.TEMPERATURE)
        bt, bs = out['beam_tokens'].cpu(), out['beam_scores'].cpu()
        tp = int(out['out_len'].max())
        re = D.rescore(feats[:nb].double(), bt[:, :, :tp], sd64, start, stop, mi=mi)
        gap = float((bs.double() - re).abs().max())
        print(f'{what}: beam {beam} |beam_scores - rescore| {gap:.2e}')
        assert gap <= 3 * D.LOGP_CLASS
        assert (bs[:, :-1] >= bs[:, 1:]).all() and (bt[:, :, tp:] == stop).all()
        assert ctx.status() == 0
    finally:
        ctx.close()
