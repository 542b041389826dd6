"""GPU: the inference decoder OFF the unit feature scale, and at features the split format
cannot hold.  DESIGN.md section 4.21.

  1. The scale sweep.  `decref.rescaled` states the same decoder in other units (features
     x 2^f, embeddings x 2^e, the weights that multiply them divided by the same power of
     two), which is exact in fp32 and float64 (tests/test_decoder_ref_host.py), so the
     float64 reference and the bounds of section 4.19 hold unchanged at every scale.  The
     exact-fp32 mode must be homogeneous bit for bit.  split_f16 must stay within the
     bounds at every scale once the context's feature and embedding scales are set
     (`Context.set_feature_scale_log2`, `set_embedding_scale_log2`, chosen by `calibrate`'s
     rule); at the default scales 2^0 it must where neither operand was scaled down, and
     below that the figure is printed next to the calibrated one.
  2. A feature of +-70000 or Inf raises at every entry point of the decoder (or reruns the
     call in f32), and leaves no stale flag behind.
  3. A NaN feature is not a saturation: it poisons its neuron as in the float64 reference
     and leaves every other neuron's bits alone, in both precisions.

The caller supplies every token here (single steps, teacher forcing): no kernel derives an
index from the altered data.  Every test prints its figures before it asserts."""
import functools
import warnings

import pytest
import torch

import decref as D
from milan_amd import decoders, encoders, hip, lang, lms, synthetic
from oracle import milan_oracle as O
from test_gpu_dtype_error import _scaled_network
from test_gpu_full_decoder import err, forced_reference, report, step_reference

pytestmark = pytest.mark.gpu

SCALE_IDS = [f'f{f}-e{e}' for f, e in D.SCALES]
CASE_IDS = [D.case_id(c) for c in D.RANGE_CASES]


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


@pytest.fixture(scope='module')
def contexts(dev):
    """One hip.Context per (geometry, log2 feature scale, log2 embedding scale) of the
    rescaled weights, made on first use."""
    made = {}

    def get(geom, precision, log2_feat=0, log2_emb=0):
        key = (geom, log2_feat, log2_emb)
        if key not in made:
            d = D.CAT_DIMS if geom == 'cat' else D.GEOMETRIES[geom]
            sd, _ = D.rescaled(D.weights(geom), torch.zeros(1), log2_feat, log2_emb)
            made[key] = hip.Context(hip.make_dims(sd, d.V - 4), sd, dev)
        made[key].set_precision(precision)
        return made[key]

    yield get
    for ctx in made.values():
        ctx.close()


# ---- 1. the scale sweep -------------------------------------------------------------------
BOUNDS = dict(h0=D.STATE_CLASS, c0=D.STATE_CLASS, pred=D.LOGP_CLASS, att=D.ATT_CLASS,
              h2=D.STATE_CLASS, c2=D.STATE_CLASS, f_pred=D.LOGP_CLASS, f_att=D.ATT_CLASS,
              mi_pred=D.LOGP_CLASS, mi_att=D.ATT_CLASS)


def run_everything(ctx, case, log2_feat, lm_step=False):
    """init_state, the single step of 4.19 and teacher forcing with and without MI on the
    features x 2^log2_feat: (outputs by name, error against float64 by name)."""
    ref = step_reference(case)
    feats = ref['feats'] * 2.0 ** log2_feat
    h0, c0 = ctx.init_state(feats)
    pred, att, h2, c2, _, _ = ctx.step(feats, ref['tok'], ref['h1'], ref['c1'], None, None,
                                       D.TEMPERATURE)
    outs = dict(h0=h0, c0=c0, pred=pred, att=att, h2=h2, c2=c2)
    if lm_step:
        # the public step with an LM state: milan_step's LM runs lm_step (the fp32 embedding
        # gather), not the split-format LM of decode; no reference, bits only
        zeros = torch.zeros(2, case.n, case.dims.H)
        mp, _, _, _, hl, cl = ctx.step(feats, ref['tok'], ref['h1'], ref['c1'], zeros, zeros,
                                       D.TEMPERATURE)
        extra = dict(lm_pred=mp.cpu(), lm_h=hl.cpu(), lm_c=cl.cpu())
    want = dict(h0=ref['st0'].h, c0=ref['st0'].c, pred=ref['pred'], att=ref['att'],
                h2=ref['st2'].h, c2=ref['st2'].c)
    length = D.forced_length(case)
    for mi, tag in ((False, 'f'), (True, 'mi')):
        _, targets, forced = forced_reference(case, mi)
        out = ctx.decode(feats, hip.FORCED, length, 1, mi, D.TEMPERATURE, forced=targets)
        outs[tag + '_pred'], outs[tag + '_att'] = out['predictions'], out['attentions']
        outs[tag + '_scores'] = out['scores']
        want[tag + '_pred'], want[tag + '_att'] = forced.predictions, forced.attentions
        want[tag + '_scores'] = forced.scores
    outs = {k: v.cpu() for k, v in outs.items()}
    figures = {k: err(outs[k], want[k]) for k in outs}
    if lm_step:
        outs.update(extra)
    return outs, figures


def in_units(what, figures, bounds):
    print(what + ': error / bound  ' +
          '  '.join(f'{k} {v / bounds[k]:.2f}' for k, v in figures.items()) +
          f'  worst {max(v / bounds[k] for k, v in figures.items()):.2f}')


_UNIT_F32 = {}   # case id -> the f32 mode's outputs at the unit scale


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('log2_feat,log2_emb', D.SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize('case', D.RANGE_CASES, ids=CASE_IDS)
def test_scale_sweep(contexts, case, log2_feat, log2_emb, precision):
    length = D.forced_length(case)
    bounds = dict(BOUNDS, f_scores=length * D.LOGP_CLASS, mi_scores=length * D.LOGP_CLASS)
    ctx = contexts(case.geom, precision, log2_feat, log2_emb)
    what = f'sweep {D.case_id(case)} f={log2_feat} e={log2_emb} {precision}'
    assert ctx.feature_scale_log2 == 0
    if precision == 'f32':
        # the exact-fp32 MFMA path is homogeneous, bit for bit
        outs, figures = run_everything(ctx, case, log2_feat)
        in_units(what, figures, bounds)
        report(what, figures, bounds)
        if D.case_id(case) not in _UNIT_F32:
            _UNIT_F32[D.case_id(case)] = run_everything(contexts(case.geom, 'f32'), case, 0)[0]
        for k, v in outs.items():
            assert torch.equal(v, _UNIT_F32[D.case_id(case)][k]), \
                f'{what}: {k} differs from the bits of the unit scale'
        assert ctx.status() == 0
        return
    assert ctx.embedding_scale_log2 == 0
    _, at_default = run_everything(ctx, case, log2_feat)
    in_units(what + ' scales 2^0, 2^0', at_default, bounds)
    if log2_feat >= 0 and log2_emb >= 0:
        report(what + ' scales 2^0, 2^0', at_default, bounds)
        assert ctx.status() == 0
    # with the scales `calibrate` would pick for these features and embedding tables
    sd = D.weights(case.geom)
    kf = hip.Context.feature_scale_log2_for(
        float(step_reference(case)['feats'].max()) * 2.0 ** log2_feat)
    ke = hip.Context.feature_scale_log2_for(
        max(float(sd['embedding.weight'].abs().max()),
            float(sd['lm.embedding.weight'].abs().max())) * 2.0 ** log2_emb)
    assert kf >= 10 - log2_feat - 1 and ke > -log2_emb, (kf, ke)
    ctx.set_feature_scale_log2(kf)
    ctx.set_embedding_scale_log2(ke)
    try:
        _, figures = run_everything(ctx, case, log2_feat)
        in_units(what + f' scales 2^{kf}, 2^{ke}', figures, bounds)
        report(what + f' scales 2^{kf}, 2^{ke}', figures, bounds)
        assert ctx.status() == 0
    finally:
        ctx.set_feature_scale_log2(0)
        ctx.set_embedding_scale_log2(0)


@pytest.mark.parametrize('case', D.RANGE_CASES + (D.CAT_CASE,),
                         ids=CASE_IDS + [D.case_id(D.CAT_CASE)])
def test_feature_scale_is_undone_exactly(contexts, case):
    """The scale is a property of the context: 2^0 after a detour gives the bits of before;
    at a set scale a subset of the neurons gets the bits it got in the full batch; and the
    scale that matches the rescaling (features or embeddings x 2^-10, scale 2^10)
    reproduces the unit case's split operands, hence its bits.  `cat` takes step_core's
    non-fused branch with the cell on its concatenated split copy, and the step with an LM
    state takes `lm_step`: the places where a scale travels through an fp32 buffer."""
    unit = contexts(case.geom, 'split_f16')
    before, _ = run_everything(unit, case, 0, lm_step=True)
    assert torch.isfinite(before['lm_pred']).all()
    unit.set_feature_scale_log2(7)
    unit.set_embedding_scale_log2(5)
    try:
        assert unit.feature_scale_log2 == 7 and unit.embedding_scale_log2 == 5
        feats = step_reference(case)['feats']
        full = unit.init_state(feats)
        part = unit.init_state(feats[1:3])
        assert torch.equal(full[0][1:3], part[0]) and torch.equal(full[1][1:3], part[1])
        _, targets, _ = forced_reference(case, True)
        length = targets.shape[1]
        a = unit.decode(feats, hip.FORCED, length, 1, True, D.TEMPERATURE, forced=targets)
        b = unit.decode(feats[1:3], hip.FORCED, length, 1, True, D.TEMPERATURE,
                        forced=targets[1:3])
        assert torch.equal(a['predictions'][1:3], b['predictions'])
    finally:
        unit.set_feature_scale_log2(0)
        unit.set_embedding_scale_log2(0)
    after, _ = run_everything(unit, case, 0, lm_step=True)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for (f, e) in ((-10, 0), (0, -10)):
        ctx = contexts(case.geom, 'split_f16', f, e)
        ctx.set_feature_scale_log2(-f)
        ctx.set_embedding_scale_log2(-e)
        try:
            same, _ = run_everything(ctx, case, f, lm_step=True)
        finally:
            ctx.set_feature_scale_log2(0)
            ctx.set_embedding_scale_log2(0)
        for k in before:
            assert torch.equal(before[k], same[k]), (f, e, k)
    with pytest.raises(ValueError):
        unit.set_feature_scale_log2(hip.FEATURE_SCALE_LOG2_MAX + 1)


# ---- the small trunk + decoder of the end-to-end cases ---------------------------------------
NV, WIDTH, K, N, SIZE = 60, 64, 3, 2, 96
BLOCKS = synthetic.RESNET_BLOCKS['resnet50']
E2E_LENGTH = 4


def _full_network(factor):
    """resnet50 (width 64) + decoder.  `factor` != 1: the trunk of
    test_small_activations_keep_the_fp32_class (pyramid levels 1..4 are `factor` x the
    original, level 0 -- the first `WIDTH` feature columns -- stays) with every decoder
    weight column that multiplies such a feature divided by `factor`."""
    full = synthetic.milan_state_dict(NV + 4, config='resnet50', seed=7, width=WIDTH,
                                      hidden_size=64, embedding_size=32,
                                      lm_hidden_size=64, lm_embedding_size=32)
    for k, v in _scaled_network(factor).items():
        assert k in full and full[k].shape == v.shape, k
        full[k] = v
    if factor != 1.0:
        emb = full['embedding.weight'].shape[1]
        for name, first in (('init_h.0.weight', 0), ('init_c.0.weight', 0),
                            ('attend.key_to_hidden.weight', 0), ('lstm.weight_ih', emb)):
            w = full[name].clone()
            w[:, first + WIDTH:] /= factor
            full[name] = w
    return full


def test_calibrated_describe_of_a_small_feature_network(dev):
    """End to end: the x 1e-3 trunk with the decoder's feature weights x 1e3 computes, in
    exact arithmetic, what the unscaled network computes.  After `calibrate` the split-f16
    `describe(..., FORCED)` must be within LOGP_CLASS x length of the unscaled network's
    float64 teacher forcing; the figure at the default feature scale is printed."""
    images, masks = synthetic.exemplars(N, k=K, size=SIZE, seed=41, zero_every=0)
    unscaled = D.promote(_full_network(1.0))
    with torch.no_grad():
        feats64 = O.encode(O.byte_to_float(images).double(), masks.double(), unscaled,
                           blocks=BLOCKS)
    g = torch.Generator().manual_seed(5)
    targets = torch.randint(0, NV + 4, (N, E2E_LENGTH), generator=g)
    sd = _full_network(1e-3)
    ctx = hip.Context(hip.make_dims(sd, NV, blocks=BLOCKS), sd, dev)
    try:
        ctx.set_precision('split_f16')
        bound = D.LOGP_CLASS * E2E_LENGTH
        for mi in (False, True):
            want = D.teacher_forced(feats64, unscaled, NV, targets, mi=mi)
            ctx.set_act_scale_log2(5)
            ctx.set_feature_scale_log2(0)
            ctx.set_embedding_scale_log2(0)
            out = ctx.describe(images, masks, hip.FORCED, E2E_LENGTH, 1, mi, D.TEMPERATURE,
                               forced=targets)
            e0 = err(out['predictions'], want.predictions)
            ka = ctx.calibrate(images.reshape(-1, 3, SIZE, SIZE))
            kf, ke = ctx.feature_scale_log2, ctx.embedding_scale_log2
            out = ctx.describe(images, masks, hip.FORCED, E2E_LENGTH, 1, mi, D.TEMPERATURE,
                               forced=targets)
            e1 = err(out['predictions'], want.predictions)
            print(f'x1e-3 network mi={int(mi)}: |predictions - float64| default scales '
                  f'{e0:.2e}; calibrated (activation 2^{ka}, feature 2^{kf}, embedding '
                  f'2^{ke}) {e1:.2e} / '
                  f'{bound:.0e}')
            assert kf > 0
            assert e1 <= bound, (e1, bound)
            assert ctx.status() == 0
        # The calibrated scale holds under ANY mask: one-pixel masks turn every feature into
        # a single tap value (far above the global averages the calibration sample pooled),
        # and `describe` on the calibration images themselves must still not saturate.
        top = float(ctx.lib.milan_get_feature_absmax(ctx._h))
        worst = 0.0
        for y, x in ((0, 0), (5, 7), (48, 48), (95, 95), (31, 64)):
            peaked = torch.zeros_like(masks)
            peaked[..., y, x] = 1
            out = ctx.describe(images, peaked, hip.FORCED, E2E_LENGTH, 1, True, D.TEMPERATURE,
                               forced=targets, want_features=True)
            assert ctx.status() == 0
            worst = max(worst, float(out['features'].abs().max()))
        limit = 65504.0 / 2.0 ** ctx.feature_scale_log2
        print(f'one-pixel masks: largest feature {worst:.3g}, bound of the taps {top:.3g}, '
              f'clamp at {limit:.3g} (feature scale 2^{ctx.feature_scale_log2})')
        assert worst <= top * (1 + 1e-5) and 8 * top <= limit
    finally:
        ctx.close()


# ---- 2. features the split format cannot hold ----------------------------------------------
RN, RK = 7, 5           # neurons, exemplars of the out-of-range cases (`small`)
BAD_AT = (3, 2, 17)     # neuron, exemplar, column of the one altered element
CALLS = ('init_state', 'step', 'decode', 'decode_mi')


@functools.lru_cache(maxsize=None)
def range_inputs():
    d = D.GEOMETRIES['small']
    case = D.Case('small', 'small', d, RK, RN)
    ref = step_reference(case)
    targets = D.forced_targets(d, RN, 4)
    return d, ref, targets


def poisoned(value):
    feats = range_inputs()[1]['feats'].clone()
    feats[BAD_AT] = value
    return feats


def call(ctx, name, feats):
    """One of the four calls -> dict of its float outputs."""
    _, ref, targets = range_inputs()
    if name == 'init_state':
        h, c = ctx.init_state(feats)
        return dict(h=h, c=c)
    if name == 'step':
        pred, att, h2, c2, _, _ = ctx.step(feats, ref['tok'], ref['h1'], ref['c1'], None,
                                           None, D.TEMPERATURE)
        return dict(pred=pred, att=att, h=h2, c=c2)
    out = ctx.decode(feats, hip.FORCED, targets.shape[1], 1, name == 'decode_mi',
                     D.TEMPERATURE, forced=targets)
    return dict(pred=out['predictions'], att=out['attentions'], scores=out['scores'])


def reference_call(name, feats):
    """The same call in float64 (decref)."""
    d, ref, targets = range_inputs()
    sd = D.promote(D.weights('small'))
    f64 = feats.double()
    if name == 'init_state':
        st = D.init_state(f64, sd)
        return dict(h=st.h, c=st.c)
    if name == 'step':
        pred, att, st = D.step(f64, D.project_keys(f64, sd), ref['tok'],
                               D.State(ref['h1'].double(), ref['c1'].double(), None, None), sd)
        return dict(pred=pred, att=att, h=st.h, c=st.c)
    f = D.teacher_forced(f64, sd, D.specials(d)[0], targets, mi=name == 'decode_mi')
    return dict(pred=f.predictions, att=f.attentions, scores=f.scores)


@pytest.mark.parametrize('name', CALLS)
@pytest.mark.parametrize('bad', [70000.0, -70000.0, float('inf')], ids=['70000', '-70000', 'inf'])
def test_out_of_range_feature_raises(contexts, monkeypatch, name, bad):
    """split_f16: the call is named in a FloatingPointError and the status word is clear
    afterwards; with on_saturation = 'f32' the call is rerun once, warns once, counts, and
    returns the f32 mode's bits.  f32: no error, no flag."""
    feats = poisoned(bad)
    ctx = contexts('small', 'split_f16')
    monkeypatch.setattr(ctx, 'on_saturation', 'raise')   # (undone after the test)
    with pytest.raises(FloatingPointError, match=f'milan_amd: {name.split("_mi")[0]}: '):
        call(ctx, name, feats)
    assert ctx.status() == 0
    clean = call(ctx, name, range_inputs()[1]['feats'])    # the next call is not blamed
    assert all(torch.isfinite(v).all() for v in clean.values())
    before = ctx.saturation_fallbacks
    monkeypatch.setattr(ctx, 'on_saturation', 'f32')
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = call(ctx, name, feats)
    reruns = [w for w in caught if 'rerunning' in str(w.message)]
    assert len(reruns) == 1 and issubclass(reruns[0].category, RuntimeWarning), caught
    assert ctx.saturation_fallbacks == before + 1 and ctx.precision == 'split_f16'
    assert ctx.status() == 0
    f32 = contexts('small', 'f32')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        want = call(f32, name, feats)
    assert f32.status() == 0
    for k in want:
        assert torch.equal(got[k], want[k]) or (
            torch.equal(torch.isnan(got[k]), torch.isnan(want[k])) and
            torch.equal(got[k].nan_to_num(), want[k].nan_to_num())), k


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('name', CALLS)
def test_nan_feature_poisons_its_neuron_like_the_reference(contexts, monkeypatch, name,
                                                           precision):
    """One NaN feature: neuron 3 is NaN wherever the float64 reference's is (everywhere),
    every other neuron keeps the bits of the call with that element finite; no flag, no
    warning, no error."""
    feats = poisoned(float('nan'))
    want = reference_call(name, feats)
    for k, v in want.items():
        nan = torch.isnan(v).reshape(RN, -1)
        assert nan[BAD_AT[0]].all() and not nan[[i for i in range(RN) if i != BAD_AT[0]]].any(), k
    ctx = contexts('small', precision)
    monkeypatch.setattr(ctx, 'on_saturation', 'raise')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = call(ctx, name, feats)
    assert ctx.status() == 0
    clean = call(ctx, name, range_inputs()[1]['feats'])
    keep = [i for i in range(RN) if i != BAD_AT[0]]
    for k in want:
        g, c = got[k].cpu(), clean[k].cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(want[k])), f'{name} {precision}: {k}'
        assert torch.equal(g[keep], c[keep]), f'{name} {precision}: {k} of the other neurons'


@pytest.fixture(scope='module')
def small_model(dev):
    """milan_amd.decoders.Decoder around the `small` weights (a foreign encoder: features
    are handed in)."""
    d = D.GEOMETRIES['small']

    class Features(encoders.Encoder):
        feature_shape = (d.F,)

        def forward(self, images, masks=None, **kwargs):
            raise AssertionError('not used')

        def properties(self):
            return {}

    indexer = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(d.V - 4)), str.split, True,
                           True, True, True, 15)
    assert len(indexer) == d.V and indexer.start_index == D.specials(d)[0]
    lm = lms.LanguageModel(indexer, d.E, d.H, layers=2)
    dec = decoders.Decoder(indexer, Features(), lm, embedding_size=d.E, hidden_size=d.H,
                           attention_hidden_size=d.A)
    res = dec.load_state_dict(D.weights('small'), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return dec.to('cuda').eval()


def test_decoder_module_entry_points(small_model):
    """`Decoder.forward(features, encode=False)` and `Decoder.step` raise, fall back and
    carry a NaN exactly as the context's calls do."""
    dec = small_model
    _, ref, targets = range_inputs()
    state = decoders.DecoderState(ref['h1'].cuda(), ref['c1'].cuda(), None, None)
    tok = ref['tok'].cuda()

    def forward(feats):
        out = dec(feats.cuda(), encode=False, strategy=targets, length=targets.shape[1],
                  mi=False, temperature=D.TEMPERATURE)
        return out.predictions.cpu()

    def step(feats):
        return dec.step(feats.cuda(), tok, state, temperature=D.TEMPERATURE).predictions.cpu()

    hot, nan, clean = poisoned(70000.0), poisoned(float('nan')), range_inputs()[1]['feats']
    keep = [i for i in range(RN) if i != BAD_AT[0]]
    for fn, what in ((forward, 'decode'), (step, 'step')):
        dec.precision = 'f32'
        want = fn(hot)
        dec.precision = 'split_f16'
        with pytest.raises(FloatingPointError, match=f'milan_amd: {what}: '):
            fn(hot)
        base = fn(clean)                       # no stale flag
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            got = fn(nan)
        assert torch.isnan(got[BAD_AT[0]]).all() and torch.equal(got[keep], base[keep])
        dec.precision = 'auto'
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            got = fn(hot)
        assert sum('rerunning' in str(w.message) for w in caught) == 1
        assert torch.equal(got, want)
    dec.precision = 'split_f16'


# ---- 3. through the trunk: a NaN pixel, and no stale flag for `encode` ----------------------
@pytest.fixture(scope='module')
def tiny(dev):
    """The smoke test's network: a width-16 resnet50 with a decoder."""
    nv, k, n, size = 60, 5, 4, 96
    sd = synthetic.milan_state_dict(nv + 4, config='resnet50', seed=11, width=16,
                                    hidden_size=64, embedding_size=16,
                                    lm_hidden_size=64, lm_embedding_size=16)
    ctx = hip.Context(hip.make_dims(sd, nv, blocks=BLOCKS), sd, dev)
    images, masks = synthetic.exemplars(n, k=k, size=size, seed=5, zero_every=0)
    g = torch.Generator().manual_seed(3)
    targets = torch.randint(0, nv + 4, (n, 4), generator=g)
    yield ctx, sd, images, masks, targets
    ctx.close()


def test_no_stale_flag_for_the_next_encode(tiny, monkeypatch):
    """A saturated feature handed to `decode` is reported by `decode`; the clean `encode`
    that follows returns."""
    ctx, _, images, masks, targets = tiny
    ctx.set_precision('split_f16')
    monkeypatch.setattr(ctx, 'on_saturation', 'raise')
    flat, mflat = images.reshape(-1, 3, 96, 96), masks.reshape(-1, 1, 96, 96)
    feats = ctx.encode(flat, mflat).reshape(images.shape[0], images.shape[1], -1).clone()
    feats[1, 2, 17] = 70000.0
    for name, run in (('init_state', lambda: ctx.init_state(feats)),
                      ('decode', lambda: ctx.decode(feats, hip.FORCED, 4, 1, True,
                                                    D.TEMPERATURE, forced=targets))):
        with pytest.raises(FloatingPointError, match=f'milan_amd: {name}: '):
            run()
        assert ctx.status() == 0
        again = ctx.encode(flat, mflat)
        assert torch.isfinite(again).all()
    # unchecked calls leave the flag for the caller, as encode(check=False) does
    ctx.init_state(feats, check=False)
    assert ctx.status() & hip.STATUS_SATURATED
    assert ctx.status() == 0


def test_graphed_decode_reads_the_flag_after_the_replay(dev, monkeypatch):
    """`enable_graphs`: a greedy decode whose features hold one 70000 raises on the direct
    run, on the capture and on every replay (the word is read after the graph ran); under
    on_saturation = 'f32' the rerun -- a call of its own, outside the capture -- returns the
    f32 mode's bits.  (70000 is finite after the clamp: every token id stays in range.)"""
    d = D.GEOMETRIES['small']
    sd = D.weights('small')
    ctx = hip.Context(hip.make_dims(sd, d.V - 4), sd, dev)
    try:
        feats = poisoned(70000.0).to(dev)
        clean = range_inputs()[1]['feats'].to(dev)
        ctx.set_precision('f32')
        want = ctx.decode(feats, hip.GREEDY, 4, 1, True, D.TEMPERATURE)
        ctx.set_precision('split_f16')
        plain = ctx.decode(clean, hip.GREEDY, 4, 1, True, D.TEMPERATURE)
        ctx.enable_graphs(True)
        monkeypatch.setattr(ctx, 'on_saturation', 'raise')
        for _ in range(3):       # direct, capture + launch, replay
            with pytest.raises(FloatingPointError, match='milan_amd: decode: '):
                ctx.decode(feats, hip.GREEDY, 4, 1, True, D.TEMPERATURE)
            assert ctx.status() == 0
        assert ctx.graph_stats()[1] >= 2
        for _ in range(3):       # the clean features, same buffers: not blamed
            out = ctx.decode(clean, hip.GREEDY, 4, 1, True, D.TEMPERATURE)
        assert torch.equal(out['tokens'], plain['tokens'])
        assert torch.equal(out['predictions'], plain['predictions'])
        monkeypatch.setattr(ctx, 'on_saturation', 'f32')
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            got = ctx.decode(feats, hip.GREEDY, 4, 1, True, D.TEMPERATURE)
        assert sum('rerunning' in str(w.message) for w in caught) == 1
        assert ctx.saturation_fallbacks == 1 and ctx.precision == 'split_f16'
        for key in ('tokens', 'scores', 'predictions', 'attentions'):
            assert torch.equal(got[key], want[key]), key
    finally:
        ctx.close()


@pytest.mark.parametrize('precision', D.PRECISIONS)
@pytest.mark.parametrize('mi', [False, True], ids=['lik', 'mi'])
def test_nan_pixel_through_describe(tiny, monkeypatch, mi, precision):
    """One NaN pixel in a float image: `describe(..., FORCED)` warns of the non-finite
    input, raises nothing, returns NaN for the neuron that owns the image -- as the oracle
    does -- and the bits of the clean call for every other neuron."""
    ctx, sd, images, masks, targets = tiny
    ctx.set_precision(precision)
    monkeypatch.setattr(ctx, 'on_saturation', 'raise')
    clean = O.byte_to_float(images).clone()
    x = clean.clone()
    x[1, 2, 0, 5, 7] = float('nan')
    with torch.no_grad():
        feats = O.encode(x, masks.float(), sd, blocks=BLOCKS)
    want = O.teacher_forced(feats, sd, 60, targets, mi=mi, temperature=D.TEMPERATURE)
    nan = torch.isnan(want.predictions).reshape(len(images), -1)
    assert nan[1].all() and not nan[[0, 2, 3]].any()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        got = ctx.describe(x, masks, hip.FORCED, 4, 1, mi, D.TEMPERATURE, forced=targets)
    assert any('NaN / Inf' in str(w.message) for w in caught)
    assert not any('rerunning' in str(w.message) for w in caught)
    assert ctx.status() == 0
    base = ctx.describe(clean, masks, hip.FORCED, 4, 1, mi, D.TEMPERATURE, forced=targets)
    for key, ref in (('predictions', want.predictions), ('attentions', want.attentions),
                     ('scores', want.scores)):
        g, b = got[key].cpu(), base[key].cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(ref)), key
        assert torch.equal(g[[0, 2, 3]], b[[0, 2, 3]]), key
