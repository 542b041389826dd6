"""float64 reference of the inference decoder, the restated dispatch of one decoder step
and the case table of tests/test_gpu_full_decoder.py (a helper module like trunkref.py,
not a test file).  DESIGN.md section 4.19.

  * Reference: `init_state`, `step`, `teacher_forced`, `beam_search`, `rescore`, `lm_score`
    in the dtype of the weights they are given -- the fp32 tensors the GPU gets, promoted
    to float64 by `promote`.  Every stage of a step passes through an optional hook
    `hook(name, value, env) -> replacement or None`, so that a test can read a stage (to
    name the kernel that went wrong) or replace it (the mutants of
    tests/test_decoder_ref_host.py).  Run in float32 the functions give the bits of
    `oracle/milan_oracle.py`, which that test pins.
  * Dispatch: `step_gemms` and the `*_path` functions restate, for the default build and
    environment, which tile / kernel `csrc/decoder.hip` and `csrc/gemm.hip` give every
    product and glue launch of a step.  The two must move together: if the dispatch changes
    there, change it here, or the case table no longer provably reaches what it names.
  * `CASES`: the table.  Every GPU test parametrises over it x `PRECISIONS`.
  * The bound: `STATE_CLASS`, `ATT_CLASS`, `LOGP_CLASS`.
  * `rescaled`: the homogeneity transform of tests/test_gpu_decoder_range.py,
    with its scales and cases.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from milan_amd import synthetic
from oracle.milan_oracle import (State, _lin, init_state, lm_layers, lm_step,  # noqa: F401
                                 project_keys)

# ---- the bound ------------------------------------------------------------------------
# Absolute bounds on |GPU - float64|.  Each is the worst error of the fp32 CPU oracle
# against float64 over the whole case table (tests/test_decoder_ref_host.py prints and
# asserts the figures; DESIGN 4.19 lists them) times 9, the ratio the trunk's bound has
# over its oracle's worst (5e-6 / 5.7e-7), rounded to one digit.
#   worst over the table: h / c 9.2e-7, attention 2.1e-7, log-probs 2.1e-6; x 9: 8.3e-6,
#   1.9e-6, 1.9e-5.  attend16_kernel's tanh_exp2 (<= 2e-7 absolute per term, decoder.hip)
#   needs no allowance on top: the GPU's attention measures <= 6e-7 in both modes.
STATE_CLASS = 8e-6   # h, c (h in [-1, 1], c a few units)
ATT_CLASS = 2e-6     # attention weights (values in [0, 1])
LOGP_CLASS = 2e-5    # log-probs (values ~ -1 .. -30); a score of `length` tokens gets length x
ORACLE_RATIO = 9.0

PRECISIONS = ('split_f16', 'f32')
TEMPERATURE = 0.2

Dims = collections.namedtuple('Dims', 'H E F A V')
Case = collections.namedtuple('Case', 'tag geom dims k n')

GEOMETRIES = {
    'prod': Dims(512, 128, 3904, 512, 5004),
    'small': Dims(64, 32, 160, 64, 2300),
    'h96': Dims(96, 32, 1056, 40, 1000),
    'k32': Dims(32, 32, 160, 32, 2300),
    'a520': Dims(64, 32, 160, 520, 2300),
    'a512': Dims(64, 32, 160, 512, 2300),
    'unfused': Dims(64, 16, 244, 64, 2300),
}


def _cases():
    out = []

    def add(tag, geom, k, ns):
        for n in ns:
            out.append(Case(tag, geom, GEOMETRIES[geom], k, n))

    add('prod', 'prod', 15, (3, 257))
    add('small', 'small', 15, (1, 255, 256, 257, 513))
    add('h96', 'h96', 15, (257,))
    add('k32', 'k32', 5, (257,))
    for k in (1, 16, 17):
        add('kK', 'small', k, (257,))
    add('a520', 'a520', 15, (64,))
    add('a512', 'a512', 15, (64,))
    add('unfused', 'unfused', 5, (257,))
    return tuple(out)


CASES = _cases()


def case_id(case):
    return f'{case.tag}-k{case.k}-n{case.n}'


# (geometry, neurons, beam) of the rows-per-neuron test; seeds chosen on the CPU
# (tests/test_decoder_ref_host.py::test_beam_seeds): in the n <= 7 cases the first seed at
# which every float64 select margin, with and without MI, is >= 2 x beamcheck.TIE.
BEAM_CASES = (('small', 1, 50), ('small', 7, 5), ('small', 64, 16), ('small', 90, 50),
              ('prod', 3, 16), ('prod', 20, 16))
BEAM_SEEDS = {('small', 1, 50): 90, ('small', 7, 5): 167, ('small', 64, 16): 0,
              ('small', 90, 50): 0, ('prod', 3, 16): 109, ('prod', 20, 16): 0}
BEAM_LENGTH = 4
BEAM_K = 15


# the fuzz of the GPU test: geometries that always take step_core's fused branch
FUZZ_SEEDS = 16


def fuzz_geometry(seed):
    """(Dims, k, n): H in {32, 64, 96, 128}, E in {16, 32, 48}, F <= 1200 with
    (E + F) % 32 == 0, V in [300, 5200], k in [1, 16], n in [1, 300]."""
    g = torch.Generator().manual_seed(2957 + seed)

    def pick(seq):
        return seq[int(torch.randint(0, len(seq), (1,), generator=g))]

    def between(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    H, E = pick((32, 64, 96, 128)), pick((16, 32, 48))
    F_ = 32 * between(1, 37) + (-E % 32)
    d = Dims(H, E, F_, pick((24, 64, 100, 256)), between(300, 5200))
    return d, between(1, 16), between(1, 300)


def forced_length(case):
    return 2 if case.geom == 'prod' else 4


# ---- inputs ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(geom, seed=0, dims=None):
    """fp32 state dict of a geometry (decoder + 2-layer LM of the same H / E)."""
    d = dims or (CAT_DIMS if geom == 'cat' else GEOMETRIES[geom])
    return synthetic.decoder_state_dict(d.V, feature_size=d.F, hidden_size=d.H,
                                        embedding_size=d.E, attention_hidden_size=d.A,
                                        lm_hidden_size=d.H, lm_embedding_size=d.E,
                                        lm_layers=2, seed=seed)


def features(dims, n, k, seed=0):
    """(n, k, F) fp32, non-negative like pooled post-ReLU activations."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * n + k)
    return torch.randn(n, k, dims.F, generator=g).abs()


def specials(dims):
    """(start, stop) token ids: the vocabulary ends with <start> <stop> <pad> <unk>."""
    return dims.V - 4, dims.V - 3


def ragged_id(dims):
    """First column of the vocabulary's last, ragged 64-column group (of its last full group
    where V % 64 == 0)."""
    return dims.V - (dims.V % 64 or 64)


def edge_tokens(dims, n, seed=0):
    """(n,) token ids.  Rows 0, 255 and 256 carry 0, V - 1 and `ragged_id` (V - V % 64 where
    V % 64 != 0) and the last row <stop>, where n has those rows and they are distinct.
    Otherwise an id goes to the free row nearest its own: at n = 257 rows 255 and 256 keep
    V - 1 and the ragged id and <stop> moves to row 254; at n = 256 row 255 keeps V - 1, the
    ragged id goes to row 254 and <stop> to row 253; at n <= 255 <stop> is on the last row and
    the other ids on the rows before it.  n = 1 carries <stop> only."""
    g = torch.Generator().manual_seed(104729 * seed + n)
    tok = torch.randint(0, dims.V - 4, (n,), generator=g)
    used = set()
    want = [(0, 0), (255, dims.V - 1), (256, ragged_id(dims))]
    last = (n - 1, specials(dims)[1])
    for row, tid in want + [last] if n - 1 in (255, 256) else [last] + want:
        free = [r for r in range(n) if r not in used]
        if not free:
            break   # n = 1: <stop> came first and stays
        row = min(free, key=lambda r: (abs(r - row), r))
        tok[row] = tid
        used.add(row)
    return tok


def forced_targets(dims, n, length, seed=0):
    """(n, length) target ids for teacher forcing; column 0 carries the edge ids."""
    g = torch.Generator().manual_seed(15485863 * seed + 17 * n + length)
    t = torch.randint(0, dims.V, (n, length), generator=g)
    t[:, 0] = edge_tokens(dims, n, seed)
    return t


def promote(x, dtype=torch.float64):
    """A tensor, or a state dict, in `dtype` (integer tensors stay)."""
    if isinstance(x, dict):
        return {k: promote(v, dtype) for k, v in x.items()}
    return x.to(dtype) if x.is_floating_point() else x


# ---- off the unit operand scale -------------------------------------------
# (log2 feature scale, log2 embedding scale) of tests/test_gpu_decoder_range.py: the feature
# sweep, the embedding sweep, and one combined case whose column blocks of `lstm.weight_ih`
# sit 2^16 apart under the layer's single weight scale.
FEATURE_SCALES = (-14, -10, -6, 6, 10)
EMBEDDING_SCALES = (-10, 6)
SCALES = (tuple((f, 0) for f in FEATURE_SCALES) + tuple((0, e) for e in EMBEDDING_SCALES) +
          ((-10, 6),))
RANGE_CASES = (Case('small', 'small', GEOMETRIES['small'], 15, 257),
               Case('prod', 'prod', GEOMETRIES['prod'], 15, 3))
# E % 16 != 0 with (E + F) % 32 == 0 and H % 32 == 0: step_core's NON-fused branch, whose cell
# product still runs on the split copy of [W_ih | W_hh] (lstm_layer) -- the scales reach it
# through embed_kernel and the fp32 gate product instead of the split-format producers.  Not a
# row of the 4.19 table: only bit-for-bit statements are made about it.
CAT_DIMS = Dims(64, 8, 152, 64, 2300)
CAT_CASE = Case('cat', 'cat', CAT_DIMS, 15, 70)


def rescaled(sd, feats, log2_feat=0, log2_emb=0):
    """(sd', feats'): the same decoder in other units.  feats' = feats * 2^f with 2^-f on
    every weight column that multiplies a feature (init_h, init_c, key_to_hidden, the feature
    columns of lstm.weight_ih); the embedding tables * 2^e with 2^-e on the columns that
    multiply an embedding (decoder and LM).  Powers of two: exact in fp32 and float64 while
    nothing under- or overflows, so the float64 reference of the rescaled case is the
    reference of the original (tests/test_decoder_ref_host.py asserts it at every scale
    used).  Works on fp32 and on promoted float64 state dicts."""
    f, e = 2.0 ** log2_feat, 2.0 ** log2_emb
    emb = sd['embedding.weight'].shape[1]
    out = dict(sd)
    for name in ('init_h.0.weight', 'init_c.0.weight', 'attend.key_to_hidden.weight'):
        out[name] = sd[name] / f
    w = sd['lstm.weight_ih'].clone()
    w[:, :emb] /= e
    w[:, emb:] /= f
    out['lstm.weight_ih'] = w
    out['embedding.weight'] = sd['embedding.weight'] * e
    if 'lm.embedding.weight' in sd:
        out['lm.embedding.weight'] = sd['lm.embedding.weight'] * e
        out['lm.lstm.weight_ih_l0'] = sd['lm.lstm.weight_ih_l0'] / e
    return out, feats * f


def resolution_hook(grid=2.0 ** -24):
    """The defect the scale sweep exists for, as a hook for `step`: a feature operand whose
    `lo` half fell into the f16 subnormals keeps an absolute resolution of 2^-24.  The
    context vector is rounded to that grid ('ctx'; the keys' features are rounded by the
    caller, who projects them)."""
    def hook(name, value, env):
        if name == 'ctx':
            return torch.round(value / grid) * grid
    return hook


# ---- the reference --------------------------------------------------------------------
# (`State`, `init_state`, `project_keys`, `lm_step`, `lm_layers` are the oracle's own: they
# compute in the dtype of what they are given.  `step` is restated for the hook and the row
# groups, the search, `rescore` and `lm_score` for the oracle's float32 constants.)
def _tap(hook, name, value, env):
    if hook is None:
        return value
    new = hook(name, value, env)
    return value if new is None else new


def _cell(gates, c):
    i, f, g, o = gates.chunk(4, dim=-1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def step(feats, keys, tokens, state, sd, temperature=TEMPERATURE, hook=None, t=0):
    """`Decoder.step` (decoders.py:576-634) for rows that share features in groups:
    feats (n, k, F), keys (n, k, A), tokens (R,) with R = n * rpn, the rpn rows of a neuron
    adjacent.  Returns (predictions (R, V), attention (R, k), State).

    Stages offered to `hook`, in order: 'q' (R, A), 'att' (R, k), 'ctx' (R, F), 'x'
    (R, E + F) = [emb | gated], 'lstm_a' (R, E + F + H) the A operand [x | h] of the cell's
    product, 'gates' (R, 4H) pre-activations (i, f, g, o), 'c_in' (R, H), 'h2', 'c2',
    'vocab_a' (R, H) the A operand of the vocabulary product, 'logits' (R, V), 'lse' (R, 1),
    'logp' (R, V), 'lm_logp' (R, V), 'pred' (R, V).  `env` holds what was computed before
    the stage (feats, keys, tokens, rpn, t and the earlier stages by name)."""
    h, c, h_lm, c_lm = state
    n, k, _ = feats.shape
    rows = len(tokens)
    rpn = rows // n
    assert rpn * n == rows
    env = dict(feats=feats, keys=keys, tokens=tokens, rpn=rpn, t=t, h=h, c=c)

    def tap(name, value):
        value = _tap(hook, name, value, env)
        env[name] = value
        return value

    q = tap('q', _lin(h, sd, 'attend.query_to_hidden'))
    hidden = torch.tanh(q.view(n, rpn, 1, -1) + keys.unsqueeze(1))
    att = F.softmax(_lin(hidden, sd, 'attend.output.0'), dim=2).view(rows, k)
    att = tap('att', att)
    ctx = att.view(n, rpn, k, 1).mul(feats.unsqueeze(1)).sum(dim=2).view(rows, -1)
    ctx = tap('ctx', ctx)
    gate = torch.sigmoid(_lin(h, sd, 'feature_gate.0'))
    x = tap('x', torch.cat((sd['embedding.weight'][tokens], ctx * gate), dim=-1))
    if hook is None:
        gates = (F.linear(x, sd['lstm.weight_ih'], sd['lstm.bias_ih']) +
                 F.linear(h, sd['lstm.weight_hh'], sd['lstm.bias_hh']))
    else:
        e_f = x.shape[1]
        a = tap('lstm_a', torch.cat((x, h), dim=-1))
        gates = (F.linear(a[:, :e_f], sd['lstm.weight_ih'], sd['lstm.bias_ih']) +
                 F.linear(a[:, e_f:], sd['lstm.weight_hh'], sd['lstm.bias_hh']))
    gates = tap('gates', gates)
    h2, c2 = _cell(gates, tap('c_in', c))
    h2, c2 = tap('h2', h2), tap('c2', c2)
    logits = tap('logits', _lin(tap('vocab_a', h2), sd, 'output.1'))
    logp = F.log_softmax(logits, dim=-1)
    if hook is not None:
        lse = logits.logsumexp(dim=-1, keepdim=True)
        new = hook('lse', lse, env)
        if new is not None:
            logp = logits - new
    pred = logp = tap('logp', logp)
    if h_lm is not None:
        lm_logp, h_lm, c_lm = lm_step(tokens, h_lm, c_lm, sd)
        pred = logp - temperature * tap('lm_logp', lm_logp)
    pred = tap('pred', pred)
    return pred, att, State(h2, c2, h_lm, c_lm)


Forced = collections.namedtuple('Forced', 'scores predictions attentions')


def teacher_forced(feats, sd, start, targets, mi=False, temperature=TEMPERATURE, hook=None):
    """The `strategy=<tensor>` branch (decoders.py:444-445): (scores (n,), predictions
    (n, T, V), attentions (n, T, k)); the score is summed in step order."""
    n, length = targets.shape
    keys = project_keys(feats, sd)
    state = init_state(feats, sd, lm=mi)
    cur = torch.full((n,), start, dtype=torch.long)
    preds, atts = [], []
    scores = feats.new_zeros(n)
    for t in range(length):
        p, a, state = step(feats, keys, cur, state, sd, temperature, hook, t)
        cur = targets[:, t]
        preds.append(p)
        atts.append(a)
        scores = scores + p[torch.arange(n), cur]
    return Forced(scores, torch.stack(preds, 1), torch.stack(atts, 1))


Search = collections.namedtuple('Search', 'tokens scores margins')


def beam_search(feats, sd, start, stop, length, beam, mi=False, temperature=TEMPERATURE,
                hook=None):
    """allennlp 2.10 `BeamSearch._search` as the reference calls it (decoders.py:465-484;
    per_node_beam_size = beam, deterministic top-k, no constraints), restated from its
    published semantics as `oracle.milan_oracle.beam_search_core` is, in the dtype of `sd`:
    tokens (n, beam, T' <= length), scores (n, beam) sorted descending, and per neuron the
    smallest gap over all steps between the last kept and the first dropped candidate.
    `hook` also sees 'rows' (the flat parent rows the state is reordered by, from step 1
    on): a replacement moves the state only, not the back-trace."""
    n = len(feats)
    keys = project_keys(feats, sd)
    state = init_state(feats, sd, lm=mi)
    vmin = torch.finfo(torch.float32).min
    margin = torch.full((n,), float('inf'), dtype=feats.dtype)

    def note(pool):
        if pool.shape[1] > beam:
            top = pool.topk(beam + 1, dim=-1).values
            torch.minimum(margin, top[:, beam - 1] - top[:, beam], out=margin)

    logp, _, state = step(feats, keys, torch.full((n,), start, dtype=torch.long), state, sd,
                          temperature, hook, 0)
    v = logp.shape[1]
    last_lp, top_cls = logp.topk(beam, dim=-1)
    note(logp)
    if beam == 1 and bool((top_cls == stop).all()):
        return Search(top_cls.unsqueeze(-1), last_lp, margin)
    predictions, backpointers = [top_cls], []

    def ex(x, dim=0):
        return None if x is None else x.repeat_interleave(beam, dim=dim)

    state = State(ex(state.h), ex(state.c), ex(state.h_lm, 1), ex(state.c_lm, 1))
    after_end = torch.full((n * beam, v), vmin, dtype=feats.dtype)
    after_end[:, stop] = 0.0
    base = torch.arange(n).unsqueeze(1) * beam
    for t in range(1, length):
        last = predictions[-1].reshape(n * beam)
        if (last == stop).all():
            break
        logp, _, state = step(feats, keys, last, state, sd, temperature, hook, t)
        cleaned = torch.where((last == stop).unsqueeze(-1), after_end, logp)
        top_lp, top_cls = cleaned.topk(beam, dim=-1)
        summed = (top_lp + last_lp.reshape(n * beam, 1)).reshape(n, beam * beam)
        classes = top_cls.reshape(n, beam * beam)
        last_lp, idx = summed.topk(beam, dim=-1)
        note(summed)
        predictions.append(classes.gather(1, idx))
        bp = torch.div(idx, beam, rounding_mode='trunc')
        backpointers.append(bp)
        rows = _tap(hook, 'rows', (bp + base).reshape(-1), dict(t=t, beam=beam))
        state = State(state.h[rows], state.c[rows],
                      None if state.h_lm is None else state.h_lm[:, rows],
                      None if state.c_lm is None else state.c_lm[:, rows])
    rec = [predictions[-1].unsqueeze(2)]
    if backpointers:
        cur = backpointers[-1]
        for t in range(len(predictions) - 2, 0, -1):
            rec.append(predictions[t].gather(1, cur).unsqueeze(2))
            cur = backpointers[t - 1].gather(1, cur)
        rec.append(predictions[0].gather(1, cur).unsqueeze(2))
    all_pred = torch.cat(list(reversed(rec)), 2)
    scores, order = torch.sort(last_lp, dim=1, descending=True)
    tokens = all_pred.gather(1, order.unsqueeze(-1).expand_as(all_pred))
    return Search(tokens, scores, margin)


def rescore(feats, beam_tokens, sd, start, stop, mi=False, temperature=TEMPERATURE):
    """Teacher-forced score of given token rows: feats (n, k, F), beam_tokens (n, beam, T)
    -> (n, beam), the sum of the log-probs (MI scores under `mi`) of the row's tokens in step
    order.  It accumulates as the search does: nothing is added after the first <stop> (a
    finished beam only ever appends <stop> at cost 0)."""
    n, beam, length = beam_tokens.shape
    rows = n * beam
    toks = beam_tokens.reshape(rows, length)
    keys = project_keys(feats, sd)
    st = init_state(feats, sd, lm=mi)

    def ex(x, dim=0):
        return None if x is None else x.repeat_interleave(beam, dim=dim)

    state = State(ex(st.h), ex(st.c), ex(st.h_lm, 1), ex(st.c_lm, 1))
    cur = torch.full((rows,), start, dtype=torch.long)
    total = feats.new_zeros(rows)
    alive = torch.ones(rows, dtype=torch.bool)
    for t in range(length):
        p, _, state = step(feats, keys, cur, state, sd, temperature, None, t)
        cur = toks[:, t]
        picked = p[torch.arange(rows), cur]
        total = torch.where(alive, total + picked, total)
        alive = alive & (cur != stop)
    return total.view(n, beam)


def lm_score(inputs, sd, stop):
    """`LanguageModel.forward(inputs, reduce=True)` (lms.py:58-101) in the dtype of `sd`;
    inputs (R, L) begin with <start>.  The reference's off-by-one is kept: the target right
    after the first <stop> is still summed (as `oracle.milan_oracle.lm_score`)."""
    r, length = inputs.shape
    w = sd['lm.lstm.weight_hh_l0']
    h = w.new_zeros(lm_layers(sd), r, w.shape[1])
    c = torch.zeros_like(h)
    total = w.new_zeros(r)
    alive = w.new_ones(r)
    for t in range(length - 1):
        logp, h, c = lm_step(inputs[:, t], h, c, sd)
        total = total + alive * logp[torch.arange(r), inputs[:, t + 1]]
        alive = alive * (inputs[:, t] != stop).to(alive.dtype)
    return total


# ---- the dispatch, restated -----------------------------------------------------------
# csrc/decoder.hip: decoder_finalize / pack_linear / cat_linear (which weights have a
# split-f16 copy), step_core (the `fused` branch), lin / lstm_layer (the other branch),
# launch_attend, launch_context, launch_row_select, lm_split_ok.  csrc/gemm_plan.h:
# plan_launch for a Linear layer (1 x 1, no hint, no environment override, MILAN_PP =
# MILAN_PP128 = 1).
def fused(d):
    """step_core's `fused` branch under split_f16: every product has a split weight copy
    (K % 32 == 0 for q / gate / vocabulary: H; for the concatenated cell weight: E + F and
    H) and x can be produced in split format (E % 16, F % 8)."""
    return d.H % 32 == 0 and (d.E + d.F) % 32 == 0 and d.E % 16 == 0 and d.F % 8 == 0


def split_tile(N, K, K1=0):
    """Tile of a split-f16 Linear product whose weight has a split copy (K % 32 == 0)."""
    cin = K1 or K
    assert cin % 32 == 0 and (K - cin) % 32 == 0
    if N <= 64:
        assert not K1
        return 'split_256x64'
    pad256, pad128 = -N % 256, -N % 128
    if N % 256 == 0 or (N > 2048 and pad256 <= pad128):
        return 'pp32_256'
    return 'pp32_128'


def f32_tile(N):
    return 'f32_256x64' if N <= 64 else 'f32_128x128'


# tile -> family of hip.profile_read_kernels()
TILE_FAMILY = {'pp32_256': 'pp32_256', 'pp32_128': 'pp32_128', 'split_256x64': 'split_other',
               'f32_256x64': 'f32', 'f32_128x128': 'f32'}


def padded_columns(N, tile):
    return -N % {'pp32_256': 256, 'pp32_128': 128, 'f32_128x128': 128}.get(tile, 64)


def step_gemms(d, rows, precision, k=None):
    """(name, M, N, K, K1, tile, epilogue) of every product of one decoder step over `rows`
    rows; K1 > 0: a two-source product whose first source holds K1 of the K columns.  With
    `k` the hoisted key projection of `milan_step` (rows * k rows) comes first."""
    H, E, F_, A, V = d
    split = precision == 'split_f16'

    def one(name, M, N, K, epi, K1=0):
        if split and K % 32 == 0:
            return (name, M, N, K, K1, split_tile(N, K, K1), epi)
        return (name, M, N, K, K1, f32_tile(N), epi)

    out = []
    if k is not None:
        out.append(one('keys', rows * k, A, F_, 'bias'))
    out.append(one('q', rows, A, H, 'bias'))
    if split and fused(d):
        out.append(one('gate', rows, F_, H, 'bias_sigmul_split'))
        out.append(one('lstm', rows, 4 * H, E + F_ + H, 'lstm', K1=E + F_))
    else:
        out.append(one('gate', rows, F_, H, 'bias_sigmul'))
        cat = (E + F_) % 32 == 0 and H % 32 == 0   # cat_linear made a split copy
        if split and cat:
            inter = (4 * H) % 64 == 0 and H % 8 == 0
            out.append(one('lstm', rows, 4 * H, E + F_ + H, 'lstm' if inter else 'bias'))
        else:
            out.append(one('lstm_ih', rows, 4 * H, E + F_, 'bias'))
            out.append(one('lstm_hh', rows, 4 * H, H, 'bias_add'))
    out.append(one('vocab', rows, V, H, 'bias'))
    return out


def gemm(gemms, name):
    return next(g for g in gemms if g[0] == name)


def attend_path(k, A):
    return 'attend16' if k <= 16 and A <= 512 else 'attend'


def attend_grid(neurons, rpn):
    """attend16's gridDim.y and whether a wave walks more than one of its neuron's rows."""
    rs = (4096 + neurons * 4 - 1) // (neurons * 4)
    rs = max(1, min(rs, (rpn + 3) // 4))
    return rs, rpn > 4 * rs


def context_path(k, F_):
    """(register-resident features, column slices gridDim.y) of context_kernel."""
    return k <= 16, (F_ // 4 + 255) // 256


def row_select_path(V, k):
    """Kernel that turns logits into log-probs (k = 0) or the k best of a row."""
    if k > 256:
        return 'wide'
    return 'reg' if V <= 24 * 256 and (k <= 1 or k <= V) else 'lds'


def lm_split_ok(d, precision, layers=2):
    """The LM token step with every operand already in split format (H, E: the LM's)."""
    return (precision == 'split_f16' and 1 <= layers <= 2 and d.E % 32 == 0 and
            d.H % 32 == 0)


# ---- comparing two searches -------------------------------------------------------------
def beam_set_excuses(got_tokens, want_tokens, margins, tie, what=''):
    """Neurons whose beam SET (token rows, whatever their order) differs between two
    searches.  A set may differ only where the float64 select margin of the neuron is below
    `tie`; anything else is an assertion failure.  Returns the number of such neurons."""
    n, beam, length = want_tokens.shape
    got_tokens = got_tokens[:, :, :length]
    excuses = 0
    for i in range(n):
        got = {tuple(r.tolist()) for r in got_tokens[i]}
        want = {tuple(r.tolist()) for r in want_tokens[i]}
        if got == want:
            continue
        assert float(margins[i]) < tie, (
            f'{what}: neuron {i} beam set differs from the float64 search although its '
            f'smallest select margin is {float(margins[i]):.3g}; missing '
            f'{sorted(want - got)[:2]}')
        excuses += 1
    return excuses
