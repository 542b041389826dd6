"""Training-mode `LanguageModel.forward` through autograd (lms.TrainingForward over
milan_lm_forward_train / milan_lm_backward).

  * After `lm.requires_grad_(True); lm.train()` both `reduce` forms carry `grad_fn`
    and `backward()` fills `.grad` on the 4 * layers + 3 tensors; with the default
    `requires_grad=False` a training-mode call is the eval call, bit for bit.
  * Outputs and parameter gradients against float64 autograd of tests/lmref.py, from
    a random upstream gradient on the log-probs, on the scores with the default mask
    and on the scores with a random float mask; an edge table and seeded draws
    (MILAN_TRAIN_FUZZ_SEEDS=<n> widens them).  The bound is the float32 class of
    test_gpu_train_fuzz.py: per tensor max|hip - ref64| <= 128 max|ref32 - ref64| +
    1e-7 max|ref64|, per row of every weight gradient with 512, ref32 the same
    restatement in float32 on the CPU.  Every case prints the C it needs.
  * The fused `milan_lm_train_step` / `milan_lm_nll`, a user's AdamW loop against the
    float64 torch loop, an LM inside a Decoder.
  * Determinism, one backward per graph, `no_grad`, and no (B, L, V) tensor with
    `reduce=True`.
"""
import os
import random

import pytest
import torch
import torch.nn.functional as F

import lmref
import trainref
from milan_amd import decoders, encoders, hip, lang, lms, synthetic
from test_gpu_lm_train import names, random_state
from test_gpu_train_fuzz import C, C_ROW, FLOOR, LOGPROB_ATOL, lm_accepted, needed_c

pytestmark = pytest.mark.gpu

# the bound test_gpu_decoder_autograd.py puts on its scores (sums of log-probs)
SCORE_ATOL = 1e-3
FORMS = ('logprobs', 'scores', 'scores_masked')


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


def peek_seed(dev):
    """The seed the next training-mode forward draws, without consuming it."""
    gen = torch.cuda.default_generators[dev.index]
    state = gen.get_state()
    seed = int(torch.randint(2**62, (), device=dev, generator=gen))
    gen.set_state(state)
    return seed


def make_lm(v, e, h, layers, p, seed, dev=None, trainable=True):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(v - 4)), str.split, True, True,
                       True, True)
    model = lms.LanguageModel(idx, e, h, layers=layers, dropout=p)
    sd = random_state(v, e, h, layers, seed=seed)
    model.load_state_dict(sd)
    if dev is not None:
        model.to(dev)
    model.requires_grad_(trainable)
    model.train()
    return model, sd


def params_of(model):
    named = dict(model.named_parameters())
    return [named[n] for n in names(model.layers)]


def seq_batch(v, rows, length, seed, hot=False, pad_mid=False):
    """Sequences as `logp` indexes them: <start>, tokens, <stop>, <pad>...; ragged, a
    row that is all pad when rows > 2, <unk>.  hot: nine in ten tokens one id (7 %
    nv).  pad_mid: a <pad> among the tokens of every row that has three or more."""
    nv = v - 4
    start, stop, pad, unk = nv, nv + 1, nv + 2, nv + 3
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, length), pad, dtype=torch.long)
    for r in range(rows):
        if r == 1 and rows > 2 and not hot:
            continue
        x[r, 0] = start
        n = max(length - 2, 0) if hot else int(torch.randint(0, max(length - 1, 1), (),
                                                             generator=g))
        if hot:
            toks = torch.where(torch.rand(n, generator=g) < .9, 7 % nv,
                               torch.randint(0, min(nv, 2), (n,), generator=g))
        else:
            toks = torch.randint(0, nv, (n,), generator=g)
            if n > 3:
                toks[-1] = unk
        if pad_mid and n >= 3:
            toks[int(torch.randint(1, n - 1, (), generator=g))] = pad
        x[r, 1:n + 1] = toks
        if n + 1 < length:
            x[r, n + 1] = stop
    return x


def upstream(form, rows, length, v, seed, zero_rows=False):
    """(G for the log-probs or g for the scores, the token mask or None)."""
    g = torch.Generator().manual_seed(seed)
    if form == 'logprobs':
        up = torch.randn(rows, length, v, generator=g)
        if zero_rows:
            up.view(-1, v)[::2] = 0  # every other position: an all-zero upstream row
        return up, None
    up = torch.randn(rows, generator=g)
    if zero_rows:
        up[::2] = 0
    masks = torch.rand(rows, length - 1, generator=g) if form == 'scores_masked' else None
    return up, masks


def objective_of(form, inputs, up, masks, stop):
    def objective(lp):
        if form == 'logprobs':
            return lp, (lp * up.to(lp.dtype)).sum()
        token_masks = lmref.default_masks(inputs, stop) if masks is None else masks
        s = lmref.scores(lp, inputs, token_masks)
        return s, (s * up.to(lp.dtype)).sum()
    return objective


def class_needs(got, r64, r32, rows=None):
    """The C this tensor needs per tensor and per row (test_gpu_train_fuzz.py's
    check_tensor without the assertions, so that a case can print before it asserts)."""
    got = got.double().cpu()
    s = float(r64.abs().max()) if r64.numel() else 0.
    e_hip = float((got - r64).abs().max()) if r64.numel() else 0.
    e_32 = float((r32.double() - r64).abs().max()) if r64.numel() else 0.
    need, need_row = needed_c(e_hip, e_32, s), 0.
    if rows is not None:
        d_hip = rows(got - r64).abs().amax(1)
        d_32 = rows(r32.double() - r64).abs().amax(1)
        over = d_hip - FLOOR * s
        live = over > 0
        if bool(live.any()):
            need_row = float((over[live] / d_32[live]).max())
    return need, need_row


def check_against_references(tag, names_, got_out, got_grads, ref64, ref32, out_atol):
    """Print the worst needed C, then assert the class per tensor and per row, the
    absolute bound on the output, and finite gradients."""
    out64, g64 = ref64
    out32, g32 = ref32
    needs = [('output', class_needs(got_out, out64, out32)[0], 0.)]
    for name, got in zip(names_, got_grads):
        assert bool(torch.isfinite(got).all()), (tag, name, 'not finite')
        rows_of = (lambda t: t) if got.dim() == 2 else None
        needs.append((name, *class_needs(got, g64[name], g32[name], rows_of)))
    out_err = float((got_out.double().cpu() - out64).abs().max()) if out64.numel() else 0.
    wt, wr = max(needs, key=lambda x: x[1]), max(needs, key=lambda x: x[2])
    print(f'LMAUTOGRAD {tag}: tensor {wt[1]:.2f} {wt[0]} | row {wr[2]:.2f} {wr[0]} | '
          f'|output err| {out_err:.1e}')
    assert out_err <= out_atol, (tag, out_err)
    for name, need, need_row in needs:
        assert need <= C, (tag, name, need)
        assert need_row <= C_ROW, (tag, name, 'rows', need_row)
    return wt[1], wr[2]


def check_exact_zeros(tag, demb, inputs, v, pad):
    """The padding row and the rows of ids no input holds are exactly 0."""
    absent = torch.ones(v, dtype=torch.bool)
    absent[inputs.flatten()] = False
    absent[pad] = True
    assert not demb.cpu()[absent].any(), (tag, 'absent / pad rows not exactly 0')


def check_case(dev, case, seed, tag, form):
    v, e, h, layers, rows, length, p = (case[x] for x in
                                        ('V', 'E', 'H', 'layers', 'rows', 'L', 'p'))
    pad, stop = v - 2, v - 3
    model, sd = make_lm(v, e, h, layers, p, seed, dev)
    inputs = seq_batch(v, rows, length, seed + 1, case.get('hot', False),
                       case.get('pad_mid', False))
    up, masks = upstream(form, rows, length, v, seed + 2, case.get('zero_rows', False))
    gen = torch.cuda.default_generators[dev.index]
    before = gen.get_state()
    dseed = peek_seed(dev)
    x = inputs.to(dev)
    if form == 'logprobs':
        out = model(x)
    else:
        out = model(x, reduce=True, masks=None if masks is None else masks.to(dev))
    assert out.grad_fn is not None, tag
    drawn = not torch.equal(gen.get_state(), before)
    assert drawn == (p > 0 and layers > 1), (tag, 'seed drawn', drawn)
    (out * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    grads = [t.grad for t in params_of(model)]
    assert all(g is not None for g in grads), tag

    drop = [lms.dropout_mask(dseed, l, rows, length, h, p)
            for l in range(layers - 1)] if p and layers > 1 else None
    objective = objective_of(form, inputs, up, masks, stop)
    ref64 = lmref.run(sd, inputs, pad, layers, objective, drop, p)
    with trainref.fp32_reference():
        ref32 = lmref.run(sd, inputs, pad, layers, objective, drop, p, dtype=torch.float32)
    worst = check_against_references(tag, names(layers), out.detach(), grads, ref64, ref32,
                                     LOGPROB_ATOL if form == 'logprobs' else SCORE_ATOL)
    check_exact_zeros(tag, grads[0], inputs, v, pad)
    return inputs, worst


# ---- 1. the surface --------------------------------------------------------------
def test_training_forward_is_differentiable(dev):
    v, e, h, layers, rows, length = 61, 16, 32, 2, 9, 7
    model, _ = make_lm(v, e, h, layers, .5, 1, dev)
    inputs = seq_batch(v, rows, length, 2).to(dev)
    pad = v - 2
    assert len(params_of(model)) == 4 * layers + 3
    for reduce in (False, True):
        for t in params_of(model):
            t.grad = None
        dseed = peek_seed(dev)
        out = model(inputs, reduce=reduce)
        assert out.requires_grad and out.grad_fn is not None
        assert out.shape == ((rows,) if reduce else (rows, length, v))
        out.sum().backward()
        for name, t in zip(names(layers), params_of(model)):
            assert t.grad is not None and t.grad.shape == t.shape, name
            assert bool(torch.isfinite(t.grad).all()), name
        assert any(float(t.grad.abs().max()) > 0 for t in params_of(model))
        check_exact_zeros(f'reduce={reduce}', model.embedding.weight.grad, inputs.cpu(), v,
                          pad)
        # the binding overwrites: NaN-filled buffers come back finite, with the bits of
        # .grad (same seed)
        ctx = model._train_context(dev)
        params = [t.detach() for t in params_of(model)]
        targets = F.pad(inputs[:, 1:], (0, 1)) if reduce else None
        lp, picked, ws = ctx.lm_forward_train(params, inputs, .5, dseed, targets=targets,
                                              want_logprobs=not reduce)
        assert (lp is None) == reduce and (picked is None) == (not reduce)
        filled = [torch.full_like(t, float('nan')) for t in params]
        if reduce:
            dpicked = torch.ones_like(picked)
            dpicked[:, -1] = 0
            dpicked[:, :-1] *= lmref.default_masks(inputs.cpu(), v - 3).to(dev)
            ctx.lm_backward(params, filled, inputs, .5, dseed, None, dpicked, targets, ws)
        else:
            ctx.lm_backward(params, filled, inputs, .5, dseed, torch.ones_like(lp), None,
                            None, ws)
        for name, t, g in zip(names(layers), params_of(model), filled):
            assert bool(torch.isfinite(g).all()), name
            assert torch.equal(g, t.grad), name


def test_frozen_parameters_get_no_grad(dev):
    model, _ = make_lm(61, 16, 32, 2, 0., 3, dev, trainable=False)
    dict(model.named_parameters())['output.0.weight'].requires_grad_(True)
    out = model(seq_batch(61, 4, 6, 4).to(dev))
    out.sum().backward()
    for name, t in model.named_parameters():
        assert (t.grad is not None) == (name == 'output.0.weight'), name


# ---- 2. the default is unchanged -------------------------------------------------
def test_default_parameters_keep_the_inference_path(dev):
    model, _ = make_lm(61, 16, 32, 2, .5, 5, dev, trainable=False)
    inputs = seq_batch(61, 9, 7, 6).to(dev)
    masks = torch.rand(9, 6, generator=torch.Generator().manual_seed(7)).to(dev)
    state = torch.cuda.default_generators[dev.index].get_state()
    model.train()
    got = [model(inputs), model(inputs, reduce=True), model(inputs, reduce=True, masks=masks)]
    assert torch.equal(torch.cuda.default_generators[dev.index].get_state(), state)
    model.eval()
    want = [model(inputs), model(inputs, reduce=True), model(inputs, reduce=True, masks=masks)]
    for a, b in zip(got, want):
        assert a.grad_fn is None and not a.requires_grad
        assert torch.equal(a, b)


# ---- 3. float64 autograd ----------------------------------------------------------
EDGES = {
    'v5': dict(V=5, E=8, H=12, layers=1, rows=6, L=5, p=0.),
    'v63': dict(V=63, E=8, H=12, layers=2, rows=7, L=6, p=0.),
    'v65': dict(V=65, E=8, H=12, layers=1, rows=7, L=6, p=0.),
    # more than one pass of the 256-thread row loops, with a ragged tail
    'v1029': dict(V=1029, E=8, H=12, layers=2, rows=5, L=6, p=.5),
    'rows1_L1': dict(V=61, E=8, H=12, layers=1, rows=1, L=1, p=0.),
    # dh_{t-1}: K = 4H = 400 splits 224 + 176
    'h100': dict(V=61, E=16, H=100, layers=2, rows=64, L=5, p=0.),
    # dW_hh: K = 481 split at 256, inside the 20th sequence
    'rows37_L13': dict(V=61, E=16, H=32, layers=1, rows=37, L=13, p=0.),
    'layers4_p09': dict(V=61, E=16, H=20, layers=4, rows=9, L=7, p=.9),
    # one layer: no mask, and no seed is drawn
    'layers1_p05': dict(V=61, E=16, H=20, layers=1, rows=9, L=7, p=.5),
    'hot_id': dict(V=261, E=16, H=32, layers=1, rows=40, L=12, p=0., hot=True),
    'pad_mid': dict(V=61, E=16, H=20, layers=2, rows=9, L=9, p=.5, pad_mid=True),
    'zero_rows': dict(V=61, E=16, H=20, layers=2, rows=9, L=7, p=0., zero_rows=True),
}


def test_edge_table_reaches_its_branches():
    for name, want in (('h100', 'partial_last'), ('rows37_L13', 'mid_sequence')):
        c = EDGES[name]
        gemms = trainref.lm_gemms(c['E'], c['H'], c['V'], c['layers'], c['rows'], c['L'])
        assert want in trainref.split_branches(gemms), name
    assert EDGES['v1029']['V'] > 4 * 256 and EDGES['v1029']['V'] % 256


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', list(EDGES))
def test_gradients_match_autograd_float64(dev, name, form):
    case = EDGES[name]
    inputs, _ = check_case(dev, case, seed=len(name), tag=f'{name} {form}', form=form)
    pad = case['V'] - 2
    if name == 'hot_id':
        assert int(torch.bincount(inputs.flatten()).max()) > 300
    if name == 'pad_mid':  # a pad with tokens on both sides
        mid = (inputs[:, 1:-1] == pad) & (inputs[:, :-2] != pad) & (inputs[:, 2:] != pad) \
            & (inputs[:, 2:] != pad - 1)
        assert bool(mid.any())


@pytest.mark.parametrize('case', ['v1029', 'h100', 'pad_mid'])
def test_both_upstreams_through_the_binding(dev, case):
    """dlogprobs and dpicked in one call: the float32 class against float64 autograd,
    and the sum of the two single-input runs within the same class."""
    c = EDGES[case]
    v, e, h, layers, rows, length, p = (c[x] for x in
                                        ('V', 'E', 'H', 'layers', 'rows', 'L', 'p'))
    pad = v - 2
    sd = random_state(v, e, h, layers, seed=11)
    inputs = seq_batch(v, rows, length, 12, pad_mid=c.get('pad_mid', False))
    g = torch.Generator().manual_seed(13)
    glp = torch.randn(rows, length, v, generator=g)
    gp = torch.randn(rows, length, generator=g)
    targets = torch.randint(0, v, (rows, length), generator=g)
    dims = hip.make_dims({f'lm.{k}': t for k, t in sd.items()}, v - 4)
    ctx = hip.Context(dims, {}, dev, finalize=False)
    params = [t.to(dev).contiguous() for t in sd.values()]
    dseed = 0xa070_1a00 + len(case)
    x, tg = inputs.to(dev), targets.to(dev)

    def run(dlp, dpk):
        lp, picked, ws = ctx.lm_forward_train(params, x, p, dseed, targets=tg)
        grads = [torch.full_like(t, float('nan')) for t in params]
        ctx.lm_backward(params, grads, x, p, dseed, dlp, dpk, tg if dpk is not None else None,
                        ws)
        torch.cuda.synchronize()
        return lp.cpu(), picked.cpu(), [t.cpu() for t in grads]

    lp, picked, both = run(glp.to(dev), gp.to(dev))
    _, _, only_lp = run(glp.to(dev), None)
    _, _, only_pk = run(None, gp.to(dev))
    assert torch.equal(picked, lp.gather(2, targets.unsqueeze(-1)).squeeze(-1))
    with pytest.raises(ValueError, match='neither'):
        ctx.lm_backward(params, both, x, p, dseed, None, None, None,
                        torch.empty(1, dtype=torch.uint8, device=dev))

    def objective(out):
        pk = out.gather(2, targets.unsqueeze(-1)).squeeze(-1)
        return out, (out * glp.to(out.dtype)).sum() + (pk * gp.to(out.dtype)).sum()

    drop = [lms.dropout_mask(dseed, l, rows, length, h, p)
            for l in range(layers - 1)] if p and layers > 1 else None
    ref64 = lmref.run(sd, inputs, pad, layers, objective, drop, p)
    with trainref.fp32_reference():
        ref32 = lmref.run(sd, inputs, pad, layers, objective, drop, p, dtype=torch.float32)
    check_against_references(f'binding {case} both', names(layers), lp, both, ref64, ref32,
                             LOGPROB_ATOL)
    check_exact_zeros(case, both[0], inputs, v, pad)
    # both = dlogprobs-only + dpicked-only, within the class of the combined objective
    worst = 0.
    for name, b, a1, a2 in zip(names(layers), both, only_lp, only_pk):
        r64, r32 = ref64[1][name], ref32[1][name]
        gap = float((b.double() - (a1.double() + a2.double())).abs().max())
        need = needed_c(gap, float((r32.double() - r64).abs().max()), float(r64.abs().max()))
        worst = max(worst, need)
        assert need <= C, (case, name, need)
    print(f'LMAUTOGRAD binding {case}: both vs sum of singles needs C {worst:.2f}')
    ctx.close()


# ---- 4. the fused step ---------------------------------------------------------------
@pytest.mark.parametrize('v,e,h,layers,rows,length,p', [(61, 16, 32, 2, 9, 7, .5),
                                                        (261, 16, 100, 2, 64, 5, 0.)])
def test_nll_loss_agrees_with_fused_step(dev, v, e, h, layers, rows, length, p):
    from test_gpu_train_fuzz import lm_batch
    pad = v - 2
    model, sd = make_lm(v, e, h, layers, p, 21, dev)
    inputs, targets = lm_batch(v, rows, length, 22)
    x, tg = inputs.to(dev), targets.to(dev)
    dseed = peek_seed(dev) if p else 0
    lp = model(x)
    loss = F.nll_loss(lp.reshape(-1, v), tg.reshape(-1), ignore_index=pad)
    loss.backward()
    got = [t.grad.cpu() for t in params_of(model)]
    params = [t.detach() for t in params_of(model)]
    fused = [torch.empty_like(t) for t in params]
    ctx = model._train_context(dev)
    terms = ctx.lm_train_step(params, fused, x, tg, p, dseed).cpu()
    drop = [lms.dropout_mask(dseed, l, rows, length, h, p)
            for l in range(layers - 1)] if p else None
    _, _, g64 = trainref.lm_loss(sd, inputs, targets, pad, layers, drop, p)
    with trainref.fp32_reference():
        _, _, g32 = trainref.lm_loss(sd, inputs, targets, pad, layers, drop, p,
                                     dtype=torch.float32)
    worst = 0.
    for name, a, b in zip(names(layers), got, fused):
        gap = float((a.double() - b.double().cpu()).abs().max())
        need = needed_c(gap, float((g32[name].double() - g64[name]).abs().max()),
                        float(g64[name].abs().max()))
        worst = max(worst, need)
    rel = abs(float(loss) - float(terms[0] / terms[1])) / float(terms[0] / terms[1])
    print(f'LMAUTOGRAD vs train_step p={p}: needs C {worst:.2f}, loss rel {rel:.1e}')
    assert worst <= C, worst
    assert rel <= 1e-6, rel
    if not p:
        nll = ctx.lm_nll(params, x, tg).cpu()
        want = float(nll[0] / nll[1])
        assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)


# ---- 5. determinism and lifetime -----------------------------------------------------
def run_graph(model, inputs, up, dev, state, reduce=False):
    torch.cuda.default_generators[dev.index].set_state(state)
    for t in model.parameters():
        t.grad = None
    out = model(inputs, reduce=reduce)
    (out * up).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), [t.grad.clone() for t in params_of(model)]


def test_deterministic_and_one_backward(dev):
    v, e, h, layers, rows, length = 1029, 32, 100, 2, 37, 13
    model, _ = make_lm(v, e, h, layers, .5, 31, dev)
    inputs = seq_batch(v, rows, length, 32).to(dev)
    g = torch.Generator().manual_seed(33)
    up = torch.randn(rows, length, v, generator=g).to(dev)
    ups = torch.randn(rows, generator=g).to(dev)
    state = torch.cuda.default_generators[dev.index].get_state()
    for reduce, u in ((False, up), (True, ups)):
        out1, g1 = run_graph(model, inputs, u, dev, state, reduce)
        out2, g2 = run_graph(model, inputs, u, dev, state, reduce)
        for a, b in zip([out1] + g1, [out2] + g2):
            assert torch.equal(a, b)
    out = model(inputs)
    loss = (out * up).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='already backpropagated'):
        loss.backward()


def test_no_grad_is_still_the_training_forward(dev):
    model, _ = make_lm(61, 16, 32, 2, .5, 41, dev)
    inputs = seq_batch(61, 9, 7, 42).to(dev)
    gen = torch.cuda.default_generators[dev.index]
    state = gen.get_state()
    with_grad = model(inputs)
    gen.set_state(state)
    with torch.no_grad():
        without = model(inputs)
        gen.set_state(state)
        scores = model(inputs, reduce=True)
    assert without.grad_fn is None and not without.requires_grad
    assert scores.grad_fn is None
    assert torch.equal(without, with_grad.detach())
    model.eval()
    evaluated = model(inputs)
    assert evaluated.grad_fn is None
    assert not torch.equal(without, evaluated)


def test_reduce_never_allocates_batch_length_vocab(dev):
    v, e, h, layers, rows, length = 1029, 8, 8, 1, 64, 32
    model, _ = make_lm(v, e, h, layers, 0., 51, dev)
    inputs = seq_batch(v, rows, length, 52).to(dev)
    blv = rows * length * v * 4
    ctx = model._train_context(dev)
    ws = int(ctx.lib.milan_lm_grad_workspace_bytes(ctx._h, rows, length))
    assert ws < 1.5 * blv  # one (B, L, V) tensor would dominate what is left
    peaks = {}
    for reduce in (True, False):
        for t in model.parameters():
            t.grad = None
        model(inputs, reduce=reduce).sum().backward()  # (allocator warm, grads freed)
        for t in model.parameters():
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        model(inputs, reduce=reduce).sum().backward()
        torch.cuda.synchronize()
        peaks[reduce] = torch.cuda.max_memory_allocated(dev) - base
    print(f'LMAUTOGRAD peak over baseline: reduce=True {peaks[True] / blv:.2f} x (B, L, V), '
          f'reduce=False {peaks[False] / blv:.2f} x; workspace {ws / blv:.2f} x')
    # the workspace holds the logits (one (B, L, V) of activations); nothing of that
    # size beside it
    assert peaks[True] < ws + blv // 2, peaks
    assert peaks[False] >= ws + blv, peaks  # (the check can tell the difference)


# ---- 6. seeded draws -----------------------------------------------------------------
WIDE = os.environ.get('MILAN_TRAIN_FUZZ_SEEDS')
SEEDS = int(WIDE) if WIDE else 30


def draw(seed):
    r = random.Random(0x1a070000 + seed)
    while True:
        d = dict(V=r.choice([5, 7, 63, 65, 257, 1029]), E=r.choice([3, 4, 12, 36, 68, 260]),
                 H=r.choice([4, 20, 30, 36, 68, 100]), layers=r.randint(1, 4),
                 rows=r.choice([1, 3, 17, 37, 70]), L=r.choice([1, 2, 5, 13, 20]),
                 p=r.choice([0., 0., .3, .9]), hot=r.random() < .2,
                 pad_mid=r.random() < .3, zero_rows=r.random() < .2, form=r.choice(FORMS))
        if lm_accepted(d):
            return d


@pytest.mark.parametrize('seed', range(SEEDS))
def test_fuzz(dev, seed):
    d = draw(seed)
    check_case(dev, d, seed=400 + seed, tag=f'seed {seed} {d}', form=d['form'])


# ---- 7. a user's loop ----------------------------------------------------------------
def test_own_adamw_loop_tracks_float64(dev):
    v, e, h, layers, rows, length = 61, 16, 32, 2, 16, 9
    from test_gpu_train_fuzz import lm_batch
    pad = v - 2
    model, sd = make_lm(v, e, h, layers, 0., 61, dev)
    batches = [lm_batch(v, rows, length, 62 + i) for i in range(3)]
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-2)
    got = []
    for inputs, targets in batches:
        lp = model(inputs.to(dev))
        loss = F.nll_loss(lp.reshape(-1, v), targets.to(dev).reshape(-1), ignore_index=pad)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        got.append(float(loss))
    w = trainref._leaves(sd, torch.float64, 'cpu')
    reference = torch.optim.AdamW(list(w.values()), lr=1e-2)
    want = []
    for inputs, targets in batches:
        lp = lmref.logprobs(w, inputs, pad, layers)
        loss = F.nll_loss(lp.reshape(-1, v), targets.reshape(-1), ignore_index=pad)
        loss.backward()
        reference.step()
        reference.zero_grad()
        want.append(float(loss))
    rel = max(abs(a - b) / abs(b) for a, b in zip(got, want))
    print(f'LMAUTOGRAD own loop: losses {got} vs {want}, max relative gap {rel:.2e}')
    assert want[2] < want[0]  # (it trains)
    assert rel <= 1e-4, rel
    gap = max(float((t.detach().cpu().double() - w[n].detach()).abs().max())
              for n, t in zip(names(layers), params_of(model)))
    print(f'LMAUTOGRAD own loop: max |param - float64| {gap:.2e}')


# ---- 8. inside a Decoder -------------------------------------------------------------
def test_lm_of_a_decoder_trains_and_rerank_follows(dev):
    nv = 40
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(nv)), str.split, True, True,
                       True, True)
    enc = encoders.PyramidConvEncoder('resnet50', width=16, pretrained=False)
    lm = lms.LanguageModel(idx, 16, 32, layers=2, dropout=.5)
    dec = decoders.Decoder(idx, enc, lm, embedding_size=16, hidden_size=32, length=8,
                           beam_size=4)
    sd = synthetic.milan_state_dict(nv + 4, 'resnet50', seed=11, width=16, hidden_size=32,
                                    embedding_size=16, lm_hidden_size=32,
                                    lm_embedding_size=16)
    dec.load_state_dict(sd, strict=True)
    dec.to(dev)
    feats = torch.randn(3, 5, dec.encoder.feature_shape[0],
                        generator=torch.Generator().manual_seed(1)).abs().to(dev)
    before = dec(feats, encode=False, strategy='rerank').scores.cpu()

    dec.lm.requires_grad_(True)
    dec.lm.train()
    inputs = seq_batch(nv + 4, 12, 8, 71).to(dev)
    optimizer = torch.optim.AdamW(dec.lm.parameters(), lr=5e-2)
    for _ in range(2):
        scores = dec.lm(inputs, reduce=True)
        assert scores.grad_fn is not None
        (-scores.mean()).backward()
        optimizer.step()
        optimizer.zero_grad()
    assert not torch.equal(dec.state_dict()['lm.output.0.weight'].cpu(), sd['lm.output.0.weight'])
    # the decoder's own rules in training mode are untouched
    dec.train()
    with pytest.raises(ValueError, match='while training'):
        dec(feats, encode=False, strategy='rerank')
    dec.eval()
    assert not dec.lm.training
    after = dec(feats, encode=False, strategy='rerank')
    assert not torch.allclose(after.scores.cpu(), before)
    # ... and they are the updated weights': a fresh decoder loaded with them agrees
    fresh = decoders.Decoder(idx, encoders.PyramidConvEncoder('resnet50', width=16,
                                                              pretrained=False),
                             lms.LanguageModel(idx, 16, 32, layers=2, dropout=.5),
                             embedding_size=16, hidden_size=32, length=8, beam_size=4)
    fresh.load_state_dict({k: t.detach().cpu() for k, t in dec.state_dict().items()})
    fresh.to(dev)
    want = fresh(feats, encode=False, strategy='rerank')
    assert torch.equal(after.scores, want.scores) and torch.equal(after.tokens, want.tokens)
