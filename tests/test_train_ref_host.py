"""The training references of tests/trainref.py, pinned on the CPU (no GPU):

  * the decoder restatement against the reference's own autograd batch
    (make_golden_decoder_fit.py: batch_grads, batch_nll, batch_reg);
  * the LM restatement against autograd through nn.Embedding / nn.LSTM /
    nn.Linear loaded with the parameters `lms.lm()` initialises, at float64,
    with and without inter-layer dropout;
  * the edge table of test_gpu_train_fuzz.py reaches every branch of the
    restated split planner it is there for.
"""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import trainref
from milan_amd import decoders, lms
from test_gpu_decoder_train import (META as DEC_META, IdentityEncoder, corpus_dataset,
                                    golden_features, grad_scale, tokenize)
from test_gpu_lm_train import META as LM_META, random_batch
from test_gpu_train_fuzz import AUTOGRAD_EDGES, DECODER_EDGES, LM_EDGES


# The reference computed its batch in float32 on the CPU, in a different order of
# operations: agreement is float32 rounding.  Measured worst gradient error 4.5e-7 x
# max|grad| of its tensor (attend.key_to_hidden.weight), NLL and regulariser within
# 4.2e-8 relative: the bounds are ~9x and ~24x that.
DEC_GOLDEN_GRAD_RTOL, DEC_GOLDEN_LOSS_RTOL = 4e-6, 1e-6


def test_decoder_restatement_matches_reference_batch():
    from conftest import GOLDEN_DIR
    golden = torch.load(GOLDEN_DIR / 'reference_goldens_decoder_fit.pt')
    dims = DEC_META['dims']
    torch.manual_seed(7)
    dec = decoders.decoder(corpus_dataset(), IdentityEncoder(dims['F']),
                           indexer_kwargs=dict(tokenize=tokenize),
                           embedding_size=dims['embedding_size'],
                           hidden_size=dims['hidden_size'], dropout=0.)
    for name in decoders.TRAIN_PARAMS:
        assert torch.equal(dec.state_dict()[name], golden['init'][name])
    w = {n: dec.state_dict()[n] for n in decoders.TRAIN_PARAMS}
    feats = golden_features()[golden['batch_rows']]
    targets = golden['batch_targets']
    rows, k = feats.shape[:2]
    total, count, regsum, grads = trainref.decoder_loss(
        w, feats, targets, dec.indexer.start_index, dec.indexer.pad_index,
        dtype=torch.float32)
    nll_rel = abs(total / count - float(golden['batch_nll'])) / float(golden['batch_nll'])
    reg_rel = abs(regsum / (rows * k) - float(golden['batch_reg'])) / \
        float(golden['batch_reg'])
    worst, where = 0., None
    for name in decoders.TRAIN_PARAMS:
        err = float((grads[name] - golden['batch_grads'][name]).abs().max())
        rel = err / grad_scale(name, golden['batch_grads'])
        if rel > worst:
            worst, where = rel, name
    print(f'decoder restatement vs reference batch: nll rel {nll_rel:.1e}, reg rel '
          f'{reg_rel:.1e}, worst grad err / max|grad| {worst:.2e} ({where})')
    assert nll_rel <= DEC_GOLDEN_LOSS_RTOL and reg_rel <= DEC_GOLDEN_LOSS_RTOL
    assert worst <= DEC_GOLDEN_GRAD_RTOL, (where, worst)


def module_loss(model, inputs, targets, masks, p):
    """Autograd through the reference's modules in float64: nn.Embedding
    (padding_idx), nn.LSTM (one multi-layer module without dropout, else one per
    layer with the explicit masks between), nn.Linear, NLLLoss(ignore pad)."""
    sd = {k: t.double() for k, t in model.state_dict().items()}
    v, e, h, layers = len(model.indexer), model.embedding_size, model.hidden_size, \
        model.layers
    pad = model.indexer.pad_index
    emb = nn.Embedding(v, e, padding_idx=pad).double()
    out = nn.Linear(h, v).double()
    if masks is None:
        lstms = [nn.LSTM(e, h, num_layers=layers, batch_first=True).double()]
        lstms[0].load_state_dict({k[5:]: t for k, t in sd.items() if k.startswith('lstm.')})
    else:
        lstms = []
        for l in range(layers):
            m = nn.LSTM(e if l == 0 else h, h, batch_first=True).double()
            m.load_state_dict({f'{n}_l0': sd[f'lstm.{n}_l{l}'] for n in
                               ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')})
            lstms.append(m)
    with torch.no_grad():
        emb.weight.copy_(sd['embedding.weight'])
        out.weight.copy_(sd['output.0.weight'])
        out.bias.copy_(sd['output.0.bias'])
    x = emb(inputs)
    for l, m in enumerate(lstms):
        x, _ = m(x)
        if masks is not None and l < layers - 1:
            x = x * masks[l].double() / (1 - p)
    lp = F.log_softmax(out(x), -1)
    total = F.nll_loss(lp.reshape(-1, v), targets.reshape(-1), ignore_index=pad,
                       reduction='sum')
    count = int((targets != pad).sum())
    (total / count).backward()
    grads = {'embedding.weight': emb.weight.grad, 'output.0.weight': out.weight.grad,
             'output.0.bias': out.bias.grad}
    for l in range(layers):
        m, sub = (lstms[0], l) if masks is None else (lstms[l], 0)
        for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            grads[f'lstm.{n}_l{l}'] = getattr(m, f'{n}_l{sub}').grad
    return float(total.detach()), count, grads


@pytest.mark.parametrize('layers,p', [(1, 0.), (2, 0.), (3, .5), (2, .9)])
def test_lm_restatement_matches_torch_modules_float64(layers, p):
    dataset = [(i, None, None, None, ann) for i, ann in enumerate(LM_META['corpus'])]
    torch.manual_seed(3 + layers)
    model = lms.lm(dataset, indexer_kwargs=dict(tokenize=tokenize), embedding_size=12,
                   hidden_size=20, layers=layers, dropout=p)
    v, pad = len(model.indexer), model.indexer.pad_index
    assert pad == v - 2
    inputs, targets = random_batch(v, 6, 9, seed=layers)
    masks = None
    if p:
        masks = [lms.dropout_mask(77, l, 6, 9, 20, p) for l in range(layers - 1)]
    want_sum, want_count, want = module_loss(model, inputs, targets, masks, p)
    got_sum, got_count, got = trainref.lm_loss(model.state_dict(), inputs, targets, pad,
                                               layers, masks, p)
    assert got_count == want_count
    assert got_sum == pytest.approx(want_sum, rel=1e-12)
    assert set(got) == set(want)
    for name, g in want.items():
        err = float((got[name] - g).abs().max())
        assert err <= 1e-12 * float(g.abs().max()) + 1e-15, (name, err)


# ---- the edge table reaches the planner's branches --------------------------------
def lm_branches(case):
    gemms = trainref.lm_gemms(case['E'], case['H'], case['V'], case['layers'],
                              case['rows'], case['L'])
    seen = trainref.split_branches(gemms)
    rows, length = case['rows'], case['L']
    if any(trainref.colsum_chunks(r) > 1 for _, r, _ in
           trainref.lm_colsums(case['H'], case['V'], case['layers'], rows, length)):
        seen.add('colsum_chunks')
    if rows * length > 256:
        seen.add('embed_N>256')
    if case['E'] > 256:
        seen.add('embed_E>256')
    return seen


def decoder_branches(case):
    gemms = trainref.decoder_gemms(case['F'], case['H'], case['E'], case['A'], case['V'],
                                   case['rows'], case['k'], case['L'])
    seen = trainref.split_branches(gemms)
    if any(trainref.colsum_chunks(r) > 1 for _, r, _ in trainref.decoder_colsums(
            case['F'], case['H'], case['A'], case['V'], case['rows'], case['k'], case['L'])):
        seen.add('colsum_chunks')
    if case['rows'] * case['L'] > 256:
        seen.add('embed_N>256')
    if case['E'] > 256:
        seen.add('embed_E>256')
    seen |= {f'k={case["k"]}'} & {'k=1', 'k=64'}
    if case['A'] > 256:
        seen.add('A>256')
    if case['F'] > 256:
        seen.add('F>256')
    return seen


def test_planner_restatement_known_shapes():
    # the two shapes the issue worked out by hand
    assert trainref.plan_splits(128, 100, 400) == (2, 224)  # dh_{t-1} at H = 100
    s, kc = trainref.plan_splits(128, 32, 37 * 13)           # dW_hh, rows 37, L 13
    assert (s, kc) == (2, 256) and kc // 13 == 19 and kc % 13  # inside the 20th sequence
    assert trainref.plan_splits(64, 64, 255) == (1, 256)
    assert trainref.colsum_chunks(64) == 1 and trainref.colsum_chunks(65) == 2
    assert trainref.colsum_chunks(10**6) == 64


def test_edge_table_reaches_every_branch():
    lm = set().union(*(lm_branches(c) for c in LM_EDGES.values()))
    dec = set().union(*(decoder_branches(c) for c in DECODER_EDGES.values()))
    auto = set().union(*(decoder_branches(c) for c in AUTOGRAD_EDGES.values()))
    for branch in ('partial_last', 'mid_sequence', 'colsum_chunks', 'embed_N>256',
                   'embed_E>256'):
        assert branch in lm, branch
    for branch in ('partial_last', 'colsum_chunks', 'embed_N>256', 'k=1', 'k=64', 'A>256',
                   'F>256'):
        assert branch in dec, branch
    assert {'k=1', 'k=64', 'F>256'} <= auto
    # the named cases reach what their names say
    assert 'partial_last' in trainref.split_branches(
        [g for g in trainref.lm_gemms(**{x: LM_EDGES['h100'][x] for x in
                                         ('E', 'H', 'V', 'layers', 'rows', 'L')})
         if g[0].startswith('dh_prev')])
    assert 'mid_sequence' in trainref.split_branches(
        [g for g in trainref.lm_gemms(**{x: LM_EDGES['rows37_L13'][x] for x in
                                         ('E', 'H', 'V', 'layers', 'rows', 'L')})
         if g[0].startswith('dW_hh')])
    # the default `fit` shape splits its grouped GEMMs on sequence boundaries
    # (dW_hh: K = 2048 in 2 x 1024, L = 16): the edge above is the one inside
    assert 'split' in lm_branches(LM_EDGES['fit_default'])
    assert 'mid_sequence' not in lm_branches(LM_EDGES['fit_default'])
