"""Training-mode teacher forcing through autograd (decoders.TeacherForced over
milan_decoder_forward_train / milan_decoder_backward).

  * `Decoder.forward` in training mode with a tensor strategy returns outputs
    with `grad_fn`, and `backward()` fills `.grad` on the 19 decoder tensors.
  * Outputs, parameter gradients and the feature gradient against float64
    autograd of a torch restatement of the teacher-forced forward, from random
    upstream gradients on the log-probs, the attentions or both, with and
    without dropout, at the goldens' and the benchmark's dims.
  * The reference's `process` loss built on the outputs: the golden batch, the
    fused `milan_decoder_train_step`, and a user's own loop that reproduces the
    reference's `fit` run.
  * A foreign torch Encoder receives the feature gradient.
  * Determinism, one backward per graph, a private workspace, and eval mode
    unchanged.
"""
import subprocess
import sys

import pytest
import torch
from torch import nn

import trainref
from conftest import REPO
from milan_amd import decoders, encoders, hip, lms, training
from test_gpu_decoder_train import (META, NOISE_ONLY, corpus_dataset,
                                    golden_decoder, golden_features, grad_scale,
                                    make_decoder, random_batch)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


@pytest.fixture(scope='module')
def golden():
    from conftest import GOLDEN_DIR
    out = torch.load(GOLDEN_DIR / 'reference_goldens_decoder_fit.pt')
    out['features'] = golden_features()
    return out


def peek_seed(dev):
    """The seed the next training-mode forward draws (as Decoder.fit does),
    without consuming it."""
    gen = torch.cuda.default_generators[dev.index]
    state = gen.get_state()
    seed = int(torch.randint(2**62, (), device=dev, generator=gen))
    gen.set_state(state)
    return seed


def params_of(dec):
    named = dict(dec.named_parameters())
    return [named[n] for n in decoders.TRAIN_PARAMS]


def process_loss(out, targets, pad, reg_weight=1.):
    """The reference's `process` (decoders.py:990-1022) on a DecoderOutput."""
    nll = nn.NLLLoss(ignore_index=pad)(out.predictions.permute(0, 2, 1), targets)
    reg = ((1 - out.attentions.sum(dim=1))**2).mean()
    return nll, reg, nll + reg_weight * reg


GRAD_RTOL = 1e-5


def worst_grad(got, want, scale_of):
    """max over tensors of max|got - want| / max|want| (scale_of: name -> scale)."""
    worst, where = 0., None
    for name in want:
        err = float((got[name].double().cpu() - want[name].cpu()).abs().max())
        rel = err / max(scale_of(name), 1e-30)
        if rel > worst:
            worst, where = rel, name
    return worst, where


def test_training_forward_is_differentiable(dev):
    v, fs, hsz, emb, rows, k, length = 60, 64, 32, 16, 9, 15, 7
    dec = make_decoder(v - 4, fs, hsz, emb, seed=1).to(dev)
    dec.dropout = .5
    dec.train()
    feats, targets = random_batch(v, rows, k, fs, length, seed=2)
    out = dec(feats.to(dev), length=length, strategy=targets.to(dev), mi=False)
    assert out.predictions.requires_grad and out.predictions.grad_fn is not None
    assert out.attentions.requires_grad and out.scores.requires_grad
    assert out.predictions.shape == (rows, length, v)
    assert out.attentions.shape == (rows, length, k)
    assert torch.equal(out.tokens.cpu(), targets)
    _, _, loss = process_loss(out, targets.to(dev), v - 2)
    loss.backward()
    for name, p in zip(decoders.TRAIN_PARAMS, params_of(dec)):
        assert p.grad is not None and p.grad.shape == p.shape, name
        assert bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for p in params_of(dec))


CASES = {
    # name: (vocab, F, H, E, rows, k, L)
    'golden_dims': (60, 64, 32, 16, 9, 15, 7),
    'bench_dims': (5004, 3904, 512, 128, 64, 15, 16),
}


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('p', [0., .5])
@pytest.mark.parametrize('upstream', ['predictions', 'attentions', 'both'])
def test_gradients_match_autograd_float64(dev, case, p, upstream):
    v, fs, hsz, emb, rows, k, length = CASES[case]
    dec = make_decoder(v - 4, fs, hsz, emb, seed=v + fs).to(dev)
    dec.dropout = p
    dec.train()
    feats, targets = random_batch(v, rows, k, fs, length, seed=rows + length)
    g = torch.Generator().manual_seed(length + int(10 * p))
    glp = torch.randn(rows, length, v, generator=g)
    gatt = torch.randn(rows, length, k, generator=g)
    use_lp, use_att = upstream in ('predictions', 'both'), upstream in ('attentions', 'both')

    seed = peek_seed(dev)
    x = feats.to(dev).requires_grad_()
    out = dec(x, length=length, strategy=targets.to(dev), mi=False)
    loss = 0.
    if use_lp:
        loss = loss + (out.predictions * glp.to(dev)).sum()
    if use_att:
        loss = loss + (out.attentions * gatt.to(dev)).sum()
    loss.backward()
    got = {n: t.grad for n, t in zip(decoders.TRAIN_PARAMS, params_of(dec))}

    mask = lms.decoder_dropout_mask(seed, rows, length, hsz, p).to(dev) if p else None
    w = {n: t.detach().double().requires_grad_()
         for n, t in zip(decoders.TRAIN_PARAMS, params_of(dec))}
    x64 = feats.to(dev).double().requires_grad_()
    lp, att = trainref.decoder_forward(w, x64, targets.to(dev), v - 4, mask, p)
    want_loss = 0.
    if use_lp:
        want_loss = want_loss + (lp * glp.to(dev).double()).sum()
    if use_att:
        want_loss = want_loss + (att * gatt.to(dev).double()).sum()
    want_loss.backward()
    # (attentions alone do not reach the output layer: its gradient is exactly 0)
    want = {n: torch.zeros_like(t) if t.grad is None else t.grad for n, t in w.items()}

    lp_err = float((out.predictions.detach().double() - lp.detach()).abs().max())
    att_err = float((out.attentions.detach().double() - att.detach()).abs().max())
    worst, where = worst_grad(got, want, lambda n: grad_scale(n, want))
    dscale = float(x64.grad.abs().max())
    df_rel = float((x.grad.double() - x64.grad).abs().max()) / max(dscale, 1e-30)
    print(f'{case} p={p} {upstream}: |log-prob err| {lp_err:.1e}, |attention err| '
          f'{att_err:.1e}, worst grad err / max|grad| {worst:.2e} ({where}), '
          f'dF {df_rel:.2e}')
    assert lp_err <= 1e-5 and att_err <= 1e-6, (lp_err, att_err)
    assert worst <= GRAD_RTOL, (where, worst)
    assert df_rel <= GRAD_RTOL, df_rel


def test_reference_batch_process_loss(dev, golden):
    model = golden_decoder().to(dev)
    model.train()
    feats = golden['features'][golden['batch_rows']].to(dev)
    targets = golden['batch_targets'].to(dev)
    pad = model.indexer.pad_index
    out = model(feats, length=targets.shape[1], strategy=targets, mi=False)
    nll, reg, loss = process_loss(out, targets, pad)
    loss.backward()
    nll_rel = abs(float(nll) - float(golden['batch_nll'])) / float(golden['batch_nll'])
    reg_rel = abs(float(reg) - float(golden['batch_reg'])) / float(golden['batch_reg'])
    got = {n: t.grad for n, t in zip(decoders.TRAIN_PARAMS, params_of(model))}
    want = {n: golden['batch_grads'][n].double() for n in decoders.TRAIN_PARAMS}
    worst, where = worst_grad(got, want, lambda n: grad_scale(n, golden['batch_grads']))
    print(f'reference batch: nll rel {nll_rel:.1e}, reg rel {reg_rel:.1e}, worst grad '
          f'err / max|grad| {worst:.2e} ({where})')
    assert nll_rel <= 1e-6 and reg_rel <= 1e-6, (nll_rel, reg_rel)
    assert worst <= GRAD_RTOL, (where, worst)


@pytest.mark.parametrize('case', list(CASES))
def test_process_loss_agrees_with_fused_step(dev, case):
    v, fs, hsz, emb, rows, k, length = CASES[case]
    dec = make_decoder(v - 4, fs, hsz, emb, seed=3).to(dev)
    dec.dropout = .5
    dec.train()
    feats, targets = random_batch(v, rows, k, fs, length, seed=6)
    feats, targets = feats.to(dev), targets.to(dev)
    seed = peek_seed(dev)
    out = dec(feats, length=length, strategy=targets, mi=False)
    nll, reg, loss = process_loss(out, targets, v - 2)
    loss.backward()
    params = [p.detach() for p in params_of(dec)]
    grads = [torch.empty_like(p) for p in params]
    terms = dec._train_context().decoder_train_step(params, grads, feats, targets, .5,
                                                    seed, 1.).cpu()
    want_nll = float(terms[0] / terms[1])
    want_reg = float(terms[2]) / (rows * k)
    nll_rel = abs(float(nll) - want_nll) / want_nll
    reg_rel = abs(float(reg) - want_reg) / want_reg
    got = {n: p.grad for n, p in zip(decoders.TRAIN_PARAMS, params_of(dec))}
    want = {n: g.double() for n, g in zip(decoders.TRAIN_PARAMS, grads)}
    worst, where = worst_grad(got, want, lambda n: grad_scale(n, want))
    print(f'{case} vs train_step: nll rel {nll_rel:.1e}, reg rel {reg_rel:.1e}, worst '
          f'grad err / max|grad| {worst:.2e} ({where})')
    assert nll_rel <= 1e-6 and reg_rel <= 1e-6, (nll_rel, reg_rel)
    assert worst <= GRAD_RTOL, (where, worst)


def test_own_loop_reproduces_reference_fit(dev, golden):
    """Decoder.fit's loop (reference :873-1070) written by a user on top of the
    differentiable forward: the same draws from torch's global generator (the
    split, each DataLoader iterator's base seed, the validation passes)."""
    model = golden_decoder().to(dev)
    dataset = corpus_dataset(golden['features'])
    features = torch.utils.data.TensorDataset(golden['features'])
    want = META['fit_split']
    torch.set_rng_state(golden['fit_split_rng'])

    class WrapperDataset(torch.utils.data.Dataset):
        def __init__(self, subset):
            self.samples = [(features[i], ann) for i in subset.indices
                            for ann in ([dataset[i][4]] if isinstance(dataset[i][4], str)
                                        else dataset[i][4])]

        def __getitem__(self, index):
            return self.samples[index]

        def __len__(self):
            return len(self.samples)

    train, val = training.random_split(dataset, hold_out=want['kwargs']['hold_out'])
    train_loader = torch.utils.data.DataLoader(WrapperDataset(train), batch_size=16,
                                               shuffle=True)
    val_loader = torch.utils.data.DataLoader(WrapperDataset(val), batch_size=16)
    optimizer = torch.optim.AdamW(model.parameters())
    pad = model.indexer.pad_index

    def batch_inputs(batch):
        (inputs,), captions = batch
        targets = torch.tensor(model.indexer(captions), device=dev)[:, 1:]
        return inputs.to(dev), targets

    seen = []
    for _ in range(want['kwargs']['max_epochs']):
        model.train()
        model.encoder.eval()
        for batch in train_loader:
            inputs, targets = batch_inputs(batch)
            out = model(inputs, length=targets.shape[1], strategy=targets, mi=False)
            nll, _, loss = process_loss(out, targets, pad)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            seen.append(float(nll))
        model.eval()
        for batch in val_loader:
            inputs, targets = batch_inputs(batch)
            with torch.no_grad():
                model(inputs, length=targets.shape[1], strategy=targets, mi=False)
        model.bleu(val, strategy=decoders.STRATEGY_GREEDY, mi=False, device=dev,
                   display_progress_as=None)
    g = torch.tensor(seen, dtype=torch.float64)
    w = torch.tensor(want['batch_train_nll'], dtype=torch.float64)
    assert len(g) == len(w)
    rel = float(((g - w).abs() / w.abs()).max())
    sd = model.state_dict()
    gaps = {name: float((sd[name].cpu() - golden['fit_split_final'][name]).abs().max())
            for name in decoders.TRAIN_PARAMS if name not in NOISE_ONLY}
    where = max(gaps, key=gaps.get)
    print(f'own loop: max relative train NLL gap {rel:.2e}, max |param - reference| '
          f'{gaps[where]:.2e} ({where})')
    assert rel <= 1e-4, rel
    assert gaps[where] <= 1e-5, gaps


class ScaledEncoder(encoders.Encoder):
    """(N, 1, 1, F) "images" -> images * scale, one learnable (F,) tensor."""

    def __init__(self, feature_size):
        super().__init__()
        self.feature_shape = (feature_size,)
        self.scale = nn.Parameter(torch.linspace(.5, 1.5, feature_size))

    def forward(self, images, masks=None, **_):
        return images.reshape(len(images), -1) * self.scale

    def properties(self):
        return {'feature_size': self.feature_shape[0]}


def test_foreign_encoder_receives_feature_gradient(dev):
    v, fs, hsz, emb, rows, k, length = 60, 64, 32, 16, 9, 15, 7
    dec = make_decoder(v - 4, fs, hsz, emb, seed=8)
    dec.encoder = ScaledEncoder(fs)
    dec = dec.to(dev)
    dec.dropout = .5
    dec.train()
    feats, targets = random_batch(v, rows, k, fs, length, seed=9)
    images = feats.view(rows, k, 1, 1, fs).to(dev)
    g = torch.Generator().manual_seed(10)
    glp = torch.randn(rows, length, v, generator=g).to(dev)
    gatt = torch.randn(rows, length, k, generator=g).to(dev)
    seed = peek_seed(dev)
    out = dec(images, encode=True, length=length, strategy=targets.to(dev), mi=False)
    ((out.predictions * glp).sum() + (out.attentions * gatt).sum()).backward()
    got = dec.encoder.scale.grad

    w = {n: t.detach().double() for n, t in zip(decoders.TRAIN_PARAMS, params_of(dec))}
    scale = dec.encoder.scale.detach().double().requires_grad_()
    mask = lms.decoder_dropout_mask(seed, rows, length, hsz, .5).to(dev)
    lp, att = trainref.decoder_forward(w, feats.to(dev).double() * scale, targets.to(dev), v - 4,
                            mask, .5)
    ((lp * glp.double()).sum() + (att * gatt.double()).sum()).backward()
    rel = float((got.double() - scale.grad).abs().max() / scale.grad.abs().max())
    print(f'foreign encoder: d scale err / max|grad| {rel:.2e}')
    assert rel <= 1e-5, rel


def run_graph(dec, feats, targets, glp, gatt, dev, state, between=None):
    """Forward and backward from a fixed generator state: (outputs, grads)."""
    torch.cuda.default_generators[dev.index].set_state(state)
    for p in dec.parameters():
        p.grad = None
    x = feats.clone().requires_grad_()
    out = dec(x, length=targets.shape[1], strategy=targets, mi=False)
    if between is not None:
        between()
    ((out.predictions * glp).sum() + (out.attentions * gatt).sum()).backward()
    torch.cuda.synchronize()
    return ([out.predictions.detach().clone(), out.attentions.detach().clone()],
            [p.grad.clone() for p in params_of(dec)] + [x.grad.clone()])


def test_deterministic_private_workspace_and_one_backward(dev):
    v, fs, hsz, emb, rows, k, length = 5004, 3904, 512, 128, 64, 15, 16
    dec = make_decoder(v - 4, fs, hsz, emb, seed=4).to(dev)
    dec.dropout = .5
    dec.train()
    feats, targets = random_batch(v, rows, k, fs, length, seed=11)
    feats, targets = feats.to(dev), targets.to(dev)
    g = torch.Generator().manual_seed(12)
    glp = torch.randn(rows, length, v, generator=g).to(dev)
    gatt = torch.randn(rows, length, k, generator=g).to(dev)
    state = torch.cuda.default_generators[dev.index].get_state()
    out1, g1 = run_graph(dec, feats, targets, glp, gatt, dev, state)
    out2, g2 = run_graph(dec, feats, targets, glp, gatt, dev, state)
    for a, b in zip(out1 + g1, out2 + g2):
        assert torch.equal(a, b)

    # an unrelated fit-style step on the decoder's own training context between
    # the forward and the backward leaves the saved activations alone
    other_f, other_t = random_batch(v, rows, k, fs, length, seed=13)
    params = [p.detach() for p in params_of(dec)]
    scratch = [torch.empty_like(p) for p in params]

    def step():
        dec._train_context().decoder_train_step(params, scratch, other_f.to(dev),
                                                other_t.to(dev), .5, 5, 1.)
    out3, g3 = run_graph(dec, feats, targets, glp, gatt, dev, state, between=step)
    for a, b in zip(out1 + g1, out3 + g3):
        assert torch.equal(a, b)

    out = dec(feats, length=length, strategy=targets, mi=False)
    loss = (out.predictions * glp).sum() + (out.attentions * gatt).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='already backpropagated'):
        loss.backward()


def test_training_mode_rules_unchanged(dev):
    v, fs, hsz, emb, rows, k, length = 60, 64, 32, 16, 4, 15, 7
    dec = make_decoder(v - 4, fs, hsz, emb, seed=14).to(dev)
    dec.dropout = .5
    dec.precision = 'f32'
    feats, targets = random_batch(v, rows, k, fs, length, seed=15)
    feats, targets = feats.to(dev), targets.to(dev)
    dec.eval()
    evaluated = dec(feats, length=length, strategy=targets, mi=False)
    dec.train()
    for strategy in ('greedy', 'sample', 'beam'):
        with pytest.raises(NotImplementedError):
            dec(feats, length=length, strategy=strategy, mi=False)
    with torch.no_grad():  # still the training forward (dropout), nothing retained
        out = dec(feats, length=length, strategy=targets, mi=False)
    assert out.predictions.grad_fn is None and not out.predictions.requires_grad
    assert not torch.equal(out.predictions, evaluated.predictions)
    dec.dropout = 0.
    with torch.no_grad():
        out = dec(feats, length=length, strategy=targets, mi=False)
    # dropout 0: the training forward's outputs are the eval forward's (other kernels)
    assert float((out.predictions - evaluated.predictions).abs().max()) <= 1e-4
    assert float((out.scores - evaluated.scores).abs().max()) <= 1e-3


EVAL_SCRIPT = r'''
import sys
import torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests', sys.argv[1] + '/neuron-descriptions_amd']
from test_gpu_decoder_train import make_decoder, random_batch
v, fs, hsz, emb, rows, k, length = 60, 64, 32, 16, 5, 15, 7
dec = make_decoder(v - 4, fs, hsz, emb, seed=16).to('cuda')
feats, targets = random_batch(v, rows, k, fs, length, seed=17)
feats, targets = feats.cuda(), targets.cuda()

def forced():
    dec.eval()
    with torch.no_grad():
        out = dec(feats, length=length, strategy=targets, mi=False)
    return [out.scores, out.predictions, out.attentions]

before = forced()  # no training-mode call in this process yet
dec.train()
dec.dropout = .5
out = dec(feats, length=length, strategy=targets, mi=False)
(out.predictions.sum() + out.attentions.sum()).backward()
after = forced()
assert all(torch.equal(a, b) for a, b in zip(before, after))
print('eval forced bits unchanged')
'''


def test_eval_forced_bits_unchanged_by_training_calls(dev):
    run = subprocess.run([sys.executable, '-c', EVAL_SCRIPT, str(REPO)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'eval forced bits unchanged' in run.stdout
