"""Decoder training on the GPU (csrc/decoder_train.hip, milan_decoder_train_step).

  * Loss terms and the gradients of the decoder's 19 tensors against float64
    autograd of a torch restatement of the teacher-forced attention LSTM (with
    dropout the host regenerates the kernel's mask), at the goldens' dims and
    at the benchmark's; with and without the regulariser; with pad inputs and
    all-pad rows (the embedding's pad row gets a real gradient).
  * One batch against the reference's own autograd (make_golden_decoder_fit.py).
  * Determinism and overwrite semantics.
  * `Decoder.fit` against the reference's training runs: per-batch losses,
    final parameters, the stop epoch; BLEU-driven early stopping; features
    from the native encoder; inference and save / load after fit.
"""
import io
import json

import pytest
import torch

import trainref
from conftest import GOLDEN_DIR
from milan_amd import decoders, encoders, hip, lang, lms, synthetic

pytestmark = pytest.mark.gpu

META = json.loads((GOLDEN_DIR / 'reference_goldens_decoder_fit.json').read_text())


@pytest.fixture(scope='module')
def dev():
    hip.load_library()
    return hip.require_device('cuda')


def golden_features():
    """The goldens' features, drawn again from their seeded CPU generator (they
    are not stored) and checked against the recorded fingerprint."""
    meta = META['features']
    g = torch.Generator().manual_seed(meta['seed'])
    features = torch.randn(*meta['shape'], generator=g)
    flat = features.reshape(-1)
    assert flat[:len(meta['head'])].tolist() == meta['head']
    assert float(flat.double().sum()) == pytest.approx(meta['sum'], rel=1e-12)
    assert float((flat.double()**2).sum()) == pytest.approx(meta['sum_squares'],
                                                           rel=1e-12)
    return features


@pytest.fixture(scope='module')
def golden():
    out = torch.load(GOLDEN_DIR / 'reference_goldens_decoder_fit.pt')
    out['features'] = golden_features()
    return out


def tokenize(texts):
    if isinstance(texts, str):
        return tuple(texts.lower().split())
    return tuple(tuple(t.lower().split()) for t in texts)


class IdentityEncoder(encoders.Encoder):
    """(N, 1, 1, F) "images" -> (N, F) features (the goldens' stand-in)."""

    def __init__(self, feature_size):
        super().__init__()
        self.feature_shape = (feature_size,)

    def forward(self, images, masks=None, **_):
        return images.reshape(len(images), -1)

    def properties(self):
        return {'feature_size': self.feature_shape[0]}


def make_decoder(nvocab, fs, hidden, emb, seed, attention_hidden_size=None):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(nvocab)), tokenize, True,
                       True, True, True)
    dec = decoders.Decoder(idx, IdentityEncoder(fs), embedding_size=emb,
                           hidden_size=hidden, attention_hidden_size=attention_hidden_size,
                           dropout=0.)
    torch.manual_seed(seed)
    dec.reset_parameters()
    return dec


def random_batch(v, rows, k, fs, length, seed, all_pad_rows=()):
    """Features in [0, 1) and targets: tokens, <stop>, then <pad> (ids of
    a vocabulary with v - 4 tokens + start, stop, pad, unk)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.rand(rows, k, fs, generator=g)
    stop, pad = v - 3, v - 2
    targets = torch.full((rows, length), pad, dtype=torch.long)
    for r in range(rows):
        n = int(torch.randint(1, length, (), generator=g))
        targets[r, :n - 1] = torch.randint(0, v - 4, (n - 1,), generator=g)
        targets[r, n - 1] = stop
    for r in all_pad_rows:
        targets[r] = pad
    return feats, targets


def train_ctx(dec, dev):
    sd = {k: v for k, v in dec.state_dict().items() if not k.startswith('encoder.')}
    return hip.Context(hip.make_dims(sd, len(dec.indexer.vocab)), {}, dev,
                       finalize=False)


def run_step(ctx, params, feats, targets, dev, p=0., seed=0, reg=1., grads=None):
    params = [t.to(dev).contiguous() for t in params]
    if grads is None:
        grads = [torch.full_like(t, float('nan')) for t in params]
    loss = ctx.decoder_train_step(params, grads, feats, targets, p, seed, reg)
    torch.cuda.synchronize()
    return loss.cpu(), [g.cpu() for g in grads]


# Target bounds: every gradient within 1e-5 x max|grad| of its tensor, the NLL and
# regulariser sums within 1e-6 relative (DESIGN.md 4.12 gives the measured values).
GRAD_RTOL, LOSS_RTOL = 1e-5, 1e-6


def grad_scale(name, want_grads):
    """max|grad| of a tensor.  The attention score bias shifts the k scores of a
    row equally and the softmax cancels it: its exact gradient is 0, and both
    sides hold the rounding of a sum of d-scores that cancels.  It is measured
    against the scale of those terms, the gradient of the score weight."""
    if name == 'attend.output.0.bias':
        name = 'attend.output.0.weight'
    return float(want_grads[name].abs().max())


def check(loss, grads, want_sum, want_count, want_reg, want_grads, tag):
    assert int(loss[1]) == want_count
    nll_rel = abs(float(loss[0]) - want_sum) / max(abs(want_sum), 1e-30)
    reg_rel = abs(float(loss[2]) - want_reg) / max(abs(want_reg), 1e-30)
    worst, where = 0., None
    for name, got in zip(decoders.TRAIN_PARAMS, grads):
        want = want_grads[name].cpu()
        scale = grad_scale(name, want_grads)
        err = float((got.double() - want).abs().max())
        if err / max(scale, 1e-30) > worst:
            worst, where = err / max(scale, 1e-30), name
    print(f'{tag}: nll rel {nll_rel:.1e}, reg rel {reg_rel:.1e}, worst grad err / '
          f'max|grad| {worst:.2e} ({where})')
    assert nll_rel <= LOSS_RTOL and reg_rel <= LOSS_RTOL, (nll_rel, reg_rel)
    assert worst <= GRAD_RTOL, (where, worst)


CASES = {
    # name: (vocab, F, H, E, rows, k, L)
    'golden_dims': (60, 64, 32, 16, 9, 15, 7),
    'bench_dims': (5004, 3904, 512, 128, 64, 15, 16),
}


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('p,reg', [(0., 0.), (0., 1.), (.5, 1.)])
def test_gradients_match_autograd_float64(dev, case, p, reg):
    v, fs, hsz, emb, rows, k, length = CASES[case]
    dec = make_decoder(v - 4, fs, hsz, emb, seed=v + fs)
    named = dict(dec.named_parameters())
    params = [named[n].detach() for n in decoders.TRAIN_PARAMS]
    feats, targets = random_batch(v, rows, k, fs, length, seed=rows + length)
    ctx = train_ctx(dec, dev)
    seed = 0x0123_4567_89ab_cdef
    loss, grads = run_step(ctx, params, feats, targets, dev, p, seed, reg)
    mask = lms.decoder_dropout_mask(seed, rows, length, hsz, p) if p else None
    want = trainref.decoder_loss(dict(zip(decoders.TRAIN_PARAMS, params)), feats, targets,
                                 v - 4, v - 2, mask, p, reg, device=dev)
    check(loss, grads, *want, tag=f'{case} p={p} reg={reg}')
    if not p:  # eval-mode terms are the same forward
        nll = ctx.decoder_nll([t.to(dev) for t in params], feats, targets).cpu()
        assert torch.equal(nll, loss)
    ctx.close()


def test_pad_inputs_and_all_pad_rows(dev):
    v, fs, hsz, emb, rows, k, length = 60, 64, 32, 16, 8, 15, 9
    dec = make_decoder(v - 4, fs, hsz, emb, seed=3)
    named = dict(dec.named_parameters())
    params = [named[n].detach() for n in decoders.TRAIN_PARAMS]
    feats, targets = random_batch(v, rows, k, fs, length, seed=5,
                                  all_pad_rows=(2, 5))
    assert (targets[:, :-1] == v - 2).any()  # pad is an input somewhere
    ctx = train_ctx(dec, dev)
    loss, grads = run_step(ctx, params, feats, targets, dev)
    want = trainref.decoder_loss(dict(zip(decoders.TRAIN_PARAMS, params)), feats, targets,
                                 v - 4, v - 2, device=dev)
    check(loss, grads, *want, tag='pad rows')
    emb_grad = grads[decoders.TRAIN_PARAMS.index('embedding.weight')]
    assert emb_grad[v - 2].abs().max() > 0  # no padding_idx: the pad row learns
    ctx.close()


def test_reference_batch_gradients(dev, golden):
    dims = META['dims']
    torch.manual_seed(7)
    dec = decoders.decoder(corpus_dataset(), IdentityEncoder(dims['F']),
                           indexer_kwargs=dict(tokenize=tokenize),
                           embedding_size=dims['embedding_size'],
                           hidden_size=dims['hidden_size'], dropout=0.)
    named = dict(dec.named_parameters())
    params = [named[n].detach() for n in decoders.TRAIN_PARAMS]
    feats = golden['features'][golden['batch_rows']]
    targets = golden['batch_targets']
    assert torch.equal(targets, torch.tensor(dec.indexer(META['batch_captions']))[:, 1:])
    ctx = train_ctx(dec, dev)
    loss, grads = run_step(ctx, params, feats, targets, dev)
    rows, k = feats.shape[:2]
    nll = float(loss[0] / loss[1])
    reg = float(loss[2]) / (rows * k)
    assert nll == pytest.approx(float(golden['batch_nll']), rel=1e-5)
    assert reg == pytest.approx(float(golden['batch_reg']), rel=1e-5)
    for name, got in zip(decoders.TRAIN_PARAMS, grads):
        want = golden['batch_grads'][name]
        scale = grad_scale(name, golden['batch_grads'])
        assert float((got - want).abs().max()) <= 1e-4 * scale + 1e-9, name
    ctx.close()


def test_deterministic_and_overwritten(dev):
    v, fs, hsz, emb, rows, k, length = 5004, 3904, 512, 128, 64, 15, 16
    dec = make_decoder(v - 4, fs, hsz, emb, seed=2)
    named = dict(dec.named_parameters())
    params = [named[n].detach().to(dev) for n in decoders.TRAIN_PARAMS]
    feats, targets = random_batch(v, rows, k, fs, length, seed=4)
    ctx = train_ctx(dec, dev)
    grads = [torch.full_like(t, 7.) for t in params]  # garbage: overwritten
    loss1, g1 = run_step(ctx, params, feats, targets, dev, .5, 99, grads=grads)
    loss2, g2 = run_step(ctx, params, feats, targets, dev, .5, 99)
    assert torch.equal(loss1, loss2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    loss3, g3 = run_step(ctx, params, feats, targets, dev, .5, 100)
    assert not torch.equal(loss1, loss3)
    assert not torch.equal(g1[-2], g3[-2])
    ctx.close()


# ---- fit against the reference's runs -----------------------------------------------
def corpus_dataset(features=None):
    k, fs = META['dims']['k'], META['dims']['F']
    out = []
    for i, ann in enumerate(META['corpus']):
        images = None if features is None else features[i].view(k, 1, 1, fs)
        out.append(('layer', i, images, torch.ones(k, 1, 1, 1), ann))
    return out


def golden_decoder():
    dims = META['dims']
    torch.manual_seed(7)
    return decoders.decoder(corpus_dataset(), IdentityEncoder(dims['F']),
                            indexer_kwargs=dict(tokenize=tokenize),
                            embedding_size=dims['embedding_size'],
                            hidden_size=dims['hidden_size'], dropout=0.)


def spy_steps(monkeypatch):
    seen = {'train': [], 'reg': [], 'val': []}
    step, nll = hip.Context.decoder_train_step, hip.Context.decoder_nll

    def train(self, params, grads, feats, *a, **k):
        terms = step(self, params, grads, feats, *a, **k)
        seen['train'].append(float(terms[0] / terms[1]))
        seen['reg'].append(float(terms[2]) / (feats.shape[0] * feats.shape[1]))
        return terms

    def val(self, *a, **k):
        terms = nll(self, *a, **k)
        seen['val'].append(float(terms[0] / terms[1]))
        return terms

    monkeypatch.setattr(hip.Context, 'decoder_train_step', train)
    monkeypatch.setattr(hip.Context, 'decoder_nll', val)
    return seen


# max |parameter - reference| after the run: 1e-5 at lr 1e-3; the lr 0.05 run's
# normalised Adam steps amplify fp32 reordering (as for the LM).  The attention
# score bias is left out: its gradient is rounding noise around an exact 0 on
# both sides (see grad_scale), which Adam normalises into full-size steps of
# either sign, and it changes no output (the softmax cancels it).
PARAM_ATOL = {'fit_split': 1e-5, 'fit_fixed': 1e-5, 'fit_stop': 1e-3}
NOISE_ONLY = ('attend.output.0.bias',)


@pytest.mark.parametrize('case', ['fit_split', 'fit_fixed', 'fit_stop'])
def test_fit_reproduces_reference_run(dev, golden, monkeypatch, case):
    model = golden_decoder()
    for name in decoders.TRAIN_PARAMS:
        assert torch.equal(model.state_dict()[name], golden['init'][name])
    model.to(dev)
    seen = spy_steps(monkeypatch)
    features = torch.utils.data.TensorDataset(golden['features'])
    torch.set_rng_state(golden[f'{case}_rng'])
    model.fit(corpus_dataset(golden['features']), batch_size=16, stop_on_bleu=False,
              features=features, display_progress_as=None, **META[case]['kwargs'])
    assert not model.training
    want = META[case]
    assert len(seen['train']) == want['epochs'] * want['train_batches']
    assert len(seen['val']) == want['epochs'] * want['val_batches']
    for kind, ref in (('train', 'batch_train_nll'), ('reg', 'batch_train_reg'),
                      ('val', 'batch_val_loss')):
        g = torch.tensor(seen[kind], dtype=torch.float64)
        w = torch.tensor(want[ref], dtype=torch.float64)
        rel = float(((g - w).abs() / w.abs()).max())
        print(f'{case} {kind}: max relative loss gap {rel:.2e}')
        assert rel <= 1e-4, (kind, rel)
    sd = model.state_dict()
    gaps = {name: float((sd[name].cpu() - golden[f'{case}_final'][name]).abs().max())
            for name in decoders.TRAIN_PARAMS if name not in NOISE_ONLY}
    where = max(gaps, key=gaps.get)
    print(f'{case}: max |param - reference| {gaps[where]:.2e} ({where}) after '
          f'{want["epochs"]} epochs')
    assert gaps[where] <= PARAM_ATOL[case], gaps


def test_fit_stops_on_bleu(dev, golden, monkeypatch):
    model = golden_decoder().to(dev)
    scores = iter([1., 3., 2., 2.5, 9., 9.])
    epochs, states = [], []

    def bleu(self, dataset, **kwargs):
        assert kwargs['strategy'] == 'greedy' and kwargs['mi'] is False
        assert not self.training
        epochs.append(len(epochs))
        states.append({k: t.detach().clone() for k, t in self.state_dict().items()})
        return type('Score', (), {'score': next(scores)})()

    monkeypatch.setattr(decoders.Decoder, 'bleu', bleu)
    torch.manual_seed(0)
    model.fit(corpus_dataset(golden['features']), batch_size=32, max_epochs=6,
              patience=1, features=torch.utils.data.TensorDataset(golden['features']),
              display_progress_as=None)
    # EarlyStopping(decreasing=False, patience=1): best 3 at epoch 1, then 2 and 2.5
    # are two bad epochs > patience: stop after epoch 3
    assert epochs == [0, 1, 2, 3]
    # the "best" state aliases the live parameters: the last epoch's values remain
    for name, t in model.state_dict().items():
        assert torch.equal(t, states[-1][name]), name


# ---- native encoder, inference and serialisation after fit --------------------------
NV = 30


def exemplar_dataset(n=12, k=3, size=64):
    images, masks = synthetic.exemplars(n, k=k, size=size, seed=3)
    tokens = synthetic.vocab_tokens(NV)
    g = torch.Generator().manual_seed(4)
    out = []
    for i in range(n):
        caps = []
        for _ in range(2):
            ids = torch.randint(0, NV, (int(torch.randint(2, 6, (), generator=g)),),
                                generator=g)
            caps.append(' '.join(tokens[j] for j in ids.tolist()))
        out.append(('layer', i, images[i], masks[i], caps))
    return out


def native_decoder(dev):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(NV)), tokenize, True, True,
                       True, True)
    enc = encoders.PyramidConvEncoder('resnet50', width=16, pretrained=False)
    lm = lms.LanguageModel(idx, 16, 32, layers=1, dropout=0.)
    dec = decoders.Decoder(idx, enc, lm, embedding_size=16, hidden_size=32, length=6,
                           beam_size=3, dropout=0.)
    sd = synthetic.milan_state_dict(NV + 4, 'resnet50', seed=11, width=16,
                                    hidden_size=32, embedding_size=16,
                                    lm_hidden_size=32, lm_embedding_size=16,
                                    lm_layers=1)
    dec.load_state_dict(sd, strict=True)
    dec.precision = 'f32'
    return dec.to(dev)


def test_fit_native_encoder_features_and_inference_after(dev):
    dataset = exemplar_dataset()
    a, b = native_decoder(dev), native_decoder(dev)
    frozen = {k: t.detach().clone() for k, t in a.state_dict().items()
              if k.startswith(('encoder.', 'lm.'))}
    features = b.encoder.map(dataset, mask=True, image_index=2, mask_index=3,
                             device=dev, display_progress_as=False)
    before = a(dataset[0][2][None].to(dev), dataset[0][3][None].to(dev),
               strategy='greedy', mi=False)
    kwargs = dict(batch_size=8, max_epochs=2, stop_on_bleu=False,
                  optimizer_kwargs=dict(lr=1e-2), display_progress_as=None)
    torch.manual_seed(1)
    a.fit(dataset, **kwargs)
    torch.manual_seed(1)
    b.fit(dataset, features=features, **kwargs)
    sa, sb = a.state_dict(), b.state_dict()
    for name in decoders.TRAIN_PARAMS:
        assert float((sa[name] - sb[name]).abs().max()) <= 1e-5, name
    for name, t in frozen.items():  # encoder and LM untouched, never given a grad
        assert torch.equal(sa[name], t), name
    for name, p in a.named_parameters():
        if name.startswith(('encoder.', 'lm.')):
            assert p.grad is None, name

    # inference uses the fitted weights: the packed context is rebuilt
    images, masks = dataset[0][2][None].to(dev), dataset[0][3][None].to(dev)
    after = a(images, masks, strategy='greedy', mi=False)
    assert not torch.equal(after.predictions, before.predictions)
    fresh = native_decoder(dev)
    fresh.load_state_dict(a.state_dict())
    want = fresh(images, masks, strategy='greedy', mi=False)
    assert torch.equal(after.predictions, want.predictions)
    assert after.captions == want.captions
    assert a.predict(dataset[:4], display_progress_as=None) == \
        fresh.predict(dataset[:4], display_progress_as=None)

    buffer = io.BytesIO()
    a.save(buffer)
    buffer.seek(0)
    loaded = decoders.Decoder.load(buffer).to(dev)
    loaded.precision = 'f32'
    for name, t in a.state_dict().items():
        assert torch.equal(loaded.state_dict()[name].to(t.device), t), name
    assert torch.equal(loaded(images, masks, strategy='greedy', mi=False).predictions,
                       after.predictions)
