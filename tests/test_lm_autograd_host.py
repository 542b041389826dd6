"""Host-side pieces of the differentiable training-mode `LanguageModel.forward` (no
GPU): the C ABI of milan_lm_forward_train / milan_lm_backward as the binding declares
it, the rule that selects the new path, and the float64 pin of tests/lmref.py against
nn.Embedding / nn.LSTM / nn.Linear."""
import fnmatch
import re

import pytest
import torch
from torch import nn

import lmref
import trainref
from conftest import REPO
from milan_amd import hip, lang, lms, synthetic

NEW_CALLS = ('milan_lm_grad_workspace_bytes', 'milan_lm_forward_train',
             'milan_lm_backward')


def make_lm(layers=2, dropout=.5):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(20)), str.split, True, True,
                       True, True)
    return lms.LanguageModel(idx, 8, 16, layers=layers, dropout=dropout)


def test_abi_11_declares_the_lm_autograd_pair():
    assert hip.ABI_VERSION == 11
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    for name in NEW_CALLS:
        proto = re.search(r'\b' + name + r'\(([^;]*)\);', header)
        assert proto, name
        n_args = len(proto.group(1).split(','))
        assert len(hip.SIGNATURES[name][1]) == n_args, name
    # the same leading parameter list as milan_lm_train_step: ctx, params, [grads,]
    # n_params, inputs
    fwd, bwd = (hip.SIGNATURES[n][1] for n in NEW_CALLS[1:])
    step = hip.SIGNATURES['milan_lm_train_step'][1]
    assert bwd[:5] == step[:5] and fwd[:4] == [step[0], step[1]] + step[3:5]
    # ... and its dropout, seed and trailing workspace, size, stream
    assert bwd[7:9] == step[8:10] == fwd[6:8]
    assert bwd[-3:] == step[-3:] == fwd[-3:]
    assert hip.SIGNATURES[NEW_CALLS[0]] == hip.SIGNATURES['milan_lm_train_workspace_bytes']


def test_new_symbols_are_exported():
    text = (REPO / 'neuron-descriptions_amd' / 'csrc' / 'exports.map').read_text()
    patterns = re.search(r'global:([^}]*?)local:', text, re.S).group(1)
    patterns = [p.strip() for p in patterns.replace('\n', ' ').split(';') if p.strip()]
    source = (REPO / 'neuron-descriptions_amd' / 'csrc' / 'lm_train.hip').read_text()
    for name in NEW_CALLS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
        assert re.search(r'\b' + name + r'\(', source.split('extern "C" {')[1]), name


def test_parameters_do_not_require_grad_by_default():
    model = make_lm()
    assert model.training  # a fresh nn.Module
    assert len(list(model.parameters())) == 4 * model.layers + 3
    assert not any(p.requires_grad for p in model.parameters())


def test_trainable_training_mode_reaches_the_hip_path():
    model = make_lm()
    inputs = torch.randint(0, 20, (3, 5))
    model.requires_grad_(True)
    model.train()
    # the differentiable path is taken, and a CPU model has no CPU fallback
    for reduce in (False, True):
        with pytest.raises(hip.HipUnavailableError):
            model(inputs, reduce=reduce)
    # one trainable tensor is enough
    model.requires_grad_(False)
    dict(model.named_parameters())['output.0.bias'].requires_grad_(True)
    with pytest.raises(hip.HipUnavailableError):
        model(inputs)


def test_masks_are_a_constant():
    model = make_lm()
    model.requires_grad_(True)
    model.train()
    inputs = torch.randint(0, 20, (3, 5))
    masks = torch.rand(3, 4, requires_grad=True)
    with pytest.raises(ValueError, match='masks'):
        model(inputs, reduce=True, masks=masks)


def test_missing_symbols_give_a_clear_error():
    class OldLibrary:
        pass

    ctx = object.__new__(hip.Context)
    ctx.lib = OldLibrary()
    with pytest.raises(hip.HipUnavailableError, match='milan_lm_'):
        ctx.lm_forward_train([], torch.zeros(1, 1, dtype=torch.long))


# ---- tests/lmref.py at float64 against the reference's modules ---------------------
def module_logprobs(sd, v, e, h, layers, pad, inputs, masks, p):
    """nn.Embedding (padding_idx), nn.LSTM (one multi-layer module without dropout,
    else one per layer with the explicit masks between), nn.Linear + log_softmax in
    float64: (log-probs, {state-dict name: parameter})."""
    sd = {k: t.double() for k, t in sd.items()}
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
    named = {'embedding.weight': emb.weight, 'output.0.weight': out.weight,
             'output.0.bias': out.bias}
    for l in range(layers):
        m, sub = (lstms[0], l) if masks is None else (lstms[l], 0)
        for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            named[f'lstm.{n}_l{l}'] = getattr(m, f'{n}_l{sub}')
    return torch.log_softmax(out(x), -1), named


@pytest.mark.parametrize('layers,p', [(1, 0.), (2, 0.), (3, .5), (2, .9)])
@pytest.mark.parametrize('reduce', [False, True])
def test_lmref_matches_torch_modules_float64(layers, p, reduce):
    from test_gpu_lm_train import random_batch, random_state
    v, e, h, rows, length = 24, 12, 20, 6, 9
    pad, stop = v - 2, v - 3
    sd = random_state(v, e, h, layers, seed=5 + layers)
    inputs, _ = random_batch(v, rows, length, seed=layers)
    inputs[0, 3] = stop  # a stop in mid-sequence: the default mask cuts after it
    masks = [lms.dropout_mask(77, l, rows, length, h, p) for l in range(layers - 1)] \
        if p else None
    g = torch.Generator().manual_seed(9)
    up = torch.randn(rows, length, v, generator=g, dtype=torch.float64)
    ups = torch.randn(rows, generator=g, dtype=torch.float64)
    token_masks = lmref.default_masks(inputs, stop)
    assert token_masks[0].tolist() == [1, 1, 1, 1] + [0] * (length - 5)

    def objective(lp):
        if not reduce:
            return lp, (lp * up).sum()
        s = lmref.scores(lp, inputs, token_masks)
        return s, (s * ups).sum()

    got, grads = lmref.run(sd, inputs, pad, layers, objective, masks, p)
    lp, named = module_logprobs(sd, v, e, h, layers, pad, inputs, masks, p)
    want, loss = objective(lp)
    loss.backward()
    assert float((got - want.detach()).abs().max()) <= 1e-12
    assert set(grads) == set(named)
    for name, param in named.items():
        g64 = param.grad if param.grad is not None else torch.zeros_like(param)
        err = float((grads[name] - g64).abs().max())
        assert err <= 1e-12 * float(g64.abs().max()) + 1e-15, (name, err)
    assert not grads['embedding.weight'][pad].any()


def test_float32_reference_is_float32():
    from test_gpu_lm_train import random_batch, random_state
    sd = random_state(24, 12, 20, 2, seed=1)
    inputs, _ = random_batch(24, 4, 6, seed=2)
    with trainref.fp32_reference():
        out, grads = lmref.run(sd, inputs, 22, 2, lambda lp: (lp, lp.sum()),
                               dtype=torch.float32)
    assert out.dtype == torch.float32
    assert all(g.dtype == torch.float32 for g in grads.values())
