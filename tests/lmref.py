"""Torch restatement of the training-mode `LanguageModel.forward`, the reference the
autograd tests compare `lms.TrainingForward` with (a helper module like trainref.py, not
a test file): the forward of `trainref.lm_loss` returning log-probs instead of a loss,
and the reference's `reduce=True` on top of them.

`run` takes `dtype`, so the same code gives the float64 truth and the float32 class
(inside `trainref.fp32_reference()`).  tests/test_lm_autograd_host.py pins it at float64
to nn.Embedding / nn.LSTM / nn.Linear.
"""
import torch
import torch.nn.functional as F

import trainref


def logprobs(w, inputs, pad, layers, masks=None, p=0.):
    """Embedding(padding_idx) -> LSTM (dropout on the output of every layer but the
    last, explicit masks) -> Linear -> log_softmax in the dtype of the leaves `w`:
    (rows, L, V).  `masks[l]`: the kept units of layer l's output, (rows, L, H) bool."""
    x = F.embedding(inputs, w['embedding.weight'], padding_idx=pad)
    rows, length = inputs.shape
    for l in range(layers):
        hsz = w[f'lstm.weight_hh_l{l}'].shape[0] // 4
        pre = x @ w[f'lstm.weight_ih_l{l}'].t() + w[f'lstm.bias_ih_l{l}'] + \
            w[f'lstm.bias_hh_l{l}']
        h = x.new_zeros(rows, hsz)
        c = x.new_zeros(rows, hsz)
        outs = []
        for t in range(length):
            gates = pre[:, t] + h @ w[f'lstm.weight_hh_l{l}'].t()
            i, f, gg, o = gates.split(hsz, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        x = torch.stack(outs, 1)
        if masks is not None and l < layers - 1:
            x = x * masks[l].to(device=x.device, dtype=x.dtype) / (1 - p)
    return F.log_softmax(x @ w['output.0.weight'].t() + w['output.0.bias'], -1)


def default_masks(inputs, stop):
    """The reference's default (lms.py:93-96), loop and all: everything after the
    first stop token is dropped, the term AFTER the stop still counts."""
    masks = inputs.new_ones((inputs.shape[0], inputs.shape[1] - 1))
    for i, j in inputs.eq(stop).nonzero():
        masks[i, j + 1:] = 0
    return masks


def scores(lp, inputs, masks):
    """The reference's `reduce=True` (lms.py:88-100) on log-probs `lp`."""
    picked = lp[:, :-1].gather(2, inputs[:, 1:].unsqueeze(-1)).squeeze(-1)
    return picked.mul(masks.to(lp.dtype)).sum(dim=-1)


def run(sd, inputs, pad, layers, objective, masks=None, p=0., dtype=torch.float64):
    """Autograd of `objective(log-probs) -> (output, scalar)` on the CPU in `dtype`:
    (output detached, {name: gradient}); a parameter the scalar does not reach has a
    zero gradient."""
    w = trainref._leaves(sd, dtype, 'cpu')
    out, loss = objective(logprobs(w, inputs, pad, layers, masks, p))
    loss.backward()
    grads = {k: torch.zeros_like(t) if t.grad is None else t.grad for k, t in w.items()}
    return out.detach(), grads
