"""Torch restatements of the training paths, the reference every training test
compares the HIP kernels with (like featclass.py and beamcheck.py, a helper
module, not a test file).

  * `lm_loss`: LanguageModel.fit's loss (csrc/lm_train.hip).
  * `decoder_forward` / `decoder_loss`: the teacher-forced attention LSTM and
    Decoder.fit's loss (csrc/decoder_train.hip).

Each takes `dtype` and `device`, so the same code gives the float64 truth and a
float32 torch result of the same maths (`fp32_reference` turns off every
reduced-precision matmul mode for the latter).  tests/test_train_ref_host.py
pins them to the reference's own autograd on the CPU.

Also here: the split planner of the shared GEMM and the column-sum chunking,
restated from tgemm.hip, and the (M, N, K) of every GEMM each training call
runs, so that the tests can say which branches a shape reaches.
"""
import contextlib

import torch
import torch.nn.functional as F


def _leaves(w, dtype, device):
    return {k: t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
            for k, t in w.items()}


def lm_loss(sd, inputs, targets, pad, layers, masks=None, p=0.,
            dtype=torch.float64, device='cpu'):
    """Autograd of Embedding(padding_idx) -> LSTM (dropout on the output of
    every layer but the last, explicit masks) -> Linear -> log_softmax -> sum
    of NLL over non-pad targets, in `dtype` on `device`.  `masks[l]`: the
    kept units of layer l's output, (rows, L, H) bool.  Returns (sum, count,
    grads of sum / count)."""
    w = _leaves(sd, dtype, device)
    inputs, targets = inputs.to(device), targets.to(device)
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
            x = x * masks[l].to(device=device, dtype=dtype) / (1 - p)
    logits = x @ w['output.0.weight'].t() + w['output.0.bias']
    lp = F.log_softmax(logits, -1)
    total = F.nll_loss(lp.reshape(-1, lp.shape[-1]), targets.reshape(-1),
                       ignore_index=pad, reduction='sum')
    count = int((targets != pad).sum())
    (total / count).backward()
    return float(total.detach()), count, {k: t.grad for k, t in w.items()}


def decoder_forward(w, feats, targets, start, mask=None, p=0.):
    """The reference's teacher-forced forward (decoders.py:431-463 over step
    :576-634) in the dtype and on the device of `w` and `feats`: (log-probs
    (rows, L, V), attentions (rows, L, k)).  The attention hidden size A is
    that of `attend.query_to_hidden.weight` (A, H), independent of H.
    `mask`: the kernel's dropout mask on h, (rows, L, H)."""
    rows, k, _ = feats.shape
    length = targets.shape[1]
    pooled = feats.mean(dim=1)
    h = torch.tanh(pooled @ w['init_h.0.weight'].t() + w['init_h.0.bias'])
    c = torch.tanh(pooled @ w['init_c.0.weight'].t() + w['init_c.0.bias'])
    keys = feats @ w['attend.key_to_hidden.weight'].t() + w['attend.key_to_hidden.bias']
    inputs = torch.cat([torch.full((rows, 1), start, dtype=torch.long,
                                   device=targets.device), targets[:, :-1]], 1)
    hsz = h.shape[1]
    logps, atts = [], []
    for t in range(length):
        q = h @ w['attend.query_to_hidden.weight'].t() + w['attend.query_to_hidden.bias']
        u = torch.tanh(q[:, None] + keys)
        s = (u @ w['attend.output.0.weight'].t()).squeeze(-1) + w['attend.output.0.bias']
        a = torch.softmax(s, dim=1)
        ctx = (a[..., None] * feats).sum(dim=1)
        gate = torch.sigmoid(h @ w['feature_gate.0.weight'].t() + w['feature_gate.0.bias'])
        x = torch.cat([w['embedding.weight'][inputs[:, t]], ctx * gate], dim=1)
        gates = (x @ w['lstm.weight_ih'].t() + w['lstm.bias_ih'] +
                 h @ w['lstm.weight_hh'].t() + w['lstm.bias_hh'])
        i, f, gg, o = gates.split(hsz, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        hd = h if mask is None else h * mask[:, t].to(h.dtype) / (1 - p)
        logps.append(F.log_softmax(hd @ w['output.1.weight'].t() + w['output.1.bias'], -1))
        atts.append(a)
    return torch.stack(logps, 1), torch.stack(atts, 1)


def decoder_loss(w, feats, targets, start, pad, mask=None, p=0., reg_weight=1.,
                 dtype=torch.float64, device='cpu'):
    """Autograd of the reference's training loss (Decoder.fit :1017-1022) in
    `dtype` on `device`: NLL(ignore pad) mean + reg_weight * mean over (row, k)
    of (1 - sum_t alpha)^2.  Returns (nll sum, count, regulariser sum of
    squares, grads)."""
    w = _leaves(w, dtype, device)
    feats = feats.to(device=device, dtype=dtype)
    targets = targets.to(device)
    if mask is not None:
        mask = mask.to(device)
    rows, k, _ = feats.shape
    lp, att = decoder_forward(w, feats, targets, start, mask, p)
    total = F.nll_loss(lp.reshape(-1, lp.shape[-1]), targets.reshape(-1),
                       ignore_index=pad, reduction='sum')
    count = int((targets != pad).sum())
    regsum = ((1 - att.sum(dim=1))**2).sum()
    (total / count + reg_weight * regsum / (rows * k)).backward()
    return (float(total.detach()), count, float(regsum.detach()),
            {n: t.grad for n, t in w.items()})


@contextlib.contextmanager
def fp32_reference():
    """float32 torch arithmetic without TF32 or other reduced-precision matmul
    modes (the float32 reference that sets the fp32 error class)."""
    saved = (torch.get_float32_matmul_precision(),
             torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.set_float32_matmul_precision('highest')
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(saved[0])
        torch.backends.cuda.matmul.allow_tf32 = saved[1]
        torch.backends.cudnn.allow_tf32 = saved[2]


# ---- the branches a shape reaches ------------------------------------------------
# Restated from neuron-descriptions_amd/csrc/tgemm.hip: plan_splits (:134-145) and
# colsum_chunks (:233-236), with the tile sizes BM = BN = 64, BK = 32 (:25).  The two
# must move together: if the planner changes there, change it here, or the edge
# table of test_gpu_train_fuzz.py no longer provably reaches the branches it names.
BM = BN = 64
BK = 32


def plan_splits(M, N, K):
    """(splits, kchunk) of one GEMM: a function of the shape alone."""
    tiles = -(-M // BM) * -(-N // BN)
    s = 1
    while s < 16 and tiles * s < 512 and K // (2 * s) >= 128:
        s *= 2
    kc = -(-K // s)
    kc = -(-kc // BK) * BK
    if kc == 0:
        kc = BK
    n = -(-K // kc)
    return (n if n > 0 else 1), kc


def colsum_chunks(R):
    c = (R + 63) // 64
    return max(1, min(64, c))


def lm_gemms(E, H, V, layers, rows, L):
    """(name, M, N, K, group) of every GEMM milan_lm_train_step runs; group:
    the rows per sequence of a grouped operand view (0: none)."""
    N = rows * L
    out = [('logits', N, V, H, L), ('dW_out', V, H, N, L), ('dH', N, H, V, 0)]
    for l in range(layers):
        cin = E if l == 0 else H
        out += [(f'x_proj{l}', N, 4 * H, cin, 0), (f'h_step{l}', rows, 4 * H, H, 0),
                (f'dh_prev{l}', rows, H, 4 * H, 0), (f'dW_hh{l}', 4 * H, H, N, L),
                (f'dW_ih{l}', 4 * H, cin, N, 0), (f'dX{l}', N, cin, 4 * H, 0)]
    return out


def lm_colsums(H, V, layers, rows, L):
    """(name, R, columns) of every column sum of milan_lm_train_step."""
    N = rows * L
    return [('db_out', N, V)] + [(f'db{l}', N, 4 * H) for l in range(layers)]


def decoder_gemms(F_, H, E, A, V, rows, k, L):
    """(name, M, N, K, group) of every GEMM of milan_decoder_train_step and
    the feature gradient of milan_decoder_backward."""
    N, BKr = rows * L, rows * k
    return [('init_h', rows, H, F_, 0), ('keys', BKr, A, F_, 0), ('x_emb', N, 4 * H, E, 0),
            ('query', rows, A, H, 0), ('gate', rows, F_, H, 0), ('x_ctx', rows, 4 * H, F_, 0),
            ('h_step', rows, 4 * H, H, 0), ('logits', N, V, H, L), ('dW_out', V, H, N, L),
            ('dY', N, H, V, 0), ('dz', rows, F_, 4 * H, 0), ('dh_q', rows, H, A, 0),
            ('dh_gate', rows, H, F_, 0), ('dh_hh', rows, H, 4 * H, 0),
            ('dW_ih', 4 * H, E + F_, N, 0), ('dW_hh', 4 * H, H, N, L), ('dW_q', A, H, N, L),
            ('dW_gate', F_, H, N, L), ('dW_k', A, F_, BKr, 0), ('dw_o', 1, A, N * k, 0),
            ('dX_emb', N, E, 4 * H, 0), ('dW_init', H, F_, rows, 0), ('dF_keys', BKr, F_, A, 0),
            ('dF_pool', rows, F_, H, 0)]


def decoder_colsums(F_, H, A, V, rows, k, L):
    N = rows * L
    return [('db_out', N, V), ('db', N, 4 * H), ('db_q', N, A), ('db_gate', N, F_),
            ('db_k', rows * k, A), ('db_o', N * k, 1), ('db_init', rows, H)]


def split_branches(gemms):
    """The planner branches a list of GEMMs reaches: 'split' (K split at all),
    'partial_last' (the last split ends before its kchunk does),
    'mid_sequence' (a grouped operand whose split boundary falls inside a
    sequence)."""
    seen = set()
    for _, M, N, K, grp in gemms:
        s, kc = plan_splits(M, N, K)
        if s < 2:
            continue
        seen.add('split')
        if K - (s - 1) * kc < kc:
            seen.add('partial_last')
        if grp and any((z * kc) % grp for z in range(1, s)):
            seen.add('mid_sequence')
    return seen
