"""The per-row top-k of the beam search alone (milan_row_select).

Every shape runs the shipped dispatch (path 0: `row_select_reg_kernel<NR>`, rank counting),
the wide kernels of csrc/beam_wide.hip (path 1: independent code), the threshold path
(path 2) and the first rank-count path (path 3) on the same rows: all four must agree bit
for bit, and path 0 is held to a float64 log_softmax on the CPU.

Shapes: the smallest (V, k) that reaches each branch -- every slot count NR the launch
dispatches on, one thread with two elements, k close to V, waves without elements (the
lower bound T0 is 0 and the threshold path runs).  Rows: see `rows_for`; the quantised and
the constant rows give long equal runs, gathers past the candidate list's 512 entries and
ties that straddle the k-th value.  All logits are finite.
"""
import functools

import pytest
import torch

from milan_amd import hip

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min
TOL = 5e-5
STOP = 3
SHAPES = [(5004, 50), (5004, 2), (5004, 64), (5004, 256), (6144, 50), (257, 50), (1000, 50),
          (300, 200), (150, 100)]
PATHS = ('wide', 'threshold', 'legacy')


def rows_for(V, k, seed):
    """(rows, V) float32 logits and the kind of every row."""
    g = torch.Generator().manual_seed(seed)
    normal = lambda: torch.randn(V, generator=g) * 4
    rows, kinds = [], []
    for _ in range(4):
        rows.append(normal()); kinds.append('normal')
    x = normal()
    x[int(torch.randint(0, V, (1,), generator=g))] += 30
    rows.append(x); kinds.append('raised')
    for _ in range(2):  # 16 levels, all as likely: V / 16 equal logits at the top
        rows.append(torch.randint(0, 16, (V,), generator=g).float() * .5)
        kinds.append('quantised')
    for _ in range(2):  # 16 levels of a normal: few at the top, many around the k-th value
        rows.append((torch.randn(V, generator=g) * 2).round().clamp(-8, 7) * .5)
        kinds.append('quantised')
    rows.append(torch.full((V,), 1.25)); kinds.append('equal')
    ramp = torch.arange(V).float() * (8. / V)
    rows.append(ramp); kinds.append('ascending')
    rows.append(ramp.flip(0)); kinds.append('descending')
    for w in range(4):  # the k largest in lanes of wave w: indices 64 w + l + 256 j
        x = normal()
        idx = torch.arange(V)
        lanes = idx[(idx % 256) // 64 == w]
        pick = lanes[torch.randperm(len(lanes), generator=g)[:k]]
        x[pick] += 40
        rows.append(x); kinds.append('one wave')
    return torch.stack(rows).float(), kinds


def forced(k):
    """allennlp's candidates of a finished beam: 0 at <stop>, finfo.min at the lowest others."""
    v = torch.full((k,), FMIN)
    v[0] = 0.
    i = torch.tensor([STOP] + [j - 1 if j - 1 < STOP else j for j in range(1, k)],
                     dtype=torch.int32)
    return v, i


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def check_against_float64(cand_v, cand_i, want64, k, what):
    """want64 (rows, V): the float64 scores.  No position is skipped."""
    cand_v, cand_i = cand_v.cpu().double(), cand_i.cpu().long()
    V = want64.shape[1]
    assert bool(((cand_i >= 0) & (cand_i < V)).all()), what
    for r in range(cand_i.shape[0]):
        assert len(set(cand_i[r].tolist())) == k, (what, r, 'indices repeat')
    at = want64.gather(1, cand_i)
    err_at = (at - cand_v).abs().max().item()
    top = want64.sort(dim=1, descending=True).values[:, :k]
    err_top = (top - cand_v).abs().max().item()
    print(f'{what}: |f64 at cand_i - cand_v| {err_at:.3g}, |f64 top-k - cand_v| {err_top:.3g}')
    assert err_at <= TOL and err_top <= TOL, what


@functools.lru_cache(maxsize=None)
def case(V, k):
    logits, kinds = rows_for(V, k, seed=V * 1000 + k)
    return logits, kinds, torch.log_softmax(logits.double(), dim=1)


@pytest.mark.parametrize('V,k', SHAPES)
def test_every_path_gives_the_same_bits_and_the_float64_top_k(V, k):
    logits, kinds, want64 = case(V, k)
    dev = logits.cuda()
    got_v, got_i = hip.row_select(dev, k)
    for path in PATHS:
        v, i = hip.row_select(dev, k, path=path)
        assert torch.equal(bits(v), bits(got_v)), (path, 'cand_v')
        assert torch.equal(i.cpu(), got_i.cpu()), (path, 'cand_i')
    check_against_float64(got_v, got_i, want64, k, f'V={V} k={k}')
    equal = kinds.index('equal')  # ties: the lowest indices win
    assert got_i[equal].cpu().tolist() == list(range(k))
    assert bool((got_v[:, :-1] >= got_v[:, 1:]).all())


@pytest.mark.parametrize('V,k', SHAPES)
def test_finished_rows_among_live_ones(V, k):
    logits, kinds, want64 = case(V, k)
    rows = logits.shape[0]
    last_tok = torch.arange(rows) % 5 + 1      # STOP = 3 on every fifth row
    last_tok[0] = STOP
    done = last_tok == STOP
    assert bool(done.any()) and not bool(done.all())
    dev, tok = logits.cuda(), last_tok.cuda()
    got_v, got_i = hip.row_select(dev, k, last_tok=tok, stop=STOP)
    for path in PATHS:
        v, i = hip.row_select(dev, k, last_tok=tok, stop=STOP, path=path)
        assert torch.equal(bits(v), bits(got_v)), (path, 'cand_v')
        assert torch.equal(i.cpu(), got_i.cpu()), (path, 'cand_i')
    fv, fi = forced(k)
    assert torch.equal(bits(got_v[done]), bits(fv.expand(int(done.sum()), k)))
    assert torch.equal(got_i[done].cpu(), fi.expand(int(done.sum()), k))
    # the live rows are what they are without last_tok
    live_v, live_i = hip.row_select(dev, k)
    assert torch.equal(bits(got_v[~done]), bits(live_v[~done]))
    assert torch.equal(got_i[~done].cpu(), live_i[~done].cpu())


def test_language_model_term_at_the_workload_shape():
    V, k, lam = 5004, 50, 0.2
    logits, kinds, want64 = case(V, k)
    g = torch.Generator().manual_seed(7)
    lm = torch.randn(logits.shape, generator=g) * 3
    lm[5] = (lm[5] * 2).round() * .5           # ties in the LM term too
    want = want64 - float(torch.tensor(lam)) * torch.log_softmax(lm.double(), dim=1)
    dev, lmdev = logits.cuda(), lm.cuda()
    got_v, got_i = hip.row_select(dev, k, lm_logits=lmdev, lam=lam)
    for path in PATHS:
        v, i = hip.row_select(dev, k, lm_logits=lmdev, lam=lam, path=path)
        assert torch.equal(bits(v), bits(got_v)), (path, 'cand_v')
        assert torch.equal(i.cpu(), got_i.cpu()), (path, 'cand_i')
    check_against_float64(got_v, got_i, want, k, 'lm term')


def test_a_path_refuses_a_shape_it_does_not_take():
    x = torch.randn(2, 7000).cuda()             # above the register kernel's 6144
    for path in ('threshold', 'legacy'):
        with pytest.raises(ValueError, match='vocab_size'):
            hip.row_select(x, 50, path=path)
    with pytest.raises(ValueError, match='k='):
        hip.row_select(x[:, :40].contiguous(), 50)
