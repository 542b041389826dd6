"""The streaming attention kernel alone (milan_attention through hip.attention) against
float64 softmax attention (vitref.attention).

Bound, as everywhere in the ViT tests: max|got - want| <= max(4 x e32, FEATURE_CLASS x
max|want|), e32 = the error of the same function in float32 on the CPU.  The tests print the
measured multiple of the bound (`VIT ...` lines); DESIGN 4.24 quotes the worst.
"""
import pytest
import torch

import vitref
from milan_amd import hip

pytestmark = pytest.mark.gpu


def gaussian(seqs, T, heads, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(seqs, T, 3 * heads * hd, generator=g, dtype=torch.float64)


def run(qkv64, heads):
    return hip.attention(qkv64.float().cuda(), heads)


def check(what, qkv64, heads):
    want = vitref.attention(qkv64, heads)
    ref32 = vitref.attention(qkv64.float(), heads)
    got = run(qkv64, heads)
    return vitref.check(what, got, want, ref32), got


def test_every_length_from_1_to_130():
    """One sequence, 2 heads of size 16: crosses every boundary of a 16-, 32- or 64-wide tile
    and of the 128-row query tile."""
    worst = 0.
    for T in range(1, 131):
        ratio, _ = check(f'attention T={T}', gaussian(1, T, 2, 16, seed=T), 2)
        worst = max(worst, ratio)
    print(f'VIT attention T=1..130: worst {worst:.3f} x bound')


@pytest.mark.parametrize('seqs,T,heads,hd', [(3, 197, 2, 32), (2, 257, 1, 64), (2, 785, 6, 64),
                                              (1, 1025, 1, 128), (2, 50, 3, 48)])
def test_shapes(seqs, T, heads, hd):
    check(f'attention {seqs}x{T}x{heads}x{hd}', gaussian(seqs, T, heads, hd, seed=T + hd), heads)


# ---- constructed cases at T = 200, head size 16 ------------------------------------------
T0, HD0, HEADS0 = 200, 16, 2


def directed(levels, seed):
    """qkv whose scores are q_t . k_j / 4 ~ 4 x levels[j] (+ noise of order 0.02 x levels): q is the
    ones vector and k_j is levels[j] x the ones vector, both with a little Gaussian noise."""
    qkv = gaussian(1, T0, HEADS0, HD0, seed)
    W = HEADS0 * HD0
    noise = .02 * qkv[..., :2 * W]
    qkv[..., :W] = 1. + noise[..., :W]
    qkv[..., W:2 * W] = levels.reshape(1, T0, 1) + noise[..., W:]
    return qkv


def scores(qkv):
    W = HEADS0 * HD0
    q = qkv[0, :, :HD0]
    k = qkv[0, :, W:W + HD0]
    return q @ k.T / 4.


def test_a_late_key_dominates():
    """Key 197, in the last partial tile, scores 60 above every earlier key: the running-max
    rescale must shrink everything accumulated before it."""
    g = torch.Generator().manual_seed(5)
    levels = torch.rand(T0, generator=g, dtype=torch.float64) * 2 - 1
    levels[197] = 17.
    qkv = directed(levels, seed=50)
    s = scores(qkv)
    assert float((s[:, 197] - s[:, :197].max(dim=1)[0]).min()) > 60
    check('attention late key', qkv, HEADS0)


def test_the_maximum_is_in_the_first_tile():
    """Key 3 has the maximum and every other score is 100 below: later tiles add nothing."""
    levels = torch.full((T0,), -26., dtype=torch.float64)
    levels[3] = 0.
    qkv = directed(levels, seed=51)
    s = scores(qkv)
    assert float((s[:, 3:4] - s[:, 4:]).min()) > 100
    _, got = check('attention first-tile maximum', qkv, HEADS0)
    W = HEADS0 * HD0
    # the softmax weight of every other key is below 1e-43: the output is v_3 to the last bit
    assert torch.equal(got.cpu(), qkv[:, 3:4, 2 * W:].float().expand(-1, T0, -1))


def test_scores_of_magnitude_150():
    """An unshifted exp overflows float32 at 89."""
    g = torch.Generator().manual_seed(6)
    signs = torch.randint(0, 2, (T0,), generator=g).double() * 2 - 1
    qkv = directed(37.5 * signs, seed=52)
    assert float(scores(qkv).abs().min()) > 140
    check('attention scores of 150', qkv, HEADS0)


def test_zero_queries_give_the_exact_mean():
    g = torch.Generator().manual_seed(7)
    T, W = 256, HEADS0 * HD0
    qkv = torch.zeros(1, T, 3 * W, dtype=torch.float64)
    qkv[..., W:2 * W] = torch.randn(1, T, W, generator=g, dtype=torch.float64)
    qkv[..., 2 * W:] = torch.randint(-50, 51, (1, T, W), generator=g).double()
    mean = qkv[..., 2 * W:].mean(dim=1, keepdim=True).expand(-1, T, -1)
    assert torch.equal(mean.float().double(), mean)  # representable: a sum of integers / 256
    assert torch.equal(run(qkv, HEADS0).cpu().double(), mean)


def test_values_distinct_per_key_and_column():
    """A transposed P V, or rows and columns swapped in the store, cannot pass."""
    qkv = gaussian(2, T0, HEADS0, HD0, seed=53)
    W = HEADS0 * HD0
    distinct = torch.arange(T0 * W, dtype=torch.float64).reshape(1, T0, W) / 64.
    qkv[..., 2 * W:] = torch.stack((distinct[0], -distinct[0].flip(0)))
    check('attention distinct values', qkv, HEADS0)


# ---- properties --------------------------------------------------------------------------
def test_a_sequence_does_not_depend_on_its_batch():
    for T, heads, hd in ((197, 2, 32), (130, 2, 64)):
        qkv = gaussian(3, T, heads, hd, seed=60).float().cuda()
        batch = hip.attention(qkv, heads)
        alone = hip.attention(qkv[1:2].contiguous(), heads)
        assert torch.equal(batch[1:2], alone)


def test_two_runs_give_the_same_bits():
    qkv = gaussian(2, 785, 6, 64, seed=61).float().cuda()
    assert torch.equal(hip.attention(qkv, 6), hip.attention(qkv, 6))


def test_other_head_sizes_are_refused():
    qkv = torch.zeros(1, 10, 3 * 40, device='cuda')
    with pytest.raises(ValueError, match='head size 20'):
        hip.attention(qkv, 2)
    with pytest.raises(ValueError, match='head size 144'):
        hip.attention(torch.zeros(1, 10, 3 * 144, device='cuda'), 1)
    torch.cuda.synchronize()
