"""The SAGAN / BigGAN attention kernel alone (milan_sagan_attention through
hip.sagan_attention) against float64 softmax attention (bigganref.attention).

Bound, as in the ViT tests: max|got - want| <= max(4 x e32, FEATURE_CLASS x max|want|), e32 =
the error of the same function in float32 on the CPU.  The tests print the measured multiple
of the bound (`BIGGAN ...` lines); DESIGN 4.26 quotes the worst.

Sizes: H x W pixels give H W queries and H W / 4 keys, streamed 32 keys at a time; C channels
give dk = C / 8 and dv = C / 2 (C = 32: one half-filled block of O; 64: one block; 192: three;
384: six).
"""
import pytest
import torch

import bigganref
from milan_amd import hip

pytestmark = pytest.mark.gpu


def run(theta64, phi_g64, H, W):
    return hip.sagan_attention(theta64.float().cuda(), phi_g64.float().cuda(), H, W)


def check(what, theta, phi_g, H, W):
    want = bigganref.attention(theta, phi_g)
    ref32 = bigganref.attention(theta.float(), phi_g.float())
    got = run(theta, phi_g, H, W)
    return bigganref.check(what, got, want, ref32), got


# 1, 9, 25, 64 and 144 keys: one key, fewer than a tile, a partial last tile, exact tiles,
# several tiles (and 4 .. 576 queries: under one wave, a partial and several query tiles)
@pytest.mark.parametrize('C', [32, 64, 192])
@pytest.mark.parametrize('side', [2, 6, 10, 16, 24])
def test_sizes(side, C):
    theta, phi_g = bigganref.inputs(2, side, side, C, seed=side * 1000 + C)
    check(f'attention {side}x{side} C={C}', theta, phi_g, side, side)


@pytest.mark.parametrize('H,W,C,n', [(8, 4, 64, 2), (4, 8, 96, 2), (8, 8, 384, 2),
                                     (12, 12, 352, 1), (64, 64, 192, 1)])
def test_shapes(H, W, C, n):
    """Non-square images, the widest block (six accumulator blocks), a width whose last block
    is half filled beside five full ones, and the production width at 4096 queries x 1024
    keys."""
    theta, phi_g = bigganref.inputs(n, H, W, C, seed=H * W + C)
    check(f'attention {H}x{W} C={C}', theta, phi_g, H, W)


def test_every_supported_width():
    worst = 0.
    for C in range(32, 385, 32):
        theta, phi_g = bigganref.inputs(1, 10, 14, C, seed=C)
        ratio, _ = check(f'attention 10x14 C={C}', theta, phi_g, 10, 14)
        worst = max(worst, ratio)
    print(f'BIGGAN attention C=32..384: worst {worst:.3f} x bound')


def test_theta_is_read_in_place_from_a_fused_conv_output():
    """The first dk columns of a theta | phi | g tensor, row stride dk + dk + dv."""
    H = W = 10
    theta, phi_g = bigganref.inputs(2, H, W, 192, seed=70)
    dk = theta.shape[2]
    fused = torch.full((2, H * W, 6 * dk), float('nan'), device='cuda')
    fused[..., :dk] = theta.float().cuda()
    view = fused[..., :dk]
    assert not view.is_contiguous()
    got = hip.sagan_attention(view, phi_g.float().cuda(), H, W)
    assert torch.equal(got, run(theta, phi_g, H, W))


# ---- constructed cases at 20 x 20 pixels, C = 32: 400 queries, 100 keys, dk = 4 ------------
H0 = W0 = 20
C0, TQ0, TK0, DK0 = 32, 400, 100, 4


def directed(levels, seed):
    """Inputs whose scores are theta_i . phi_j ~ 4 x levels[j] (+ noise of order 0.04 x
    levels): theta is the ones vector and phi_j is levels[j] x the ones vector, both with a
    little Gaussian noise."""
    theta, phi_g = bigganref.inputs(1, H0, W0, C0, seed)
    theta = 1. + .02 * theta
    phi_g[..., :DK0] = levels.reshape(1, TK0, 1) + .02 * phi_g[..., :DK0]
    return theta, phi_g


def scores(theta, phi_g):
    return theta[0] @ phi_g[0, :, :DK0].T


def test_a_late_key_dominates():
    """Key 98, in the last partial tile, scores 60 above every earlier key: the running-max
    rescale must shrink everything accumulated before it."""
    g = torch.Generator().manual_seed(5)
    levels = torch.rand(TK0, generator=g, dtype=torch.float64) * 2 - 1
    levels[98] = 18.
    theta, phi_g = directed(levels, seed=50)
    s = scores(theta, phi_g)
    assert float((s[:, 98] - s[:, :98].max(dim=1)[0]).min()) > 60
    check('attention late key', theta, phi_g, H0, W0)


def test_the_maximum_is_in_the_first_tile():
    """Key 3 has the maximum and every other score is 100 below: later tiles add nothing."""
    levels = torch.full((TK0,), -28., dtype=torch.float64)
    levels[3] = 0.
    theta, phi_g = directed(levels, seed=51)
    s = scores(theta, phi_g)
    assert float((s[:, 3:4] - s[:, 4:]).min()) > 100
    _, got = check('attention first-tile maximum', theta, phi_g, H0, W0)
    # the softmax weight of every other key is below 1e-43: the output is g_3 to the last bit
    assert torch.equal(got.cpu(), phi_g[:, 3:4, DK0:].float().expand(-1, TQ0, -1))


def test_scores_of_magnitude_150():
    """There is no 1 / sqrt(dk) here, and an unshifted exp overflows float32 at 89."""
    g = torch.Generator().manual_seed(6)
    signs = torch.randint(0, 2, (TK0,), generator=g).double() * 2 - 1
    theta, phi_g = directed(37.5 * signs, seed=52)
    assert float(scores(theta, phi_g).abs().min()) > 140
    check('attention scores of 150', theta, phi_g, H0, W0)


def test_zero_queries_give_the_exact_mean():
    g = torch.Generator().manual_seed(7)
    H = W = 32  # 256 keys
    theta, phi_g = bigganref.inputs(1, H, W, C0, seed=8)
    theta = torch.zeros_like(theta)
    phi_g[..., DK0:] = torch.randint(-50, 51, phi_g[..., DK0:].shape, generator=g).double()
    mean = phi_g[..., DK0:].mean(dim=1, keepdim=True).expand(-1, H * W, -1)
    assert torch.equal(mean.float().double(), mean)  # representable: a sum of integers / 256
    assert torch.equal(run(theta, phi_g, H, W).cpu().double(), mean)


def test_values_distinct_per_key_and_column():
    """A transposed P V, or rows and columns swapped in the store, cannot pass."""
    theta, phi_g = bigganref.inputs(2, H0, W0, 64, seed=53)
    dk, dv = bigganref.widths(64)
    distinct = torch.arange(TK0 * dv, dtype=torch.float64).reshape(TK0, dv) / 64.
    phi_g[..., dk:] = torch.stack((distinct, -distinct.flip(0)))
    check('attention distinct values', theta, phi_g, H0, W0)


# ---- properties --------------------------------------------------------------------------
def test_an_image_does_not_depend_on_its_batch():
    for side, C in ((14, 192), (18, 96)):
        theta, phi_g = (t.float().cuda() for t in bigganref.inputs(3, side, side, C, seed=60))
        batch = hip.sagan_attention(theta, phi_g, side, side)
        alone = hip.sagan_attention(theta[1:2].contiguous(), phi_g[1:2].contiguous(), side, side)
        assert torch.equal(batch[1:2], alone)


def test_two_runs_give_the_same_bits():
    theta, phi_g = (t.float().cuda() for t in bigganref.inputs(2, 24, 24, 192, seed=61))
    assert torch.equal(hip.sagan_attention(theta, phi_g, 24, 24),
                       hip.sagan_attention(theta, phi_g, 24, 24))


def test_other_shapes_are_refused():
    def zeros(H, W, dk):
        return (torch.zeros(1, H * W, dk, device='cuda'),
                torch.zeros(1, H * W // 4, 5 * dk, device='cuda'))

    with pytest.raises(ValueError, match='channels 40 '):  # dk = 5
        hip.sagan_attention(*zeros(4, 4, 5), 4, 4)
    with pytest.raises(ValueError, match='channels 48 '):  # dk = 6: not a multiple of 4
        hip.sagan_attention(*zeros(4, 4, 6), 4, 4)
    with pytest.raises(ValueError, match='channels 416 '):
        hip.sagan_attention(*zeros(4, 4, 52), 4, 4)
    with pytest.raises(ValueError, match='height 3 '):
        hip.sagan_attention(*zeros(3, 4, 4), 3, 4)
    with pytest.raises(ValueError, match='a quarter of it'):  # keys of another image size
        hip.sagan_attention(torch.zeros(1, 24, 4, device='cuda'),
                            torch.zeros(1, 4, 20, device='cuda'), 4, 6)
    with pytest.raises(ValueError, match='width 5 '):
        hip.sagan_attention(torch.zeros(1, 20, 4, device='cuda'),
                            torch.zeros(1, 5, 20, device='cuda'), 4, 5)
    torch.cuda.synchronize()
    # the library is still usable
    theta, phi_g = bigganref.inputs(1, 4, 4, 32, seed=62)
    check('attention after refusals', theta, phi_g, 4, 4)
