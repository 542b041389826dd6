"""tests/gemmref.py against torch's float64 convolution; tests/splitfmt.py's round trips (CPU)."""
import pytest
import torch
import torch.nn.functional as F

import gemmref
import splitfmt


def oihw(w, kh, kw):
    """(groups, N, K = (tap, channel)) -> (groups * N, Cin, kh, kw)"""
    g, n, k = w.shape
    return w.reshape(g * n, kh, kw, k // (kh * kw)).permute(0, 3, 1, 2).contiguous()


CONVS = [
    # images, H, W, Cin/group, N/group, kh, kw, stride, pad, groups
    (2, 7, 5, 4, 3, 3, 3, 1, 1, 1),
    (3, 9, 6, 8, 5, 3, 3, 2, 1, 1),
    (1, 11, 13, 4, 6, 5, 5, 1, 2, 2),
    (2, 8, 8, 12, 4, 1, 1, 2, 0, 3),
    (2, 6, 9, 4, 7, 7, 7, 2, 3, 1),
    (2, 5, 4, 8, 8, 2, 3, 1, 0, 2),
]


@pytest.mark.parametrize('case', CONVS)
def test_gemm_is_conv2d(case):
    n, h, w, cin, cout, kh, kw, stride, pad, groups = case
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, h, w, cin * groups, generator=gen, dtype=torch.float64)
    wt = torch.randn(groups, cout, kh * kw * cin, generator=gen, dtype=torch.float64)
    bias = torch.randn(groups * cout, generator=gen, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), oihw(wt, kh, kw), bias, stride, pad, groups=groups)
    want = want.permute(0, 2, 3, 1).reshape(-1, groups * cout)
    aux = torch.randn(want.shape, generator=gen, dtype=torch.float64)
    got, pre, mag = gemmref.gemm(x, wt, bias, None, gemmref.EPI_BIAS, kh, kw, stride, pad, groups)
    assert got.shape == want.shape
    assert (got - want).abs().max() <= 1e-12 * mag.max()
    assert torch.equal(got, pre) and (mag >= got.abs() - 1e-12).all()
    for epi, fn in ((gemmref.EPI_BIAS_RELU, lambda v: v.clamp_min(0)),
                    (gemmref.EPI_BIAS_RES_RELU, lambda v: (v + aux).clamp_min(0)),
                    (gemmref.EPI_BIAS_TANH, torch.tanh),
                    (gemmref.EPI_BIAS_SIGMUL, lambda v: aux / (1 + torch.exp(-v))),
                    (gemmref.EPI_BIAS_ADD, lambda v: v + aux)):
        out = gemmref.gemm(x, wt, bias, aux, epi, kh, kw, stride, pad, groups)[0]
        assert (out - fn(want)).abs().max() <= 1e-12 * mag.max(), epi


def test_anisotropic_stride_and_pad():
    """the pixel-pair stem's class: stride 2 / pad 3 down, stride 1 / pad 1 across, 7 x 4 taps on
    a non-square input"""
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 13, 6, 8, generator=gen, dtype=torch.float64)
    wt = torch.randn(1, 5, 7 * 4 * 8, generator=gen, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), oihw(wt, 7, 4), None, (2, 1), (3, 1))
    got = gemmref.gemm(x, wt, kh=7, kw=4, stride=2, pad=3, stride_w=1, pad_w=1)[0]
    assert want.shape[2:] == (7, 5)
    assert (got - want.permute(0, 2, 3, 1).reshape(-1, 5)).abs().max() <= 1e-12 * got.abs().max()


@pytest.mark.parametrize('stride2', (1, 2))
def test_second_source_is_a_strided_1x1_conv_added(stride2):
    """K-concatenation: conv(x, W[:, :K1]) + conv1x1(x2, W[:, K1:], stride2), x2 non-square"""
    gen = torch.Generator().manual_seed(stride2)
    ho, wo = 5, 3
    h2, w2 = (ho - 1) * stride2 + 1, (wo - 1) * stride2 + 1 + (stride2 - 1)   # (one spare column)
    x = torch.randn(2, ho, wo, 8, generator=gen, dtype=torch.float64)
    x2 = torch.randn(2, h2, w2, 12, generator=gen, dtype=torch.float64)
    wt = torch.randn(1, 6, 8 + 12, generator=gen, dtype=torch.float64)
    first = F.conv2d(x.permute(0, 3, 1, 2), oihw(wt[:, :, :8], 1, 1))
    second = F.conv2d(x2.permute(0, 3, 1, 2), oihw(wt[:, :, 8:], 1, 1), stride=stride2)
    want = (first + second[:, :, :ho, :wo]).permute(0, 2, 3, 1).reshape(-1, 6)
    got = gemmref.gemm(x, wt, x2=x2, stride2=stride2)[0]
    assert (got - want).abs().max() <= 1e-12 * got.abs().max()


def test_live_rows():
    assert gemmref.live_rows(10).tolist() == list(range(10))
    assert gemmref.live_rows(10, 0, 4).tolist() == []
    assert gemmref.live_rows(10, 2, 4).tolist() == list(range(8))
    assert gemmref.live_rows(10, 3, 4).tolist() == list(range(10))
    assert gemmref.live_rows(10, 2, 1, [1, 4, 7, 9]).tolist() == [1, 4]


# ---- the split format ---------------------------------------------------------------------------
def test_split_round_trip():
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(7, 24, generator=gen) * 3
    packed, held = splitfmt.to_split(x)
    assert packed.shape == x.shape and packed.dtype == torch.float32
    assert torch.equal(splitfmt.from_split(packed), held)
    # hi + lo carries ~22 bits of x
    assert ((held - x.double()).abs() <= x.double().abs() * 2.0 ** -21 + 2.0 ** -25).all()
    # what the buffer holds splits again to itself
    again, held2 = splitfmt.to_split(held.float())
    assert torch.equal(again, packed) and torch.equal(held2, held)


@pytest.mark.parametrize('k', (0, 5, -3))
def test_split_scale_argument(k):
    gen = torch.Generator().manual_seed(k + 10)
    x = torch.randn(3, 16, generator=gen)
    packed, held = splitfmt.to_split(x, k)
    assert torch.equal(splitfmt.from_split(packed, k), held)
    # a power-of-two scale moves the exponent only
    unscaled, held0 = splitfmt.to_split(x * 2.0 ** k)
    assert torch.equal(packed, unscaled) and torch.equal(held, held0 / 2.0 ** k)


def test_split_subnormal_lo_half():
    """x = 1 + 2^-20: hi = 1, lo = 2^-20 -- below f16's smallest normal 2^-14, a subnormal that is
    still exact; so is x = 1 + 2^-23, two steps of the subnormal grid 2^-24"""
    x = torch.zeros(1, 8)
    x[0, 0] = 1 + 2.0 ** -20
    x[0, 1] = 1 + 2.0 ** -23
    packed, held = splitfmt.to_split(x)
    halves = packed.view(torch.float16).view(1, 2, 8)
    assert halves[0, 0, 0] == 1 and halves[0, 1, 0] == 2.0 ** -20
    assert 0 < float(halves[0, 1, 0]) < 2.0 ** -14
    assert held[0, 0] == 1 + 2.0 ** -20
    assert held[0, 1] == 1 + 2.0 ** -23 and torch.equal(splitfmt.from_split(packed), held)


def test_split_clamps_at_the_largest_f16():
    x = torch.zeros(1, 8)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 7e4, -1e9, 65504., 2100.
    packed, held = splitfmt.to_split(x)
    assert held[0, :4].tolist() == [65504., -65504., 65504., 2100.]
    assert torch.isfinite(splitfmt.from_split(packed)).all()
    # at scale 2^5 the clamp is at 65504 / 32 = 2047
    packed, held = splitfmt.to_split(x, 5)
    assert held[0, :4].tolist() == [2047., -2047., 2047., 2047.]
