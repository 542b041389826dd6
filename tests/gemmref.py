"""What one GemmArgs launch computes (csrc/gemm_plan.h), restated in float64 with plain torch.

    C[m][q * N + n] = epi( sum_k A(m, q)[k] * W[q][n][k] + bias[q][n], aux[m][q * N + n] )

Row m = (image, ho, wo).  A(m, q) is the implicit im2col row of group q: k = (kh, kw, c) with c
fastest over the group's Cin channels of the input pixel (ho * stride - pad + kh, wo * stride_w -
pad_w + kw), zero outside the image (stride_w / pad_w = stride / pad unless anisotropic), followed
by the channels of the second source's pixel (ho * stride2, wo * stride2) when there is one.

The operands are the values the device buffers HOLD (tests/splitfmt.py: from_split of what was
uploaded), so that the quantisation of the inputs is not counted as an error of the kernel.
"""
import torch

EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RES_RELU, EPI_BIAS_TANH, EPI_BIAS_SIGMUL, EPI_BIAS_ADD = range(6)
EPILOGUES = ('bias', 'relu', 'res_relu', 'tanh', 'sigmul', 'add')   # (gemm_plan_dump's names)
USES_AUX = (EPI_BIAS_RES_RELU, EPI_BIAS_SIGMUL, EPI_BIAS_ADD)


def out_extent(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def im2col(x, kh, kw, stride, pad, stride_w=None, pad_w=None):
    """x (images, H, W, C) -> (images * Ho * Wo, kh * kw * C), k = (tap, channel)"""
    stride_w = stride if stride_w is None else stride_w
    pad_w = pad if pad_w is None else pad_w
    n, h, w, c = x.shape
    ho, wo = out_extent(h, kh, stride, pad), out_extent(w, kw, stride_w, pad_w)
    padded = x.new_zeros(n, h + 2 * pad + kh, w + 2 * pad_w + kw, c)
    padded[:, pad:pad + h, pad_w:pad_w + w] = x
    taps = []
    for i in range(kh):
        for j in range(kw):
            taps.append(padded[:, i:i + (ho - 1) * stride + 1:stride,
                               j:j + (wo - 1) * stride_w + 1:stride_w])
    return torch.stack(taps, dim=3).reshape(n * ho * wo, kh * kw * c)


def operand_rows(x, kh, kw, stride, pad, groups=1, x2=None, stride2=1, stride_w=None, pad_w=None):
    """[groups] matrices (M, K): the rows A(m, q).  x (images, H, W, groups * Cin); x2 (images,
    H2, W2, C2) or None (one group only)."""
    n, h, w, c = x.shape
    cin = c // groups
    ho = out_extent(h, kh, stride, pad)
    wo = out_extent(w, kw, stride if stride_w is None else stride_w,
                    pad if pad_w is None else pad_w)
    rows = [im2col(x[..., q * cin:(q + 1) * cin], kh, kw, stride, pad, stride_w, pad_w)
            for q in range(groups)]
    if x2 is not None:
        assert groups == 1
        second = x2[:, ::stride2, ::stride2][:, :ho, :wo]
        assert second.shape[1:3] == (ho, wo), (second.shape, ho, wo)
        rows[0] = torch.cat([rows[0], second.reshape(n * ho * wo, -1)], dim=1)
    return rows


def epilogue(acc, epi, aux=None):
    if epi == EPI_BIAS:
        return acc
    if epi == EPI_BIAS_RELU:
        return acc.clamp_min(0)
    if epi == EPI_BIAS_RES_RELU:
        return (acc + aux).clamp_min(0)
    if epi == EPI_BIAS_TANH:
        return torch.tanh(acc)
    if epi == EPI_BIAS_SIGMUL:
        return torch.sigmoid(acc) * aux
    if epi == EPI_BIAS_ADD:
        return acc + aux
    raise ValueError(epi)


def gemm(x, w, bias=None, aux=None, epi=EPI_BIAS, kh=1, kw=1, stride=1, pad=0, groups=1,
         x2=None, stride2=1, stride_w=None, pad_w=None):
    """Every row of the launch in float64: (want, pre, mag), each (M, groups * N).
    w (groups, N, K); bias (groups * N) or None; aux (M, groups * N) or None.
    pre = the pre-activation acc + bias (what TANH / SIGMUL apply their function to);
    mag = sum_k |A| |W| + |bias| + |aux|, the magnitude an fp32 accumulation bound scales with."""
    x, w = x.double(), w.double()
    x2 = None if x2 is None else x2.double()
    g, n, k = w.shape
    assert g == groups
    rows = operand_rows(x, kh, kw, stride, pad, groups, x2, stride2, stride_w, pad_w)
    assert rows[0].shape[1] == k, (rows[0].shape, k)
    pre = torch.cat([rows[q] @ w[q].t() for q in range(g)], dim=1)
    mag = torch.cat([rows[q].abs() @ w[q].abs().t() for q in range(g)], dim=1)
    if bias is not None:
        pre = pre + bias.double()
        mag = mag + bias.double().abs()
    if epi in USES_AUX:
        aux = aux.double()
        if epi != EPI_BIAS_SIGMUL:
            mag = mag + aux.abs()
    return epilogue(pre, epi, aux), pre, mag


def live_rows(m, m_live=None, m_live_mul=1, row_list=None):
    """the rows a launch sized for `m` writes: a LongTensor, ascending"""
    if row_list is not None:
        return torch.as_tensor(row_list[:m_live], dtype=torch.long)
    if m_live is None:
        return torch.arange(m)
    return torch.arange(max(0, min(m, m_live * m_live_mul)))
