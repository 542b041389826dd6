"""Every product kernel form of the implicit GEMM against float64, at its edge shapes.

tests/gemm_forms.py is the case table; each case is ONE launch through hip.gemm_probe (every
launcher argument in the test's hand) of the kernel the case names -- asserted first, against
tools/gemm_plan_dump.cpp's plan of the same arguments with this device's CU count.  The reference
is tests/gemmref.py (float64) on the values the device buffers hold.

Per case:
 1. fp32 forms (fp32 operands): elementwise |got - want| <= (K + 8) 2^-24 (|A| |W| + |bias| +
    |aux|) for the epilogues 0, 1, 2, 5 -- K fp32 additions and the epilogue's, nothing measured.
    TANH and SIGMUL apply tanhf / expf to that: their pre-activation carries the bound above times
    the function's largest slope (1; |aux| / 4), and the function itself is allowed TANH_ULPS /
    SIGMUL_ULPS units in the last place of the fp32 result: twice the maximum measured on an
    MI355X against float64 on the kernel's own fp32 pre-activations (epilogue 0 of the same
    launch) over the fp32-output cases of the table: tanhf 1.32 ulp (157,284 values, the worst
    at |x| = 0.64), (1 / (1 + expf(-x))) * aux 2.32 ulp (140,836 values) --
    profiles/gemm_forms.txt.
 2. split forms (split-f16 operands), the standing rule of test_gpu_parity.py: err_split <=
    max(4 err_f32, 2e-6 scale) and err_split <= 1e-5 scale, err = max |got - want| over the
    launch, scale = max |want|, err_f32 = the fp32 general kernel on the SAME held operands (a
    Linear over the explicit im2col rows), itself held to 1.  Split OUTPUT adds at most 2^-22 |v|
    + 2^-25 per value: below the 2e-6 scale floor for the unit-scale operands used here (|v| <=
    scale, 2^-22 = 2.4e-7).
 3. Nothing else is written: C sits at a column offset of a wider row between guard rows, all
    pre-filled with a sentinel bit pattern; everything but the live rows' slice keeps it.
 4. Dead rows are not read into live ones: every operand pixel that no live row reads, and every
    word of the wider operand rows outside the slice, holds 60000; the status word stays 0.
 5. Saturation: one output beyond 65504 sets MILAN_STATUS_SATURATED and holds the clamp, the
    others keep their bound; the same launch with the value just inside leaves the word 0.
 6. The bit-equalities csrc/gemm_plan.h promises: list = dense, live = full, grouped = per group,
    class tiles = linear order, knob forms = default forms.
 7. Permutation-like weights on distinct small integers: every value exact, torch.equal.

The knob forms run in one fresh child process per setting (the knobs are read once per process).
"""
import math
import os
import pathlib
import re
import subprocess
import sys
import zlib

import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
if __name__ == '__main__':   # (a knob child: no conftest)
    for p in (REPO / 'tests', REPO, REPO / 'neuron-descriptions_amd'):
        sys.path.insert(0, str(p))

import gemm_forms  # noqa: E402
import gemmref  # noqa: E402
import splitfmt  # noqa: E402
from gemm_forms import CASES, SAME_BITS, by_id, geometry  # noqa: E402
from milan_amd import hip  # noqa: E402
from test_gemm_plan_host import dump  # noqa: E402,F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fa5c3d2   # (a NaN as fp32, two NaNs as f16: a stray read of it shows as well)
POISON = 60000.0        # finite, exact in f16, below the clamp
GUARD = 8               # rows of C before and after the launch's
TANH_ULPS, SIGMUL_ULPS = 2 * 1.32, 2 * 2.32
SATURATED = 1           # MILAN_STATUS_SATURATED
SAT_ROW_FRACTION, SAT_COL, SAT_CH = 0.5, 5, 3


# ---- a case's operands: CPU tensors, deterministic in the case's id ------------------------------
def listed_rows(spec, m, howo, gen):
    if spec == 'all':
        return list(range(m))
    if spec == 'one':
        return [m // 2 + 17]
    if spec == 'gaps':
        return [r for r in range(m) if (r // howo) % 3 != 2 and (r * 7) % 5 != 0]
    return sorted(torch.randperm(m, generator=gen)[:spec].tolist())


def held_split(t2d, scale_log2=0):
    packed, held = splitfmt.to_split(t2d, scale_log2)
    assert torch.equal(held.float().double(), held)   # (hi + lo is an fp32 value)
    return packed, held


def widen(rows, col, stride, split):
    """(P, C) words -> (P, stride) with the slice at `col` and POISON everywhere else"""
    p, c = rows.shape
    wide = torch.full((p, stride), POISON)
    if split:
        wide = splitfmt.to_split(wide)[0]
    wide[:, col:col + c] = rows
    return wide.contiguous()


class Data:
    pass


def make_data(c, mode='random'):
    g = geometry(c)
    d = Data()
    d.c, d.g, d.mode = c, g, mode
    gen = torch.Generator().manual_seed(zlib.crc32(c['id'].encode()))
    G, N, K, M = g['groups'], g['N'], g['K'], g['M']
    GN, cin_all = G * N, G * g['Cin']
    split = bool(g['a_split'])
    npix, npix2 = g['images'] * g['H'] * g['Wd'], g['images'] * g['H2'] * g['W2d']
    x = torch.randn(npix, cin_all, generator=gen)
    x2 = torch.randn(npix2, g['C2'], generator=gen) if g['C2'] else None
    w = torch.randn(G, N, K, generator=gen) / K ** 0.5
    bias = torch.randn(GN, generator=gen)
    aux = torch.randn(M, GN, generator=gen) if g['aux_fmt'] else None
    # the rows the launch writes
    d.m_live = d.row_list = None
    if 'rows' in c:
        d.row_list = listed_rows(c['rows'], M, g['Ho'] * g['Wo'], gen)
        d.m_live, d.m_live_mul = len(d.row_list), 1
    elif 'm_live' in c:
        d.m_live, d.m_live_mul = c['m_live']
    d.live = gemmref.live_rows(M, d.m_live, getattr(d, 'm_live_mul', 1), d.row_list)

    if mode == 'perm':
        # distinct small integers through permutation-like weights: exact in every format
        pix = torch.arange(npix).view(-1, 1)
        ch = torch.arange(cin_all).view(1, -1)
        x = ((pix * 31 + ch * 7) % 251 - 125).float()
        if x2 is not None:
            pix2, ch2 = torch.arange(npix2).view(-1, 1), torch.arange(g['C2']).view(1, -1)
            x2 = ((pix2 * 29 + ch2 * 11) % 241 - 120).float()
        w = torch.zeros(G, N, K)
        for q in range(G):
            for n in range(N):
                w[q, n, (n * 5 + 3 + q) % K] = 1 + n % 3
                if x2 is not None:   # (one column of each source)
                    w[q, n, g['K1'] + (n * 3 + 1) % g['C2']] = 1 + (n + 1) % 2
        bias = (torch.arange(GN) % 7 - 3).float()
        if aux is not None:
            aux = ((torch.arange(M).view(-1, 1) * 13 + torch.arange(GN).view(1, -1) * 3) % 61
                   - 30).float()
    d.sat = None
    if mode in ('sat-over', 'sat-inside'):
        # one output beyond (or just inside) the clamp: pixel m0's channel SAT_CH is 4096 and only
        # column SAT_COL's centre tap has a weight on that channel
        assert g['stride'] == 1 and g['Ho'] == g['H'] and g['Wo'] == g['Wd'] and not g['C2']
        m0 = int(d.live[int(len(d.live) * SAT_ROW_FRACTION)])
        centre = (g['KH'] // 2) * g['KW'] + g['KW'] // 2
        x[m0, SAT_CH] = 4096.
        w[0, :, SAT_CH::g['Cin']] = 0
        w[0, SAT_COL, centre * g['Cin'] + SAT_CH] = 17. if mode == 'sat-over' else 15.
        if c.get('epi', 0) == gemmref.EPI_BIAS_SIGMUL:
            aux[m0, SAT_COL] = 7e4 if mode == 'sat-over' else 6e4
        d.sat = (m0, SAT_COL)

    # 4. every pixel no live row reads holds POISON
    def unread(n_img, h, wd, kh, kw, s, p, sw, pw):
        ids = torch.arange(1, n_img * h * wd + 1, dtype=torch.float64).view(n_img, h, wd, 1)
        read = gemmref.im2col(ids, kh, kw, s, p, sw, pw)[d.live].unique().long()
        mask = torch.ones(n_img * h * wd, dtype=torch.bool)
        mask[read[read > 0] - 1] = False
        return mask
    x[unread(g['images'], g['H'], g['Wd'], g['KH'], g['KW'], g['stride'], g['pad'],
             g['stride_w'], g['pad_w'])] = POISON
    if x2 is not None:
        ids = torch.arange(npix2, dtype=torch.float64).view(g['images'], g['H2'], g['W2d'], 1)
        read = ids[:, ::g['stride2'], ::g['stride2']][:, :g['Ho'], :g['Wo']].reshape(-1)[d.live]
        mask = torch.ones(npix2, dtype=torch.bool)
        mask[read.long()] = False
        x2[mask] = POISON

    # the values the buffers hold
    if split:
        d.x_words, d.x = held_split(x)
        if x2 is not None:
            d.x2_words, d.x2 = held_split(x2)
        # the entry point splits the weights at the library's scale: 2^e with max |w| 2^e in
        # [8192, 16384); they are given values that this split holds exactly
        amax = float(w.abs().max())
        d.w_scale_log2 = 14 - math.frexp(amax)[1] if amax > 0 else 0
        d.w = held_split(w.view(GN, K), d.w_scale_log2)[1].view(G, N, K)
        again = splitfmt.to_split(d.w.float().view(GN, K), d.w_scale_log2)[1].view(G, N, K)
        assert torch.equal(again, d.w)
    else:
        d.x_words, d.x = x, x.double()
        if x2 is not None:
            d.x2_words, d.x2 = x2, x2.double()
        d.w = w.double()
    d.has_x2 = x2 is not None
    d.bias = bias
    d.aux = d.aux_words = None
    if aux is not None:
        if g['aux_fmt'] == 'split':
            d.aux_words, d.aux = held_split(aux)
        else:
            d.aux_words, d.aux = aux, aux.double()

    d.want, d.pre, d.mag = gemmref.gemm(
        d.x.view(g['images'], g['H'], g['Wd'], cin_all), d.w, d.bias, d.aux, g['epilogue'],
        g['KH'], g['KW'], g['stride'], g['pad'], G,
        d.x2.view(g['images'], g['H2'], g['W2d'], g['C2']) if d.has_x2 else None, g['stride2'],
        g['stride_w'], g['pad_w'])
    if g['out_split']:
        d.want = d.want.clamp(-splitfmt.F16_MAX, splitfmt.F16_MAX)
    return d


# ---- one launch ----------------------------------------------------------------------------------
def launch(d, dev, group=None, **override):
    """C as (GUARD + M + GUARD, ldc) int32 words and the status word.  group=q: group q of a
    grouped case as a plain launch on shifted pointers (shift_group)."""
    g = d.g
    G, N, M = g['groups'], g['N'], g['M']
    split = bool(g['a_split'])
    A = widen(d.x_words, g['a_col'], g['a_pix_stride'], split).to(dev)
    C = torch.full(((GUARD + M + GUARD) * g['ldc'],), SENTINEL, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    q = group or 0
    f = dict(
        A=A.data_ptr() + 4 * (g['a_col'] + q * g['Cin']),
        C=C.data_ptr() + 4 * (GUARD * g['ldc'] + g['c_col'] + q * N),
        weight=d.w.float()[q:q + 1 if group is not None else G].contiguous().to(dev),
        bias=d.bias[q * N:(q + 1) * N if group is not None else G * N].contiguous().to(dev),
        status=status,
        a_pix_stride=g['a_pix_stride'], a_img_stride=g['H'] * g['Wd'] * g['a_pix_stride'],
        M=M, N=N, K=g['K'], ldc=g['ldc'], ldaux=g['ldaux'] if d.aux is not None else 0,
        H=g['H'], Wd=g['Wd'], Cin=g['Cin'], Ho=g['Ho'], Wo=g['Wo'], KH=g['KH'], KW=g['KW'],
        stride=g['stride'], pad=g['pad'], aniso=g['aniso'],
        stride_w=g['stride_w'] if g['aniso'] else 0, pad_w=g['pad_w'] if g['aniso'] else 0,
        epilogue=g['epilogue'], a_split=g['a_split'], out_split=g['out_split'],
        aux_split=g['aux_split'], groups=G if G > 1 and group is None else 0,
        tap_ncls=d.c.get('tap_ncls', 0), no_wt=int(bool(d.c.get('no_wt'))))
    if G > 1:   # (one group of a grouped conv keeps its strides: gemm_plan.h, group_part)
        f.update(a_grp=g['Cin'], bias_grp=N, c_grp=N, aux_grp=N)
    keep = [A, C, status, f['weight'], f['bias']]
    if d.aux is not None:
        aux = widen(d.aux_words, g['aux_col'], g['ldaux'], g['aux_fmt'] == 'split').to(dev)
        f['aux'] = aux.data_ptr() + 4 * (g['aux_col'] + q * N)
        keep.append(aux)
    if d.has_x2:
        A2 = widen(d.x2_words, g['a2_col'], g['a2_pix_stride'], split).to(dev)
        f.update(A2=A2.data_ptr() + 4 * g['a2_col'], K1=g['K1'], H2=g['H2'], W2d=g['W2d'],
                 stride2=g['stride2'], a2_pix_stride=g['a2_pix_stride'],
                 a2_img_stride=g['H2'] * g['W2d'] * g['a2_pix_stride'])
        keep.append(A2)
    if d.m_live is not None:
        f['m_live'] = torch.tensor([d.m_live], dtype=torch.int32, device=dev)
        f['m_live_mul'] = d.m_live_mul
    if d.row_list is not None:
        f['row_list'] = torch.tensor(d.row_list + [0], dtype=torch.int32, device=dev)
    f.update(override)
    f = {k: v for k, v in f.items() if v is not None}
    hip.gemm_probe(device=dev, **f)
    return C.view(GUARD + M + GUARD, g['ldc']).cpu(), int(status.item())


def f32_companion(d, dev):
    """The fp32 general kernel on the same held operands: a Linear over the explicit im2col rows
    of every group, fp32 residual.  (M, groups * N) float64."""
    g = d.g
    G, N, K, M = g['groups'], g['N'], g['K'], g['M']
    rows = gemmref.operand_rows(
        d.x.view(g['images'], g['H'], g['Wd'], -1), g['KH'], g['KW'], g['stride'], g['pad'], G,
        d.x2.view(g['images'], g['H2'], g['W2d'], g['C2']) if d.has_x2 else None, g['stride2'],
        g['stride_w'], g['pad_w'])
    out = []
    for q in range(G):
        A = rows[q].float().contiguous().to(dev)
        C = torch.empty(M, N, device=dev)
        f = dict(A=A, C=C, weight=d.w[q:q + 1].float().contiguous().to(dev),
                 bias=d.bias[q * N:(q + 1) * N].contiguous().to(dev), a_pix_stride=K,
                 a_img_stride=K, M=M, N=N, K=K, ldc=N, H=1, Wd=1, Cin=K, Ho=1, Wo=1, KH=1, KW=1,
                 stride=1, epilogue=g['epilogue'])
        if d.aux is not None:
            f.update(aux=d.aux[:, q * N:(q + 1) * N].float().contiguous().to(dev), ldaux=N)
        hip.gemm_probe(device=dev, **f)
        out.append(C.cpu().double())
    return torch.cat(out, dim=1)


# ---- the checks ----------------------------------------------------------------------------------
def written_slice(d, C):
    g = d.g
    return C[GUARD:GUARD + g['M'], g['c_col']:g['c_col'] + g['groups'] * g['N']]


def values(d, C):
    words = written_slice(d, C).contiguous().view(torch.float32)
    return splitfmt.from_split(words) if d.g['out_split'] else words.double()


def fp32_bound(d):
    """check 1: the elementwise bound of an fp32 form, (M, GN)"""
    g = d.g
    acc = (g['K'] + 8) * 2.0 ** -24 * d.mag
    ulp = 2.0 ** (torch.frexp(d.want)[1].double() - 24)
    if g['epilogue'] == gemmref.EPI_BIAS_TANH:
        return acc + TANH_ULPS * ulp
    if g['epilogue'] == gemmref.EPI_BIAS_SIGMUL:
        return acc * d.aux.abs() / 4 + SIGMUL_ULPS * ulp
    return acc


def check_untouched(d, C):
    """check 3: everything but the live rows' slice is the sentinel, bit for bit"""
    g = d.g
    untouched = torch.ones_like(C, dtype=torch.bool)
    untouched[GUARD + d.live, g['c_col']:g['c_col'] + g['groups'] * g['N']] = False
    stray = (C != SENTINEL) & untouched
    assert not stray.any(), ('written outside the launch (row, word): %s'
                             % stray.nonzero()[:8].tolist())
    live_words = written_slice(d, C)[d.live]
    if not g['out_split']:   # (a live fp32 value may be anything but the sentinel's NaN)
        assert (live_words != SENTINEL).all(), 'live rows not written'


def check_values(d, C, status, dev, report=None):
    g = d.g
    check_untouched(d, C)
    live = d.live
    if len(live) == 0:
        assert status == 0
        return
    got, want = values(d, C)[live], d.want[live]
    keep = torch.ones_like(want, dtype=torch.bool)
    if d.sat is not None:
        r = int((live == d.sat[0]).nonzero())
        keep[r, d.sat[1]] = False
        if d.mode == 'sat-over':
            assert status == SATURATED, status
            assert got[r, d.sat[1]] == splitfmt.F16_MAX, got[r, d.sat[1]]
        else:
            assert status == 0, status
            assert abs(got[r, d.sat[1]] - want[r, d.sat[1]]) <= 2.0 ** -20 * want[r, d.sat[1]]
    else:
        assert status == 0, 'status word %d' % status
    err = ((got - want).abs() * keep)
    assert torch.isfinite(got).all()
    if not g['a_split']:
        excess = err - fp32_bound(d)[live]
        assert (excess <= 0).all(), ('fp32 bound missed by %.3g at %s'
                                     % (excess.max(), (excess > 0).nonzero()[:4].tolist()))
        if report is not None:
            report('%s fp32 max err / bound %.3f' % (d.c['id'], (err / fp32_bound(d)[live]).max()))
        return
    f32 = f32_companion(d, dev)[live]
    assert ((f32 - want).abs() * keep <= fp32_bound(d)[live]).all(), 'the fp32 companion misses 1'
    scale = float((want.abs() * keep).max())
    err_split, err_f32 = float(err.max()), float(((f32 - want).abs() * keep).max())
    if report is not None:
        report('%s err_split %.3g err_f32 %.3g ratio %.2f scale %.3g' % (
            d.c['id'], err_split, err_f32, err_split / max(err_f32, 1e-300), scale))
    assert err_split <= max(4 * err_f32, 2e-6 * scale), (err_split, err_f32, scale)
    assert err_split <= 1e-5 * scale, (err_split, scale)


# ---- the default environment's cases -----------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cus(dev):
    return max(8, torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8)


_RUNS = {}


def run(c, dev, mode='random'):
    """(data, C, status) of a default-environment case, once per module"""
    key = (c['id'], mode, c.get('tap_ncls'), 'rows' in c, 'm_live' in c)
    if key not in _RUNS:
        d = make_data(c, mode)
        _RUNS[key] = (d,) + launch(d, dev)
    return _RUNS[key]


def assert_plan(dump, cus, c):
    p = dump(*gemm_forms.dump_args(c), 'cus=%d' % cus)
    assert p.get('kernel') == c['kernel'], p


DEFAULT = [c for c in CASES if 'env' not in c and 'refused' not in c]
REFUSED = [c for c in CASES if 'refused' in c]
KNOB = [c for c in CASES if 'env' in c]


def ids(cases):
    return [c['id'] for c in cases]


@pytest.mark.parametrize('c', DEFAULT, ids=ids(DEFAULT))
def test_form(dev, dump, cus, c):
    assert_plan(dump, cus, c)
    d, C, status = run(c, dev)
    check_values(d, C, status, dev, report=print)


@pytest.mark.parametrize('c', REFUSED, ids=ids(REFUSED))
def test_refusal(dev, c):
    d = make_data(c)
    with pytest.raises(ValueError, match=re.escape(c['refused'])):
        launch(d, dev)


# 5. saturation: one case per split-output epilogue, and the other tiles that write split rows
SATURATING = ['pp32n128-split-epi-bias', 'pp32n128-split-epi-relu', 'pp32n128-split-epi-res_relu',
              'pp32n128-split-epi-sigmul', 'pp32n128-split-epi-add', 'pp32-k96-slices',
              's64c32-k96-slices', 'tm2-borders', 'tap0-res_relu']


@pytest.mark.parametrize('id', SATURATING)
def test_saturation_is_reported_and_clamped(dev, id):
    for mode in ('sat-over', 'sat-inside'):
        d, C, status = run(by_id(id), dev, mode)
        check_values(d, C, status, dev)


# 7. one case per kernel form with the epilogues that keep integers exact
def one_per_kernel(cases):
    seen = {}
    for c in cases:
        if c.get('epi', 0) in (0, 1, 2, 5) and 'm_live' not in c:
            seen.setdefault(c['kernel'], c)
    return list(seen.values())


PERMUTED = one_per_kernel(DEFAULT)


@pytest.mark.parametrize('c', PERMUTED, ids=ids(PERMUTED))
def test_permutation_weights_are_exact(dev, c):
    """A transposed or shifted fragment shows as wrong VALUES, not as noise (MI355X guide rule 16:
    asymmetric operands)."""
    d, C, status = run(c, dev, 'perm')
    check_untouched(d, C)
    assert status == 0
    assert torch.equal(values(d, C)[d.live], d.want[d.live])


# 6. the promised bit-equalities
def variant(c, drop=(), **fields):
    """the same case (same id = same data) without the fields `drop`, with `fields`"""
    return dict({k: x for k, x in c.items() if k not in drop}, **fields)


LISTS = [c for c in DEFAULT if 'rows' in c]
LIVE = [c for c in DEFAULT if 'm_live' in c]
GROUPED = [c for c in DEFAULT if c.get('groups', 1) > 1]
TAPS = [c for c in DEFAULT if c['kernel'] in (gemm_forms.PP32T % 128, gemm_forms.PP32T % 256,
                                              gemm_forms.GPP32T) and 'tap_ncls' not in c]


@pytest.mark.parametrize('c', LISTS, ids=ids(LISTS))
def test_listed_rows_equal_the_dense_launch(dev, c):
    d, C, _ = run(c, dev)
    _, dense, _ = run(variant(c, drop=('rows',)), dev)
    assert torch.equal(written_slice(d, C)[d.live], written_slice(d, dense)[d.live])


@pytest.mark.parametrize('c', LIVE, ids=ids(LIVE))
def test_live_rows_equal_the_full_launch(dev, c):
    d, C, _ = run(c, dev)
    _, full, _ = run(variant(c, drop=('m_live',)), dev)
    assert torch.equal(written_slice(d, C)[d.live], written_slice(d, full)[d.live])


@pytest.mark.parametrize('c', GROUPED, ids=ids(GROUPED))
def test_grouped_launch_equals_its_groups(dev, c):
    """one grouped launch = `groups` plain launches on shift_group's pointers; a group's
    launch leaves the neighbours' columns alone"""
    d, C, _ = run(c, dev)
    n = d.g['N']
    for q in range(d.g['groups']):
        part, status = launch(d, dev, group=q)
        assert status == 0
        cols = slice(q * n, (q + 1) * n)
        assert torch.equal(written_slice(d, part)[:, cols], written_slice(d, C)[:, cols])
        others = written_slice(d, part).clone()
        others[:, cols] = SENTINEL
        assert (others == SENTINEL).all() and (part[:GUARD] == SENTINEL).all()


@pytest.mark.parametrize('c', TAPS, ids=ids(TAPS))
def test_class_tiles_equal_the_linear_order(dev, c):
    d, C, _ = run(c, dev)
    _, linear, status = run(variant(c, tap_ncls=-1), dev)
    assert status == 0 and torch.equal(C, linear)


# ---- the forms behind a knob: one fresh process per setting -----------------------------------
SETTINGS = sorted({tuple(sorted(c['env'].items())) for c in KNOB})


def child(out_path, case_ids):
    dev = torch.device('cuda:0')
    out = {}
    for key in case_ids:     # 'id' or 'id:mode'
        id, _, mode = key.partition(':')
        out[key] = launch(make_data(by_id(id), mode or 'random'), dev)
    torch.save(out, out_path)


@pytest.mark.parametrize('setting', SETTINGS, ids=['-'.join('%s=%d' % kv for kv in s)
                                                   for s in SETTINGS])
def test_knob_forms(dev, dump, cus, tmp_path, setting):
    cases = [c for c in KNOB if tuple(sorted(c['env'].items())) == setting]
    for c in cases:
        assert_plan(dump, cus, c)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', **{k: str(v) for k, v in setting})
    out_path = tmp_path / 'knob.pt'
    hip.release_workspaces()
    permuted = one_per_kernel(cases)   # 7. on the knob forms too
    subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), str(out_path)] +
                   ids(cases) + [c['id'] + ':perm' for c in permuted], env=env, check=True,
                   timeout=300)
    got = torch.load(out_path)
    for c in permuted:
        C, status = got[c['id'] + ':perm']
        d = make_data(c, 'perm')
        check_untouched(d, C)
        assert status == 0
        assert torch.equal(values(d, C)[d.live], d.want[d.live]), c['id']
    for c in cases:
        C, status = got[c['id']]
        d = make_data(c)
        check_values(d, C, status, dev, report=print)
        if c['id'] in SAME_BITS:
            twin = by_id(SAME_BITS[c['id']])
            assert_plan(dump, cus, twin)
            # (the twin has the knob case's shape; its data follow the knob case's id)
            tC, tstatus = launch(make_data(dict(twin, id=c['id'])), dev)
            assert tstatus == 0 and torch.equal(C, tC), c['id']


if __name__ == '__main__':
    child(sys.argv[1], sys.argv[2:])
