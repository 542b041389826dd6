"""The coverage ledger of tests/gemm_forms.py (CPU): every product kernel form of
MILAN_GEMM_KERNELS (csrc/gemm_plan.h) is the planned kernel of at least one case of the table or
is listed in EXEMPT with its reason, and every case's plan names the kernel (or the refusal) the
case was written for.  A new line in MILAN_GEMM_KERNELS fails here until it has a case.

tools/gemm_plan_dump.cpp answers both questions on the host: no GPU, no HIP call.
"""
import pytest

import gemm_forms
from gemm_forms import CASES, EXEMPT, EXEMPT_EPILOGUES
from test_gemm_plan_host import dump  # noqa: F401  (the module-scoped fixture)


def plan(dump, c):
    return dump(*gemm_forms.dump_args(c))


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_case_runs_the_kernel_it_names(dump, c):
    p = plan(dump, c)
    if 'refused' in c and c.get('refused_by') != 'launcher':
        assert p.get('msg') == c['refused'] and p.get('err') == '-2', p
        return
    assert 'err' not in p, p
    if 'refused' not in c:
        assert p['kernel'] == c['kernel'], p
        assert p['launches'] == 'one', p
        want_mode = 'split8' if c.get('out', c['prec']) == 'split' else \
            ('scalar' if c.get('ldc', 0) % 4 else 'vec4')
        assert p['out_mode'] == want_mode, p


def product_kernels(dump):
    return list(dump('kernels').values())


def test_every_product_kernel_has_a_case_or_a_reason(dump):
    kernels = product_kernels(dump)
    assert len(kernels) == len(set(kernels)) > 0, kernels
    planned = {plan(dump, c).get('kernel') for c in CASES if 'refused' not in c}
    assert not set(EXEMPT) & planned, 'an exempt kernel has a case: drop the exemption'
    assert set(EXEMPT) <= set(kernels), 'an exemption names no product kernel'
    for reason in list(EXEMPT.values()) + list(EXEMPT_EPILOGUES.values()):
        assert reason.strip()
    uncovered = [k for k in kernels if k not in planned and k not in EXEMPT]
    assert not uncovered, 'product kernels without a case in tests/gemm_forms.py: %s' % uncovered
    assert set(kernels) == (planned - {None}) | set(EXEMPT), sorted(planned - set(kernels) - {None})


def test_every_accepted_epilogue_form_has_a_case(dump):
    """epilogue x output format: each pair the plan accepts for one plain N = 128 layer has a
    case; each pair it refuses is a refusal case with the plan's text; LSTM and LSE are exempt."""
    have = {(c.get('epi', 0), c.get('out', c['prec'])) for c in CASES
            if c['prec'] == 'split' and 'refused' not in c}
    have_f32 = {(c.get('epi', 0), 'scalar' if c.get('ldc', 0) % 4 else 'vec4') for c in CASES
                if c['prec'] == 'f32' and 'refused' not in c}
    refused = {(c.get('epi', 0), c.get('out', c['prec'])) for c in CASES if 'refused' in c}
    for e, name in enumerate(gemm_forms.EPI):
        for out in ('split', 'f32'):
            p = dump(128, 32, 1, 1, 1, 0, 1, 1, 64, 'split', 'out_split=%d' % (out == 'split'),
                     'epilogue=' + name)
            if 'err' in p:
                assert (e, out) in refused, (name, out, p)
            else:
                assert (e, out) in have, (name, out)
        for mode in ('vec4', 'scalar'):
            assert (e, mode) in have_f32, (name, mode)
    assert set(EXEMPT_EPILOGUES) == {'lstm', 'lse'}
