"""The plan that tools/gemm_plan_dump.cpp prints is the launch that runs: for six
small convs the kernel family that milan_profile_read_kernels counts is the family the host
program names for the same arguments, with as many launches as it says."""
import pytest
import torch

import test_gemm_plan_host as H
from milan_amd import hip

pytestmark = pytest.mark.gpu
dump = H.dump

# (name, cout, cin, k, precision, options of the dump beyond the geometry).  hip.conv2d_nhwc
# writes fp32 (out_split=0) and, in split mode, makes the tap-inner weight copy of a k x k conv.
CONVS = [
    ('f32', 64, 64, 1, 'f32', ()),
    ('N 64 3x3', 64, 64, 3, 'split_f16', ('out_split=0', 'Wt=1')),
    ('N 128', 128, 64, 1, 'split_f16', ('out_split=0',)),
    ('N 256 1x1', 256, 64, 1, 'split_f16', ('out_split=0',)),
    ('N 256 3x3', 256, 64, 3, 'split_f16', ('out_split=0', 'Wt=1')),
]


def launches_by_family(run):
    hip.profile_enable(True)
    try:
        run()
        table = hip.profile_read_kernels()
    finally:
        hip.profile_enable(False)
    return {name: int(row['launches']) for name, row in table.items() if row['launches']}


@pytest.mark.parametrize('name,cout,cin,k,precision,opts', CONVS, ids=[c[0] for c in CONVS])
def test_conv_runs_in_the_family_the_plan_names(dump, name, cout, cin, k, precision, opts):
    dev = hip.require_device('cuda')
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 14, 14, cin, generator=g).to(dev)
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k)**0.5).to(dev)
    plan = dump(*H.conv(cout, cin, k, 'f32' if precision == 'f32' else 'split', *opts))
    assert plan['launches'] == 'one', plan
    got = launches_by_family(lambda: hip.conv2d_nhwc(x, w, None, 1, k // 2, precision=precision))
    assert got == {plan['family']: 1}, (plan, got)


def test_grouped_conv_runs_as_the_plan_says(dump):
    """conv1 and the two-group 5 x 5 conv2 of the Places365 AlexNet at width 8, fp32: the plan
    names the grouped form of the general kernel, one launch each."""
    import test_gpu_places as P
    images = P.pictures((67, 75), 1)
    # conv1: 3 (padded to 4) -> 24 channels, 11 x 11 / 4 on 67 x 75; pool1 leaves 7 x 8;
    # conv2: 2 groups of 12 -> 32 channels, 5 x 5 / pad 2
    conv1 = dump(24, 4, 11, 11, 4, 0, 67, 75, 1, 'f32')
    conv2 = dump(32, 12, 5, 5, 1, 2, 7, 8, 1, 'f32', 'groups=2')
    assert conv2['kernel'] == 'igemm_kernel<256, 64, 2, false, false, true>', conv2
    assert conv2['grid'].endswith(',2') and conv2['launches'] == 'one', conv2
    assert conv1['family'] == conv2['family'] == 'f32'
    ctx = P.make_context(P.model_sd(8), head=False)
    try:
        ctx.set_precision('f32')
        got = launches_by_family(lambda: ctx.activations(images, [1]))
    finally:
        ctx.close()
    assert got == {'f32': 2}, got
