"""The schedule tools/enc_plan_dump.cpp prints is the pass that runs (csrc/enc_plan.h).

The dump is plain host C++ over the same plan_encoder() the library walks; here one
Context.encode per case runs with the profiler on, and milan_profile_read_kernels has to count
the launches per kernel family that the dump names for the same trunk, images, masks, precision
and fusion bits.  The width-16 trunks have no split weight copies (Cin % 32 != 0): their passes
are fp32 in either precision; only the width-64 trunk reaches the chains, the 3x3 front and the
row-list tiles, which is why it is here, on 96 x 96 images.
"""
import pathlib
import shutil
import subprocess

import pytest
import torch

from milan_amd import hip, synthetic

pytestmark = pytest.mark.gpu
REPO = pathlib.Path(__file__).resolve().parent.parent
PREFIX = 'encoder.encoder.model.'
N, SIZE = 5, 96


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    cxx = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = tmp_path_factory.mktemp('enc_plan') / 'enc_plan_dump'
    subprocess.run([cxx, '-std=c++17', '-O1', str(REPO / 'tools' / 'enc_plan_dump.cpp'), '-o',
                    str(exe)], check=True)

    def families(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True)
        line = next(l for l in out.stdout.splitlines() if l.startswith('families'))
        return {f.split(':')[0]: int(f.split(':')[1]) for f in line.split()[1:] if ':' in f}
    return families


@pytest.fixture(scope='module')
def contexts():
    hip.load_library()
    dev = hip.require_device('cuda')
    made = {}

    def get(arch, width):
        if (arch, width) not in made:
            sd = synthetic.resnet_state_dict(arch, seed=3, width=width, prefix=PREFIX)
            made[arch, width] = hip.Context(
                hip.make_dims(sd, 10, blocks=synthetic.RESNET_BLOCKS[arch]), sd, dev)
        return made[arch, width]

    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope='module')
def batch():
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (N, 3, SIZE, SIZE), dtype=torch.uint8, generator=g)
    masks = torch.zeros(N, 1, SIZE, SIZE, dtype=torch.uint8)
    for i in range(1, N):   # (image 0 has an empty mask: it skips the trunk)
        masks[i, 0, 10 * i:10 * i + 30, 5 * i:5 * i + 40] = 1
    return images, masks


@pytest.mark.parametrize('precision', ['split_f16', 'f32'])
@pytest.mark.parametrize('arch,width,tail_lists', [
    ('resnet50', 64, True), ('resnet50', 64, False), ('resnet50', 16, True), ('resnet18', 16, True)])
def test_the_pass_launches_what_the_dump_names(dump, contexts, batch, arch, width, tail_lists,
                                               precision):
    ctx = contexts(arch, width)
    ctx.set_precision(precision)
    ctx.set_fusion(tail_lists=tail_lists)
    hip.profile_enable(True)
    try:
        ctx.encode(*batch)
        counted = hip.profile_read_kernels()
    finally:
        hip.profile_enable(False)
        ctx.set_fusion()
    assert ctx.status() == 0
    ran = {name: int(row['launches']) for name, row in counted.items() if row['launches']}
    named = dump(arch, width, N, SIZE, SIZE, 'split' if precision == 'split_f16' else 'f32',
                 'tail_lists=%d' % tail_lists)
    print(arch, width, precision, 'lists' if tail_lists else 'copies', 'ran', ran, 'dump', named)
    assert ran == named
    assert set(ran) <= set(hip.KERNEL_FAMILIES)
