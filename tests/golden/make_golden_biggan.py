"""Generate the BigGAN goldens from the reference's own code, on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_biggan.py

Imports the reference's `src.deps.ext.pretorched.gans.biggan` unmodified (with the stubs
make_golden.py uses for the absent third-party packages), builds its `Generator` at two tiny
configurations and wraps it with its own `SeqGPreprocess` / `SeqGBlock` / `SeqGOutput`, in the
order its `SeqBigGAN` does (that function itself goes through `BigGAN(pretrained=...)`, which
is not called here: nothing is fetched).

    c32: resolution 32, G_ch 8, attention at 16 (C = 32), hier, SN, BN_eps 1e-4, dim_z 32,
         shared_dim 16, 10 classes
    c64: resolution 64, G_ch 2, attention at 32 (C = 8), not hierarchical, SN, BN_eps 1e-5,
         dim_z 20, shared_dim 12, 7 classes.  (A 64 x 64 generator wide enough for
         milan_sagan_attention, G_ch 8, has 1.9 MB of weights.  This one pins the architecture
         table, the non-hierarchical path, the eager modules and the refusal of the native
         walk; tests/test_gpu_biggan.py runs the native walk at resolution 64 against
         bigganref alone.)

The weights are tests/bigganref.py's seeded ones (nothing left at its init value) rounded to
float16 values, so that they can be stored in two bytes each, loaded into the reference's
module with strict=True.  Stored per configuration: the state dict (float16, exact), z, hard
and soft y for two samples, the child names, every `layerN` / `attnN` output of sample 0 with
hard y, the images of both samples for both kinds of y, and the eval-mode spectrally
normalised weight of three layers (float32).

Output: reference_goldens_biggan.npz (data only).
"""
import collections
import pathlib
import sys

import numpy
import torch
from torch import nn

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'neuron-descriptions_amd'))
sys.path.insert(0, str(ROOT / 'tests'))
sys.path.insert(0, str(HERE))

import make_golden  # noqa: E402
import bigganref  # noqa: E402

CONFIGS = collections.OrderedDict(
    c32=dict(dims=bigganref.make_dims(32, 8, 16, 32, 16, 10, hier=True, bn_eps=1e-4), seed=71),
    c64=dict(dims=bigganref.make_dims(64, 2, 32, 20, 12, 7, hier=False, bn_eps=1e-5), seed=72),
)
N = 2
SN_LAYERS = ('linear', 'blocks.1.0.conv1', 'blocks.0.0.bn1.gain')


def main():
    make_golden.import_reference()
    from src.deps.ext.pretorched.gans import biggan as ext
    from src.deps.pretorched.gans import biggan

    out = {}
    for name, config in CONFIGS.items():
        d = config['dims']
        generator = biggan.Generator(
            G_ch=d['ch'], dim_z=d['dim_z'], bottom_width=d['bottom_width'],
            resolution=d['resolution'], G_attn=str(d['attn']), n_classes=d['n_classes'],
            shared_dim=d['shared_dim'], hier=d['hier'], BN_eps=d['bn_eps'], G_param='SN',
            skip_init=True, no_optim=True)
        sd = bigganref.cast(bigganref.cast(bigganref.weights(d, config['seed']), torch.float16),
                            torch.float32)
        generator.load_state_dict(sd, strict=True)
        generator.eval()
        modules = [('preprocess', ext.SeqGPreprocess(generator))]
        for index, blocks in enumerate(generator.blocks):
            for block in blocks:
                key = 'layer' if isinstance(block, biggan.GBlock) else 'attn'
                modules.append((key + str(index), ext.SeqGBlock(block, index)))
        modules.append(('output', ext.SeqGOutput(generator)))
        seq = nn.Sequential(collections.OrderedDict(modules))

        z, hard, soft = bigganref.latents(d, N, config['seed'] + 100)
        z, soft = z.float(), soft.float()
        out[f'{name}/children'] = numpy.array([k for k, _ in modules])
        out[f'{name}/z'], out[f'{name}/y_hard'], out[f'{name}/y_soft'] = (
            z.numpy(), hard.numpy(), soft.numpy())
        for key, value in sd.items():
            out[f'{name}/sd/{key}'] = value.numpy().astype(numpy.float16)
            assert (out[f'{name}/sd/{key}'].astype(numpy.float32) == value.numpy()).all()
        with torch.no_grad():
            for kind, y in (('hard', hard), ('soft', soft)):
                data = ext.GInputs(z, y)
                for key, child in seq.named_children():
                    data = child(data)
                    if key not in ('preprocess', 'output') and kind == 'hard':
                        out[f'{name}/{kind}/{key}'] = data.h[:1].numpy().copy()
                out[f'{name}/{kind}/images'] = data.numpy().copy()
                # the un-wrapped generator agrees with its sequential form
                direct = generator(z, y, embed=True)
                assert torch.equal(direct, data)
            for layer in SN_LAYERS:
                out[f'{name}/sn/{layer}'] = generator.get_submodule(layer).W_().numpy().copy()
    path = HERE / 'reference_goldens_biggan.npz'
    numpy.savez_compressed(path, **out)
    print(f'wrote {path}: {path.stat().st_size} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
