"""Generate the Places365 goldens from the reference's own code.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_places.py

Imports the reference's `src.deps.alexnet` and `src.deps.resnet152` unmodified (with the
stubs make_golden.py uses for the absent third-party packages) and runs, in `.eval()`:

  - its own `AlexNet()` at full width (96 / 256 / 384 / 384 / 256 channels, 4096 hidden, 365
    classes), with and without `include_lrn`, on 2 seeded 227 x 227 images.  The weights are
    tests/placesref.py's seeded ones, pushed in with `load_state_dict`;
  - its `OldResNet152()` on 2 seeded 224 x 224 images, with seeded torchvision-shaped weights
    (`synthetic.resnet_state_dict` plus a seeded `fc`) pushed in under the old key names.

Stored are results only: the logits, and in the .json the child names and state-dict keys of
`AlexNet` for every flag combination and the (key, shape) list of `OldResNet152().state_dict()`.

Outputs: reference_goldens_places.pt / .json (data only).
"""
import itertools
import json
import pathlib
import sys

import torch

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'neuron-descriptions_amd'))
sys.path.insert(0, str(ROOT / 'tests'))
sys.path.insert(0, str(HERE))

import make_golden  # noqa: E402
import placesref  # noqa: E402
from milan_amd import classifiers, synthetic  # noqa: E402

ALEX = dict(seed=61, width=32, hidden=4096, classes=365, n_images=2, geometry=[227, 227])
RESNET = dict(seed=67, width=64, classes=365, n_images=2, geometry=[224, 224])


def compact(obj, level=0):
    """json text with a dict's entries one per line and every list on one line."""
    if isinstance(obj, dict):
        pad = ' ' * (level + 1)
        body = ',\n'.join(f'{pad}{json.dumps(k)}: {compact(v, level + 1)}' for k, v in obj.items())
        return '{\n' + body + '\n' + ' ' * level + '}'
    return json.dumps(obj)


def main():
    torch.set_num_threads(8)
    make_golden.import_reference()
    from src.deps import alexnet, resnet152
    out, meta = {}, dict(alexnet=dict(ALEX), resnet152=dict(RESNET))

    # -- AlexNet: names for every flag combination, logits with and without the LRN
    meta['alexnet']['variants'] = {}
    for lrn, groups, dropout in itertools.product((False, True), repeat=3):
        model = alexnet.AlexNet(include_lrn=lrn, split_groups=groups, include_dropout=dropout)
        meta['alexnet']['variants'][f'lrn={int(lrn)},groups={int(groups)},dropout={int(dropout)}'] = dict(
            modules=[name for name, _ in model.named_children()],
            state_dict=[[k, list(v.shape)] for k, v in model.state_dict().items()])
    sd = placesref.make_state_dict(ALEX['seed'], ALEX['width'], ALEX['hidden'], ALEX['classes'])
    x = placesref.make_images(ALEX['seed'], ALEX['n_images'], tuple(ALEX['geometry']))
    for lrn in (False, True):
        model = alexnet.AlexNet(include_lrn=lrn)
        model.load_state_dict(sd, strict=True)
        model.eval()
        with torch.no_grad():
            out[f'alexnet.lrn{int(lrn)}.logits'] = model(x).clone()

    # -- OldResNet152: key list, logits under seeded weights in the old key names
    model = resnet152.OldResNet152()
    old = model.state_dict()
    meta['resnet152']['state_dict'] = [[k, list(v.shape)] for k, v in old.items()]
    new_names = list(classifiers.rekey_old_resnet152(old).keys())
    tv = placesref.make_resnet152_state_dict(RESNET['seed'], RESNET['width'], RESNET['classes'])
    pushed = {}
    for key, name in zip(old.keys(), new_names):
        pushed[key] = old[key] if name.endswith('num_batches_tracked') else tv[name]
        assert pushed[key].shape == old[key].shape, (key, name)
    model.load_state_dict(pushed, strict=True)
    model.eval()
    x = placesref.make_images(RESNET['seed'], RESNET['n_images'], tuple(RESNET['geometry']))
    with torch.no_grad():
        out['resnet152.logits'] = model(x).clone()

    torch.save(out, HERE / 'reference_goldens_places.pt')
    (HERE / 'reference_goldens_places.json').write_text(compact(meta) + '\n')
    for k, v in out.items():
        print(k, tuple(v.shape), float(v.abs().max()))


if __name__ == '__main__':
    main()
