"""Golden G18: netdissect's `RunningTopK` loading the tally state this repo WRITES.

Run in the build container only (needs the reference, like make_golden.py):

    python tests/golden/make_golden_topk_state.py

For each case of tests/test_exemplar_state.py the same seeded `milan_amd.exemplars.
RunningTopK` is built, its `state_dict()` goes through an .npz file as the tally cache
does, and the reference's own class (src/deps/netdissect/runningstats.py:118-149) loads
it; its `result()` and `size()` are stored.  The test then needs no reference.
"""
import json
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO / 'neuron-descriptions_amd'))

import numpy  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402
from milan_amd import exemplars  # noqa: E402

# (units, k, filled) of test_topk_state_dict_is_netdissect_format
CASES = [(7, 5, 5), (4, 4, 4), (6, 15, 9), (1, 3, 2)]


def case_name(units, k, filled):
    return f'u{units}_k{k}_f{filled}'


def filled_topk(units, k, filled, count, seed=0):
    """The state the test builds (tests/test_exemplar_state.py::_filled_topk)."""
    g = torch.Generator().manual_seed(seed)
    top = exemplars.RunningTopK(k=k)
    values, order = torch.rand(units, k, generator=g).sort(dim=1, descending=True)
    top.values = values
    top.index = torch.randint(0, count, (units, k), generator=g)
    top.values[:, filled:] = 0
    top.filled, top.count = filled, count
    return top


def main(tmp=HERE / '_topk_state.npz'):
    for n in ('statsmodels', 'statsmodels.stats',
              'statsmodels.stats.correlation_tools'):
        make_golden._stub(n, cov_nearest=None, corr_nearest=None)
    make_golden.import_reference()
    from src.deps.netdissect import runningstats
    out, meta = {}, {}
    try:
        for units, k, filled in CASES:
            top = filled_topk(units, k, filled, count=1000 + units)
            state = top.state_dict()
            numpy.savez(tmp, **{k_: v for k_, v in state.items() if v is not None})
            loaded = dict(numpy.load(tmp, allow_pickle=True))
            ref = runningstats.RunningTopK(state=loaded)
            values, index = ref.result()
            name = case_name(units, k, filled)
            out[f'{name}_values'] = values.clone()
            out[f'{name}_index'] = index.clone()
            meta[name] = dict(units=units, k=k, filled=filled, size=int(ref.size()))
    finally:
        tmp.unlink(missing_ok=True)
    torch.save(out, HERE / 'reference_goldens_topk_state.pt')
    with open(HERE / 'reference_goldens_topk_state.json', 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'tensors')


if __name__ == '__main__':
    main()
