"""Host side of the wide beam search: the new entry points are declared where the
C-ABI test looks for them, old builds of the library stay loadable, and
DecoderWithCLIP keeps the reference's default beam (no GPU)."""
import pathlib
import re

import pytest
import torch

from milan_amd import decoders, hip

REPO = pathlib.Path(__file__).resolve().parent.parent
NEW = ('milan_beam_merge', 'milan_set_beam_path', 'milan_get_beam_path')


def test_new_entry_points_are_declared_exported_and_probed():
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    lib = hip.load_library()
    for name in NEW:
        assert name in hip.SIGNATURES
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert hasattr(lib, name), name
        # added without a new ABI version: a library built before them still loads
        assert name in hip.PROBED
    assert len(hip.SIGNATURES['milan_beam_merge'][1]) == 13
    assert hip.ABI_VERSION == 11 == lib.milan_abi_version()
    assert lib.milan_get_beam_path(None) == -1


def test_beam_path_setter_rejects_a_null_context():
    lib = hip.load_library()
    assert lib.milan_set_beam_path(None, 1) != 0  # null context
    assert b'null ctx' in lib.milan_last_error()


def test_beam_merge_has_no_cpu_fallback():
    cand = torch.zeros(1, 1, 4)
    with pytest.raises(hip.HipUnavailableError):
        hip.beam_merge(cand, cand.int())


def test_decoder_with_clip_keeps_the_reference_default_beam():
    import json
    from milan_amd import encoders, lang, synthetic
    golden = REPO / 'tests' / 'golden'
    meta = json.loads((golden / 'reference_goldens_clip.json').read_text())
    weights = torch.load(golden / 'reference_goldens_clip.pt', weights_only=True)['weights/odd']
    dims = meta['configs']['odd']
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(12)), None, True, True, True, True, 15)
    enc = encoders.PyramidConvEncoder('resnet50', width=8, pretrained=False)
    model = decoders.DecoderWithCLIP(
        idx, enc, embedding_size=4, hidden_size=8,
        reranker_kwargs=dict(weights=weights, vision_heads=dims['vision_heads'],
                             text_heads=dims['text_heads']))
    assert model.beam_size == 1000 and model.properties()['beam_size'] == 1000
