"""CPU-only tests of image sharing's host side: the three C entry points, the Python
plumbing from `Decoder` down to the context, and the script's flag."""
import ctypes
import importlib.util
import pathlib
import re

import torch

from milan_amd import decoders, hip
from test_host import tiny_decoder

REPO = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = ('milan_set_image_sharing', 'milan_get_image_sharing', 'milan_image_sharing_stats')


def test_symbols_are_in_header_export_map_and_ctypes_table():
    header = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'milan_hip.h').read_text(), flags=re.S)
    lib = hip.load_library()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in hip.SIGNATURES
        assert hasattr(lib, name)   # (exports.map: global milan_*)
    assert 'milan_*' in (REPO / 'neuron-descriptions_amd' / 'csrc' / 'exports.map').read_text()
    # probed for, not versioned
    assert 'hasattr(lib, "milan_set_image_sharing")' in (REPO / 'include' / 'milan_hip.h').read_text()


def test_null_context_is_an_argument_error():
    lib = hip.load_library()
    assert lib.milan_set_image_sharing(None, 1) == hip.ERR_ARG
    assert lib.milan_get_image_sharing(None) == -1
    a, b = ctypes.c_longlong(7), ctypes.c_longlong(7)
    assert lib.milan_image_sharing_stats(None, ctypes.byref(a), ctypes.byref(b), 0,
                                         None) == hip.ERR_ARG
    assert (a.value, b.value) == (7, 7)
    assert lib.milan_workspace_bytes(None, 1, 1, 224, 1, 1) == 0


class StubContext:
    """what Decoder._apply_share_images needs of a hip.Context"""

    def __init__(self):
        self.image_sharing = False
        self.calls = []

    def set_image_sharing(self, enable):
        self.calls.append(enable)
        self.image_sharing = bool(enable)


def test_decoder_attribute_reaches_the_context(monkeypatch):
    monkeypatch.delenv('MILAN_SHARE_IMAGES', raising=False)
    dec = tiny_decoder()
    assert dec.share_images is False
    assert 'share_images' not in dec.properties()
    stub = StubContext()
    dec._apply_share_images(stub)
    assert stub.calls == [] and stub.image_sharing is False
    dec.share_images = True
    dec._apply_share_images(stub)
    dec._apply_share_images(stub)
    assert stub.calls == [True] and stub.image_sharing is True
    dec.share_images = False
    dec._apply_share_images(stub)
    assert stub.calls == [True, False]
    # MILAN_SHARE_IMAGES=1 (read by the context at creation) is not switched off by the default
    monkeypatch.setenv('MILAN_SHARE_IMAGES', '1')
    stub.image_sharing = True
    dec._apply_share_images(stub)
    assert stub.calls == [True, False] and stub.image_sharing is True
    on = decoders.Decoder(dec.indexer, dec.encoder, None, embedding_size=4, hidden_size=8,
                          share_images=True)
    assert on.share_images is True


def test_predict_overrides_the_attribute_for_the_call(monkeypatch):
    dec = tiny_decoder()
    seen = []

    def forward(images, masks=None, **kwargs):
        assert 'share_images' not in kwargs
        seen.append((dec.share_images, kwargs.get('strategy')))
        return decoders.DecoderOutput(('a',) * len(images), None, None, None, None, None, None,
                                      None)

    monkeypatch.setattr(dec, 'forward', forward)
    samples = [(0, 0, torch.zeros(2, 3, 8, 8, dtype=torch.uint8),
                torch.ones(2, 1, 8, 8, dtype=torch.uint8)) for _ in range(3)]
    kw = dict(batch_size=2, display_progress_as=None, strategy='greedy')
    assert dec.predict(samples, **kw) == ('a',) * 3
    assert dec.predict(samples, share_images=True, **kw) == ('a',) * 3
    assert dec.share_images is False
    dec.share_images = True
    dec.predict(samples, share_images=False, **kw)
    dec.predict(samples, **kw)
    assert dec.share_images is True
    assert seen == [(False, 'greedy'), (True, 'greedy'), (False, 'greedy'), (True, 'greedy')]


def test_script_flag_parses():
    path = REPO / 'neuron-descriptions_amd' / 'scripts' / 'compute_milan_descriptions.py'
    spec = importlib.util.spec_from_file_location('compute_milan_descriptions_share', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    assert module.parse_args(['alexnet', 'imagenet']).share_images is False
    assert module.parse_args(['alexnet', 'imagenet', '--share-images']).share_images is True
