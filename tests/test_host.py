"""CPU-only tests of the host side: C-ABI surface, caption reconstruction,
checkpoint format, the Python mirror's error behaviour, sharding (gloo)."""
import ctypes
import os
import pathlib
import re
import subprocess
import sys

import numpy
import pytest
import torch
import torch.multiprocessing as mp

from milan_amd import (datasets, decoders, encoders, hip, lang, lms, loaders,
                       serialize, sharding, synthetic)

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'milan_hip.h'


# ---- C ABI -----------------------------------------------------------------
def header_symbols():
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(milan_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_header_symbol():
    """The .so loads (no GPU needed) and exports exactly what the header
    declares; the ctypes table covers all of it."""
    syms = header_symbols()
    assert 'milan_describe' in syms and 'milan_decode' in syms
    lib = hip.load_library()
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in milan_hip.h but not exported'
    assert sorted(hip.SIGNATURES) == syms
    header_version = int(re.search(r'#define MILAN_ABI_VERSION (\d+)',
                                   HEADER.read_text()).group(1))
    assert lib.milan_abi_version() == header_version == hip.ABI_VERSION
    out = subprocess.run(['nm', '-D', '--defined-only', str(hip.LIB_PATH)],
                         capture_output=True, text=True, check=True).stdout
    exported = sorted(
        set(re.findall(r' T (milan_[a-z0-9_]+)$', out, flags=re.M)))
    assert exported == syms, 'undocumented or missing C-ABI exports'
    # -fvisibility=hidden: no C++ internals (launchers, StageScope, ...) in the
    # dynamic symbol table -- every defined function symbol is a C entry point
    functions = re.findall(r' [TW] (\S+)$', out, flags=re.M)
    stray = sorted(f for f in functions if f not in syms
                   and f not in ('_init', '_fini'))
    assert not stray, f'internal symbols exported: {stray[:5]}'


def test_dims_struct_matches_header_layout():
    text = HEADER.read_text()
    body = text[text.index('typedef struct milan_dims {'):text.
                index('} milan_dims;')]
    fields = re.findall(r'int32_t\s+([a-z_]+)(\[4\])?;', body)
    assert [f for f, _ in fields] == [n for n, _ in hip.Dims._fields_]
    assert ctypes.sizeof(hip.Dims) == 4 * (len(fields) + 3)


def test_missing_library_is_loud(tmp_path):
    with pytest.raises(hip.HipUnavailableError, match='no CPU fallback'):
        hip.load_library(tmp_path / 'libmilan_hip.so')


def test_argument_errors_need_no_gpu():
    lib = hip.load_library()
    assert lib.milan_create(None, 0, None) == hip.ERR_ARG
    assert b'null argument' in lib.milan_last_error()
    d = hip.Dims()
    h = ctypes.c_void_p()
    assert lib.milan_create(ctypes.byref(h), 0, ctypes.byref(d)) == hip.ERR_SHAPE
    assert lib.milan_workspace_bytes(None, 1, 1, 224, 1, 1) == 0


# ---- no silent CPU path --------------------------------------------------------
def tiny_decoder(lm=True, encoder=None):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(12)), None, True,
                       True, True, True, 15)
    enc = encoder or encoders.PyramidConvEncoder(
        'resnet50', width=8, pretrained=False)
    model = lms.LanguageModel(idx, 4, 8) if lm else None
    return decoders.Decoder(idx, enc, model, embedding_size=4, hidden_size=8)


@pytest.mark.skipif(torch.cuda.is_available(), reason='CPU-only behaviour')
def test_product_path_fails_loudly_without_gpu():
    d = tiny_decoder()
    feats = torch.rand(2, 3, d.feature_size)
    with pytest.raises(hip.HipUnavailableError, match='no CPU fallback'):
        d(feats, strategy='greedy')
    with pytest.raises(hip.HipUnavailableError):
        d.init_state(feats)
    with pytest.raises(hip.HipUnavailableError):
        d.encoder(torch.rand(1, 3, 64, 64))
    with pytest.raises(hip.HipUnavailableError):
        d.lm(torch.zeros(1, 4, dtype=torch.long), reduce=True)


def test_product_never_imports_the_oracle():
    pkg = REPO / 'neuron-descriptions_amd'
    for path in list(pkg.rglob('*.py')) + list(pkg.rglob('*.hip')) + list(
            pkg.rglob('*.h')):
        text = path.read_text()
        assert 'milan_oracle' not in text and 'import oracle' not in text \
            and 'from oracle' not in text, path


# ---- reference error conventions (decoders.py:395-409, encoders.py:265) ------
def test_forward_validation_matches_reference():
    d = tiny_decoder(lm=False)
    feats = torch.rand(2, 3, d.feature_size)
    with pytest.raises(ValueError, match='without an LM'):
        d(feats, strategy='rerank')
    with pytest.raises(ValueError, match='without an LM'):
        d(feats, strategy='greedy', mi=True)
    with pytest.raises(ValueError, match='unknown strategy: nope'):
        d(feats, strategy='nope')
    with pytest.raises(ValueError, match='strategy must be 2D'):
        d(feats, strategy=torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match='strategy must have length 15'):
        d(feats, strategy=torch.zeros(2, 4, dtype=torch.long))
    d2 = tiny_decoder(lm=True)
    with pytest.raises(ValueError, match='cannot set `mi=` decoding'):
        d2(feats, strategy='rerank', mi=True)
    d2.train()
    with pytest.raises(ValueError, match='while training'):
        d2(feats, strategy='rerank')
    with pytest.raises(ValueError, match='encoder not supported: bad-config'):
        encoders.PyramidConvEncoder(config='bad-config')
    st = decoders.DecoderState(torch.zeros(2, 8), torch.zeros(2, 8),
                               torch.zeros(2, 2, 8), None)
    with pytest.raises(ValueError, match='both h_lm and c_lm'):
        d2.step(feats, torch.zeros(2, dtype=torch.long), st)


def test_defaults_and_attributes_match_reference():
    d = tiny_decoder()
    assert d.strategy == 'rerank' and d.beam_size == 50 and d.length == 15
    assert d.temperature == .2 and not d.training
    assert tiny_decoder(lm=False).strategy == 'beam'
    assert d.vocab_size == 16 and d.feature_size == 61 * 8
    assert d.indexer.start_index == 12 and d.indexer.stop_index == 13
    assert d.indexer.pad_index == 14 and d.indexer.unk_index == 15
    assert decoders.STRATEGIES == ('greedy', 'sample', 'beam', 'rerank')
    assert decoders.DecoderOutput._fields[:3] == ('captions', 'scores',
                                                  'tokens')


def test_vocab_mismatch_raises_like_reference():
    idx = lang.Indexer(lang.Vocab(('a', 'b')), None)
    other = lang.Indexer(lang.Vocab(('a', 'c')), None)
    enc = encoders.PyramidConvEncoder('resnet50', width=8)
    with pytest.raises(ValueError, match='different vocabs'):
        decoders.Decoder(idx, enc, lms.LanguageModel(other, 4, 8),
                         embedding_size=4, hidden_size=8)


# ---- captions ------------------------------------------------------------------
def test_reconstruct_matches_reference_table(golden_meta):
    idx = lang.Indexer(lang.Vocab(tuple(golden_meta['g6_vocab'])), None)
    for case, want in zip(golden_meta['g6_cases'], golden_meta['g6_expected']):
        assert idx.reconstruct(case) == want
    assert list(idx.reconstruct(
        golden_meta['g6_cases'])) == golden_meta['g6_expected_batch']
    for case, want in zip(golden_meta['g6_cases'], golden_meta['g6_unindex']):
        assert list(idx.unindex(case)) == want
    with pytest.raises(ValueError, match='unknown index: 99'):
        idx.reconstruct([5, 99])
    with pytest.raises(ValueError, match='at least one seq'):
        idx.reconstruct([])
    with pytest.raises(ValueError, match='input seq 1 is empty'):
        idx.reconstruct([[1], []])
    assert idx.reconstruct(['the', 'dog', '.']) == 'The dog.'
    lazy = lang.LazyCaptions(idx, torch.tensor([[[5, 8, 13], [8, 13, 13]]]))
    assert len(lazy) == 1 and lazy[0] == ('The dog', 'Dog')


# ---- checkpoints ----------------------------------------------------------------
def test_state_dict_names_match_reference_skeleton(golden_meta):
    """Every parameter name/shape of the reference Decoder (G7) exists here."""
    skel = golden_meta['g7_skeleton']
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(12)), None, True,
                       True, True, True, 15)

    class Fake(encoders.Encoder):
        feature_shape = (61,)

        def properties(self):
            return {'feature_size': 61}

    d = decoders.Decoder(idx, Fake(), lms.LanguageModel(idx, 4, 8),
                         embedding_size=4, hidden_size=8)
    mine = {k: f'tensor{tuple(v.shape)}:{v.dtype}'
            for k, v in d.state_dict().items()}
    assert mine == skel['state_dict']
    ser = d.serialize(state_dict=False)
    assert set(ser['properties']) == set(skel['properties'])
    assert set(ser['properties']['indexer']['properties']) == set(
        skel['properties']['indexer']['properties'])


def test_checkpoint_roundtrip_and_foreign_pickles(tmp_path):
    d = tiny_decoder()
    sd = synthetic.milan_state_dict(16, 'resnet50', seed=3, width=8,
                                    hidden_size=8, embedding_size=4,
                                    lm_hidden_size=8, lm_embedding_size=4)
    missing = d.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    path = tmp_path / 'milan-base.pth'
    d.save(path)
    back = decoders.Decoder.load(path)
    assert not back.training
    for k, v in d.state_dict().items():
        assert torch.equal(v, back.state_dict()[k]), k
    assert back.indexer.vocab.tokens == d.indexer.vocab.tokens
    assert back.encoder.config == 'resnet50' and back.encoder.width == 8

    # a reference checkpoint pickles spaCy/thinc objects we cannot import
    payload = d.serialize()
    import types
    mod = types.ModuleType('thinc_not_installed')

    Config = type('Config', (dict,), {
        '__module__': 'thinc_not_installed',
        '__qualname__': 'Config'
    })
    mod.Config = Config
    sys.modules['thinc_not_installed'] = mod
    try:
        payload['properties']['indexer']['properties']['tokenize'] = {
            'properties': {'nlp': (Config(lang='en'), b'\x00spacy-bytes'),
                           'lemmatize': False},
            'children': {}}
        torch.save(payload, path)
    finally:
        del sys.modules['thinc_not_installed']
    back = decoders.Decoder.load(path)  # must not need thinc
    assert back.indexer.tokenize['properties']['lemmatize'] is False

    os.environ['MILAN_MODELS_DIR'] = str(tmp_path)
    try:
        assert isinstance(loaders.pretrained('base'), decoders.Decoder)
        with pytest.raises(KeyError, match='no such model in hub'):
            loaders.pretrained('nonsense')
        (tmp_path / 'milan-base.pth').unlink()
        with pytest.raises(FileNotFoundError):
            loaders.pretrained('base')
    finally:
        del os.environ['MILAN_MODELS_DIR']
    with pytest.raises(ValueError, match='not a serialized MILAN module'):
        torch.save({'x': 1}, path)
        decoders.Decoder.load(path)


# ---- dataset -----------------------------------------------------------------
def test_top_images_dataset_contract(tmp_path):
    """Same on-disk format and validation as the reference loader
    (src/milannotations/datasets.py:159-197; tests/conftest.py:74-85)."""
    rng = numpy.random.default_rng(0)
    for layer, units in (('layer1', 3), ('layer2', 2)):
        (tmp_path / layer).mkdir()
        numpy.save(tmp_path / layer / 'images.npy',
                   rng.integers(0, 256, (units, 5, 3, 16, 16), dtype=numpy.uint8))
        numpy.save(tmp_path / layer / 'masks.npy',
                   rng.integers(0, 2, (units, 5, 1, 16, 16), dtype=numpy.uint8))
    numpy.save(tmp_path / 'layer2' / 'units.npy', numpy.array([7, 9]))
    ds = datasets.TopImagesDataset(tmp_path)
    assert len(ds) == 5 and ds.layers == ('layer1', 'layer2')
    s = ds[4]
    assert (s.layer, s.unit) == ('layer2', 9)
    assert s.images.dtype == torch.float32 and s.images.shape == (5, 3, 16, 16)
    assert float(s.images.max()) <= 1.0 and set(s.masks.unique().tolist()) <= {0., 1.}
    im, mk = ds.slice_uint8(1, 5)  # spans the layer boundary
    assert im.dtype == torch.uint8 and im.shape == (4, 5, 3, 16, 16)
    mul = torch.tensor(1 / 255, dtype=torch.float64).float()
    assert torch.equal(im[3].float().mul(mul), s.images)
    assert torch.equal(mk[3].float(), s.masks)
    # lookup is positional and echoes the key it was given, like the reference
    # (datasets.py:252-259)
    found = ds.lookup('layer2', 1)
    assert found.unit == 1 and torch.equal(found.images, s.images)
    assert ds.k == 5 and ds.unit(4) == ('layer2', 9)
    with pytest.raises(KeyError):
        ds.lookup('nope', 0)
    with pytest.raises(FileNotFoundError):
        datasets.TopImagesDataset(tmp_path / 'missing')
    (tmp_path / 'layer3').mkdir()
    with pytest.raises(FileNotFoundError, match='missing images.npy'):
        datasets.TopImagesDataset(tmp_path)


def test_slice_uint8_equals_getitem_when_units_file_truncates(tmp_path):
    """A `units.npy` shorter than `images.npy` truncates that layer
    (reference datasets.py:201-204); the uint8 fast path must hand out the
    same samples as `__getitem__`, in the same order."""
    import numpy
    g = torch.Generator().manual_seed(3)
    for layer, n_img, units in (('a', 4, [7, 9]), ('b', 3, None),
                                ('c', 5, [1, 2, 3])):
        d = tmp_path / layer
        d.mkdir()
        numpy.save(d / 'images.npy', torch.randint(
            0, 256, (n_img, 2, 3, 8, 8), dtype=torch.uint8, generator=g).numpy())
        numpy.save(d / 'masks.npy', torch.randint(
            0, 2, (n_img, 2, 1, 8, 8), dtype=torch.uint8, generator=g).numpy())
        if units is not None:
            numpy.save(d / 'units.npy', numpy.array(units))
    ds = datasets.TopImagesDataset(tmp_path)
    assert len(ds) == 2 + 3 + 3
    mul = torch.tensor(1 / 255, dtype=torch.float64).float()
    for lo, hi in ((0, 8), (0, 5), (1, 3), (2, 7), (4, 8), (3, 3)):
        im, mk = ds.slice_uint8(lo, hi) if hi > lo else (None, None)
        for j in range(lo, hi):
            s = ds[j]
            assert torch.equal(im[j - lo].float().mul(mul), s.images), (lo, hi, j)
            assert torch.equal(mk[j - lo].float(), s.masks)
        if hi > lo:
            # `out=`: rows land in caller-provided (e.g. pinned) staging buffers
            buf_i = torch.full((9, 2, 3, 8, 8), 255, dtype=torch.uint8)
            buf_m = torch.full((9, 2, 1, 8, 8), 255, dtype=torch.uint8)
            im2, mk2 = ds.slice_uint8(lo, hi, out=(buf_i, buf_m))
            assert torch.equal(im2, im) and torch.equal(mk2, mk)
            assert im2.data_ptr() == buf_i.data_ptr()
            im3, mk3 = ds.slice_uint8(lo, hi, out=(None, buf_m))
            assert torch.equal(im3, im) and mk3.data_ptr() == buf_m.data_ptr()
    with pytest.raises(IndexError):
        ds.slice_uint8(0, 9)
    assert ds.slice_uint8(3, 3)[0].shape == (0, 2, 3, 8, 8)


# ---- sharding ------------------------------------------------------------------
def test_partition_alignment_keeps_the_single_process_batch_groups():
    """Shards aligned to predict()'s batch_size: the union of the ranks'
    batch-of-16 groups equals the 1-process run's groups (allennlp's
    early-exit length T' is a per-group quantity and feeds the rerank score)."""
    for n in (1000, 1152, 3904, 4096, 17, 16, 0):
        for world in (1, 2, 3, 8):
            want = [(a, min(n, a + 16)) for a in range(0, n, 16)]
            got = []
            spans = [sharding.partition(n, world, r, align=16)
                     for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (lo, hi), nxt in zip(spans, spans[1:] + [(n, n)]):
                assert hi == nxt[0] and (lo % 16 == 0 or lo == n)
                got += [(a, min(hi, a + 16)) for a in range(lo, hi, 16)]
            assert got == want, (n, world)


def test_partition_is_contiguous_and_complete():
    for n in (0, 1, 7, 8, 4096, 1153):
        for world in (1, 2, 3, 8):
            spans = [sharding.partition(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (a, b), (c, d) in zip(spans, spans[1:]):
                assert b == c and a <= b and c <= d
            assert max(b - a for a, b in spans) == -(-n // world)
    with pytest.raises(ValueError):
        sharding.partition(4, 2, 2)


def _gloo_worker(rank, world, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    r, w, _ = sharding.init_from_env(world, backend='gloo')
    dev = torch.device('cpu')
    sd = synthetic.decoder_state_dict(20, feature_size=244, hidden_size=8,
                                      embedding_size=4, lm_hidden_size=8,
                                      lm_embedding_size=4) if r == 0 else None
    if r == 0:
        sd['encoder.encoder.model.bn1.num_batches_tracked'] = torch.tensor(5)
    got = sharding.broadcast_state_dict(sd, dev, src=0)
    ref = synthetic.decoder_state_dict(20, feature_size=244, hidden_size=8,
                                       embedding_size=4, lm_hidden_size=8,
                                       lm_embedding_size=4)
    ok = all(torch.equal(got[k], v) for k, v in ref.items())
    ok &= int(got['encoder.encoder.model.bn1.num_batches_tracked']) == 5
    ok &= got['encoder.encoder.model.bn1.num_batches_tracked'].dtype == torch.int64
    ok &= list(got)[:len(ref)] == list(ref)
    # ragged shards: 7 neurons over 2 ranks -> 4 + 3
    lo, hi = sharding.partition(7, w, r)
    tokens = torch.arange(lo, hi).view(-1, 1).repeat(1, 3)
    scores = torch.arange(lo, hi).float()
    t, s = sharding.gather_results(tokens, scores, dst=0)
    if r == 0:
        ok &= torch.equal(t[:, 0], torch.arange(7)) and torch.equal(
            s, torch.arange(7.))
    ok &= sharding.max_over_ranks(float(r), dev) == float(w - 1)
    sharding.finalize()
    pathlib.Path(tmp, f'ok{rank}').write_text(str(bool(ok)))


def test_world_size_two_broadcast_and_gather_over_gloo(tmp_path):
    port = 29000 + os.getpid() % 1000
    mp.spawn(_gloo_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / 'ok0').read_text() == 'True'
    assert (tmp_path / 'ok1').read_text() == 'True'


def _gloo_worker8(rank, world, port, tmp):
    """World 8, shards aligned to 16: ragged last shard AND empty shards (VERDICT r2
    item 6b).  Every neuron must come back exactly once, in order, on rank 0."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    r, w, _ = sharding.init_from_env(world, backend='gloo')
    ok = True
    for n in (100, 16, 7, 0, 1152):  # 100: ranks 0-5 x16, rank 6 x4, rank 7 empty
        lo, hi = sharding.partition(n, w, r, align=16)
        tokens = torch.arange(lo, hi).view(-1, 1).repeat(1, 15)
        scores = torch.arange(lo, hi).float() * 0.5
        t, s = sharding.gather_results(tokens, scores, dst=0)
        if r == 0:
            ok &= t.shape == (n, 15) and torch.equal(t[:, 3], torch.arange(n))
            ok &= torch.equal(s, torch.arange(n).float() * 0.5)
    sharding.finalize()
    pathlib.Path(tmp, f'ok{rank}').write_text(str(bool(ok)))


def test_world_size_eight_gather_with_ragged_and_empty_shards(tmp_path):
    # the partition arithmetic at the BASELINE sizes (no data needed)
    for n in (4096, 3904, 1152, 65536, 100, 7):
        spans = [sharding.partition(n, 8, r, align=16) for r in range(8)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(b == c for (_, b), (c, _) in zip(spans, spans[1:]))
        assert all(lo % 16 == 0 or lo == n for lo, _ in spans)
        assert max(hi - lo for lo, hi in spans) <= -(-(-(-n // 8)) // 16) * 16
    port = 29000 + (os.getpid() + 7) % 1000
    mp.spawn(_gloo_worker8, args=(8, port, str(tmp_path)), nprocs=8, join=True)
    for rank in range(8):
        assert (tmp_path / f'ok{rank}').read_text() == 'True', rank


def _sharded_load_worker(rank, world, port, tmp, path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sharding.init_from_env(world, backend='gloo')
    from milan_amd import loaders
    ok = True
    # only rank 0 can see the file: the others must get skeleton + weights by broadcast
    mine = path if rank == 0 else str(pathlib.Path(tmp, 'nowhere.pth'))
    model = loaders.pretrained_sharded('base', path=mine)
    want = torch.load(path, map_location='cpu')['state_dict']
    got = model.state_dict()
    ok &= all(torch.equal(got[k], v) for k, v in want.items())
    ok &= tuple(model.indexer.vocab.tokens) == tuple(synthetic.vocab_tokens(12))
    ok &= not model.training
    # a failure on the reading rank is raised on EVERY rank (nobody hangs in the
    # broadcast)
    try:
        loaders.pretrained_sharded('base', path=str(pathlib.Path(tmp, 'missing.pth')))
        ok = False
    except FileNotFoundError:
        pass
    sharding.finalize()
    pathlib.Path(tmp, f'ok{rank}').write_text(str(bool(ok)))


def test_pretrained_sharded_broadcasts_checkpoint_and_errors_over_gloo(tmp_path):
    d = tiny_decoder()
    path = tmp_path / 'milan-base.pth'
    d.save(path)
    port = 29000 + (os.getpid() + 13) % 1000
    mp.spawn(_sharded_load_worker, args=(2, port, str(tmp_path), str(path)),
             nprocs=2, join=True)
    assert (tmp_path / 'ok0').read_text() == 'True'
    assert (tmp_path / 'ok1').read_text() == 'True'


def test_shard_view_keeps_the_fast_path_of_predict(tmp_path):
    """One rank's block of a sharded run (scripts/compute_milan_descriptions.py):
    same samples as the parent's [lo, hi), `slice_uint8(..., out=)` included, and the
    attributes `Decoder.predict` checks before taking the uint8 path."""
    import numpy
    g = torch.Generator().manual_seed(5)
    for layer, n_img in (('a', 5), ('b', 4)):
        d = tmp_path / layer
        d.mkdir()
        numpy.save(d / 'images.npy', torch.randint(
            0, 256, (n_img, 2, 3, 8, 8), dtype=torch.uint8, generator=g).numpy())
        numpy.save(d / 'masks.npy', torch.randint(
            0, 2, (n_img, 2, 1, 8, 8), dtype=torch.uint8, generator=g).numpy())
    ds = datasets.TopImagesDataset(tmp_path)
    view = datasets.ShardView(ds, 3, 8)
    assert len(view) == 5 and view.unit(0) == ds.unit(3)
    assert view.transform_images is None and view.device is None
    assert torch.equal(view[1].images, ds[4].images) and view[-1].unit == ds[7].unit
    im, mk = ds.slice_uint8(4, 7)
    buf_i = torch.zeros(6, 2, 3, 8, 8, dtype=torch.uint8)
    im2, mk2 = view.slice_uint8(1, 4, out=(buf_i, None))
    assert torch.equal(im2, im) and torch.equal(mk2, mk)
    assert im2.data_ptr() == buf_i.data_ptr()
    import inspect
    assert 'out' in inspect.signature(view.slice_uint8).parameters
    ds.transform_images = lambda x: x
    assert view.transform_images is ds.transform_images  # predict() then avoids it
    with pytest.raises(IndexError):
        view.slice_uint8(0, 6)
    with pytest.raises(IndexError):
        datasets.ShardView(ds, 3, 10)


def test_exemplars_fail_loudly_without_gpu():
    """No CPU fallback in the exemplar computation either."""
    from milan_amd import exemplars
    model = synthetic.exemplar_model(3, 2, 0)
    dataset = torch.utils.data.TensorDataset(synthetic.exemplar_images(4, 16, 1))
    if torch.cuda.is_available():
        pytest.skip('needs a box without a GPU')
    with pytest.raises(hip.HipUnavailableError):
        exemplars.discriminative(model, dataset, layer='conv_2', k=2,
                                 image_size=16, num_workers=0)
    with pytest.raises(hip.HipUnavailableError):
        exemplars.RunningTopK(k=2).add(torch.zeros(3, 4))


def test_graft_entry_build_runs():
    """`__graft_entry__.build()` is the driver's "does it build" check."""
    import __graft_entry__
    __graft_entry__.build()
    assert callable(__graft_entry__.smoke)


def test_bench_and_script_entry_points_parse():
    """bench.py / the drop-in script at least import and parse their flags on
    a CPU-only host (the driver launches them by path)."""
    import subprocess
    import sys
    root = HEADER.parent.parent
    for path in (root / 'bench.py',
                 root / 'neuron-descriptions_amd' / 'scripts' /
                 'compute_milan_descriptions.py'):
        out = subprocess.run([sys.executable, str(path), '--help'],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-500:]
    out = subprocess.run([sys.executable, str(root / 'bench.py'), '--gpus', '1',
                          '--steps', '1'], capture_output=True, text=True,
                         timeout=300)
    # no GPU here: must fail loudly, not fall back to a CPU path
    assert out.returncode != 0
    assert 'no CPU fallback' in out.stderr or 'HIP' in out.stderr or \
        'cuda' in out.stderr.lower()


def test_bench_dump_outputs_types_and_budget(tmp_path):
    """bench.py --dump-outputs: one .npy per array describe() returned (integers as float64,
    floats as float32, values unchanged); over the byte budget, a seeded sample of rows --
    the same rows in every array of one leading length, the same sample on every run --
    and the budget holds also when an array that is not one row per neuron dominates."""
    if str(REPO) not in sys.path:
        sys.path.insert(0, str(REPO))
    import bench
    n, beam, length = 40, 6, 5
    g = torch.Generator().manual_seed(3)
    out = dict(tokens=torch.randint(0, 5004, (n, length), generator=g),
               scores=torch.randn(n, generator=g),
               predictions=None,
               beam_tokens=torch.randint(0, 5004, (n, beam, length), generator=g),
               beam_scores=torch.randn(n, beam, generator=g),
               out_len=torch.full((3,), length, dtype=torch.int32))
    shapes = bench.dump_outputs(out, tmp_path / 'all', n)
    assert shapes == {k: list(v.shape) for k, v in out.items() if v is not None}
    for name, want in out.items():
        if want is None:
            continue
        got = numpy.load(tmp_path / 'all' / f'{name}.npy')
        assert got.dtype == (numpy.float32 if want.is_floating_point() else numpy.float64)
        assert numpy.array_equal(got, want.double().numpy())
    budget = 12000
    for d in ('a', 'b'):
        bench.dump_outputs(out, tmp_path / d, n, budget=budget)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= budget
    rows = numpy.load(tmp_path / 'a' / 'rows.npy')
    assert numpy.array_equal(rows, numpy.load(tmp_path / 'b' / 'rows.npy'))
    assert 0 < len(rows) < n and numpy.all(numpy.diff(rows) > 0)
    idx = torch.from_numpy(rows).long()
    for name in ('tokens', 'scores', 'beam_tokens', 'beam_scores'):
        got = numpy.load(tmp_path / 'a' / f'{name}.npy')
        assert numpy.array_equal(got, out[name][idx].double().numpy()), name
    idx3 = torch.from_numpy(numpy.load(tmp_path / 'a' / 'rows_3.npy')).long()
    assert numpy.array_equal(numpy.load(tmp_path / 'a' / 'out_len.npy'),
                             out['out_len'][idx3].double().numpy())
    # an array of another leading length that alone exceeds the budget is sampled as well
    big = dict(out, attentions=torch.randn(7, 4000, generator=g))
    shapes = bench.dump_outputs(big, tmp_path / 'c', n, budget=5 * budget)
    assert sum(f.stat().st_size for f in (tmp_path / 'c').iterdir()) <= 5 * budget
    idx7 = torch.from_numpy(numpy.load(tmp_path / 'c' / 'rows_7.npy')).long()
    assert 0 < len(idx7) < 7 and shapes['attentions'] == [len(idx7), 4000]
    assert numpy.array_equal(numpy.load(tmp_path / 'c' / 'attentions.npy'),
                             big['attentions'][idx7].numpy())


def test_bench_plain_run_is_lean_and_full_runs_every_leg():
    """A plain `bench.py --gpus 1 --steps N --warmup W` runs no leg beyond the headline
    (PCIe-inclusive, f32 / fast modes, other configs, CPU baseline, live PMC traffic);
    `--full` turns every one on at its former default, and a flag given explicitly wins
    either way."""
    if str(REPO) not in sys.path:
        sys.path.insert(0, str(REPO))
    import bench
    legs = ('cpu_sample', 'from_host_steps', 'fast_steps', 'also_f32_steps',
            'live_traffic', 'other_configs')
    plain = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not plain.full and all(getattr(plain, k) == 0 for k in legs)
    assert (plain.steps, plain.warmup, plain.chunk, plain.precision) == (20, 5, 640, 'split_f16')
    full = bench.parse_args(['--full'])
    assert full.full
    assert {k: getattr(full, k) for k in legs} == {
        'cpu_sample': 32, 'from_host_steps': -1, 'fast_steps': 8, 'also_f32_steps': 8,
        'live_traffic': 1, 'other_configs': 1}
    assert bench.parse_args(['--full', '--cpu-sample', '0']).cpu_sample == 0
    assert bench.parse_args(['--also-f32-steps', '2']).also_f32_steps == 2


def test_shared_gpu_probe_is_quiet_without_a_gpu(recwarn):
    """hip.other_compute_processes(): PIDs with compute queues on a GPU this process
    uses (/sys/class/kfd/kfd/proc/<pid>/queues/*/gpuid).  A process without queues --
    every CPU test -- has no such neighbours, and the warning stays silent."""
    assert hip.other_compute_processes() == []
    hip.warn_if_gpu_is_shared()
    assert not [w for w in recwarn.list if 'compute queues' in str(w.message)]


def test_check_isa_pins_the_instruction_streams_of_the_ring_kernels():
    """VERDICT r4 item 8 / ADVICE r3: the hand-counted `s_waitcnt vmcnt(N)` sites were written
    against a definite number of VMEM operations per kernel; tools/check_isa.py disassembles
    the built objects and asserts them (runs in build() and as `make check-isa`)."""
    import subprocess
    import sys
    build = REPO / 'neuron-descriptions_amd' / 'csrc' / 'build'
    if not (build / 'chain3.o').exists():
        pytest.skip('library objects not built in this checkout')
    out = subprocess.run([sys.executable, str(REPO / 'tools' / 'check_isa.py')],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert 'kernels match' in out.stdout


def test_check_isa_catches_a_destination_touched_before_its_wait(tmp_path):
    """chain3 / chain / conv3 read LDS through inline asm with "=v" outputs
    and hand-counted lgkmcnt waits; between the read and the wait that covers it the compiler
    may copy or spill the destination.  tools/check_isa.py::pending_hazards walks the
    disassembly with the in-order queue model and must flag exactly that -- shown on
    deliberately broken kernels (a destination copied before the wait, a wait that allows one
    read too many, an asm VMEM load stored before vmcnt covers it) and on their correct twin."""
    import subprocess
    import sys
    hipcc = pathlib.Path('/opt/rocm/bin/hipcc')
    if not hipcc.exists():
        pytest.skip('no hipcc')
    sys.path.insert(0, str(REPO / 'tools'))
    import check_isa
    obj = tmp_path / 'hz.o'
    subprocess.run([str(hipcc), '--offload-arch=gfx950', '-O3', '-c',
                    str(REPO / 'tests' / 'golden' / 'isa_hazard_cases.hip'), '-o', str(obj)],
                   check=True, capture_output=True)
    found = {name: check_isa.pending_hazards(lines)
             for name, lines in check_isa.kernels(check_isa.disassemble(obj)).items()}
    by = lambda key: next(v for k, v in found.items() if key in k)
    assert by('hazard_good') == []
    count, copy, vmem = by('hazard_broken_count'), by('hazard_broken_copy'), by('hazard_broken_vmem')
    assert len(count) == 1 and count[0][0].startswith('v_add_f32') and 'ds_read_b128' in count[0][1]
    assert len(copy) == 1 and copy[0][0].startswith('v_mov_b32') and 'ds_read_b128' in copy[0][1]
    assert len(vmem) == 1 and vmem[0][0].startswith('global_store') and 'global_load' in vmem[0][1]


def test_check_isa_queue_model_on_handwritten_streams():
    """The queue model itself, on instruction streams small enough to read: in-order retire
    by lgkmcnt(N), LDS writes counting as 'issued behind', a skipped (execz) load, a loop
    whose back edge carries a pending read into the next iteration's first instruction."""
    import sys
    sys.path.insert(0, str(REPO / 'tools'))
    import check_isa

    def asm(*rows):
        return [f'{text:<60}// {0x1000 + 4 * k:012X}: 00000000{tgt}'
                for k, (text, tgt) in enumerate(
                    (r if isinstance(r, tuple) else (r, '')) for r in rows)]

    ok = asm('ds_read_b128 v[0:3], v8', 'ds_read_b128 v[4:7], v9', 's_waitcnt lgkmcnt(1)',
             'v_mov_b32_e32 v10, v0', 's_waitcnt lgkmcnt(0)', 'v_mov_b32_e32 v11, v4', 's_endpgm')
    assert check_isa.pending_hazards(ok) == []
    # an LDS write behind the read retires it at lgkmcnt(1); a scalar load would not
    ok2 = asm('ds_read_b128 v[0:3], v8', 'ds_write_b128 v9, v[4:7]', 's_waitcnt lgkmcnt(1)',
              'v_mov_b32_e32 v10, v0', 's_endpgm')
    assert check_isa.pending_hazards(ok2) == []
    bad = asm('ds_read_b128 v[0:3], v8', 's_load_dword s4, s[0:1], 0x0', 's_waitcnt lgkmcnt(1)',
              'v_mov_b32_e32 v10, v0', 's_endpgm')
    assert len(check_isa.pending_hazards(bad)) == 1
    # the load under `s_cbranch_execz` may be skipped: vmcnt(1) then does NOT cover the first one
    skip = asm('global_load_dwordx4 v[0:3], v[8:9], off',
               ('s_cbranch_execz 1', ' <k+0xc>'),
               'global_load_dwordx4 v[4:7], v[10:11], off',
               's_waitcnt vmcnt(1)', 'v_mov_b32_e32 v12, v0', 's_endpgm')
    assert len(check_isa.pending_hazards(skip)) == 1
    # scratch spill of a pending destination = what the allocator did to chain3 in round 5
    spill = asm('ds_read_b128 v[0:3], v8', 'scratch_store_dwordx4 off, v[0:3], off',
                's_waitcnt lgkmcnt(0)', 's_endpgm')
    assert len(check_isa.pending_hazards(spill)) == 1
    # loop: the read issued at the bottom is consumed at the top of the next trip without a wait
    loop = asm('v_mov_b32_e32 v10, v0', 'ds_read_b128 v[0:3], v8',
               ('s_cbranch_scc1 65533', ' <k+0x0>'), 's_waitcnt lgkmcnt(0)', 's_endpgm')
    assert len(check_isa.pending_hazards(loop)) == 1
    assert check_isa.scratch_in_loops(asm(
        'scratch_load_dword v1, off, off', 'v_mov_b32_e32 v10, v0',
        'scratch_load_dword v2, off, off', ('s_cbranch_scc1 65533', ' <k+0x4>'),
        's_endpgm')) == ['scratch_load_dword v2, off, off']
