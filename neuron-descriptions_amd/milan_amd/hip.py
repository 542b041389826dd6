"""ctypes binding of libmilan_hip.so (the C ABI in include/milan_hip.h).

This is the only place the Python mirror touches native code.  There is NO
fallback: if the library cannot be loaded, or no HIP device is present,
everything that computes raises `HipUnavailableError` -- the product path
never routes through torch ops or the CPU oracle.

Tensors cross the boundary as raw device pointers (`tensor.data_ptr()`) on
torch's current HIP stream; torch only owns memory here.
"""
import ctypes
import os
import pathlib
import weakref
from typing import Dict, Optional, Sequence, Tuple

import torch

from milan_amd import synthetic

# MILAN_LIB=<path>: load another build of the library (A/B timing of compiler options)
LIB_PATH = pathlib.Path(os.environ.get('MILAN_LIB') or
                       pathlib.Path(__file__).resolve().parent / 'lib' / 'libmilan_hip.so')
# `make EXPERIMENTS=1` (built by __graft_entry__.build() as well): the measured-and-rejected
# kernels, for the parity tests of those kernels and the tools/bench/ launchers
EXP_LIB_PATH = pathlib.Path(__file__).resolve().parent / 'lib' / 'libmilan_hip_exp.so'

GREEDY, FORCED, BEAM, RERANK = 0, 1, 2, 3  # MILAN_GREEDY / _FORCED / _BEAM / _RERANK
PRECISION_F32, PRECISION_SPLIT_F16, PRECISION_F16 = 0, 1, 2
# 'f16' = the fast mode: narrower than the reference's fp32 (include/milan_hip.h), never a default
PRECISIONS = {'f32': PRECISION_F32, 'split_f16': PRECISION_SPLIT_F16, 'f16': PRECISION_F16}
FUSE_CHAIN, FUSE_CHAIN_WIDE, FUSE_STEM, FUSE_CONV3, FUSE_SKIP_EMPTY, FUSE_BNECK, FUSE_SPARSE_TAIL = 1, 2, 4, 8, 16, 32, 64  # milan_set_fusion flags (include/milan_hip.h)
FUSE_TAIL_LISTS = 128
SKETCH_COMPACT, SKETCH_INSERT, SKETCH_MOVE, SKETCH_HALVE = 0, 1, 2, 3
# milan_status bits (include/milan_hip.h)
STATUS_SATURATED, STATUS_NONFINITE_INPUT = 1, 2
FEATURE_SCALE_LOG2_MAX = 30  # MILAN_FEATURE_SCALE_LOG2_MAX
# enum milan_kernel_family (milan_profile_read_kernels)
KERNEL_FAMILIES = ('other', 'pp32_256', 'pp32_128', 'split_other', 'f32', 'chain',
                   'chain_wide', 'stem', 'conv3', 'f16', 'pp32t_256', 'bneck')


class SketchOp(ctypes.Structure):
    """`milan_sketch_op` (include/milan_hip.h)."""
    _fields_ = [('kind', ctypes.c_int32), ('src', ctypes.c_int32),
                ('dst', ctypes.c_int32), ('offset', ctypes.c_int32),
                ('extremes', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('n', ctypes.c_int64), ('position', ctypes.c_int64),
                ('capacity', ctypes.c_int64)]


DRAW_BIT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)
# conv2d_nhwc test hook only: split_f16 with the LDS-strip 3x3 kernel forced
_CONV_PRECISIONS = dict(f32=0, split_f16=1, split_f16_strip=3, split_f16_tap_major=4,
                        split_f16_tap_linear=5)
DTYPE_U8, DTYPE_F32 = 0, 1

ERR_ARG, ERR_SHAPE, ERR_STATE, ERR_WORKSPACE, ERR_NO_LM = -1, -2, -3, -4, -5
ERR_INDEX = -6  # a unit beyond its layer's channels (milan_set_ablation): IndexError


class HipUnavailableError(RuntimeError):
    """libmilan_hip.so or a HIP device is missing."""


class Dims(ctypes.Structure):
    """struct milan_dims."""
    _fields_ = [
        ('trunk_width', ctypes.c_int32),
        ('trunk_blocks', ctypes.c_int32 * 4),
        ('feature_size', ctypes.c_int32),
        ('hidden_size', ctypes.c_int32),
        ('embedding_size', ctypes.c_int32),
        ('attention_size', ctypes.c_int32),
        ('vocab_size', ctypes.c_int32),
        ('start_index', ctypes.c_int32),
        ('stop_index', ctypes.c_int32),
        ('pad_index', ctypes.c_int32),
        ('has_lm', ctypes.c_int32),
        ('lm_hidden_size', ctypes.c_int32),
        ('lm_embedding_size', ctypes.c_int32),
        ('lm_layers', ctypes.c_int32),
        ('trunk_kind', ctypes.c_int32),
    ]


class ClipDims(ctypes.Structure):
    """struct milan_clip_dims."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        'resolution', 'patch', 'vision_width', 'vision_layers', 'vision_heads',
        'embed_dim', 'context_length', 'vocab_size', 'text_width',
        'text_layers', 'text_heads')]


class BertDims(ctypes.Structure):
    """struct milan_bert_dims."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        'vocab_size', 'width', 'layers', 'heads', 'intermediate',
        'max_positions', 'type_vocab', 'position_offset')] + [('eps', ctypes.c_float)]


BERT_MAX_TOKENS = 64  # MILAN_BERT_MAX_TOKENS


class VitDims(ctypes.Structure):
    """struct milan_vit_dims."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        'resolution', 'patch', 'width', 'layers', 'heads', 'hidden')] + [('eps', ctypes.c_float)]


class GanDims(ctypes.Structure):
    """struct milan_gan_dims."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        'ch', 'dim_z', 'shared_dim', 'n_classes', 'resolution', 'bottom_width',
        'attn_resolution', 'hier')] + [('bn_eps', ctypes.c_float),
                                       ('out_bn_eps', ctypes.c_float)]


ABI_VERSION = 11  # MILAN_ABI_VERSION this binding was written against

# milan_dims.trunk_kind and the pyramid width multiplier (F = mult * width)
TRUNK_BOTTLENECK, TRUNK_BASIC, TRUNK_ALEXNET, TRUNK_NONE = 0, 1, 2, 3
TRUNK_ALEXNET_PLACES = 4  # the Places365 AlexNet: classify / ablate / activations only
# torchvision's VGG-11/13/16/19 (no batch norm): classify / ablate / activations only
TRUNK_VGG = 5
# (a VGG context cannot encode: nothing reads its multiplier but `make_dims`)
_FEATURE_MULT = {TRUNK_BOTTLENECK: 61, TRUNK_BASIC: 16, TRUNK_ALEXNET: 18,
                 TRUNK_ALEXNET_PLACES: 43, TRUNK_VGG: 23}
# channels of conv1..conv5 per unit of `trunk_width` (the reference's net has width 32)
PLACES_ALEXNET_CHANNELS = synthetic.PLACES_ALEXNET_CHANNELS


def level_shapes(kind: int, width: int, h: int, w: int):
    """[(C, h, w)] of the tensors of levels 0..4 (`Context.activations`) that a trunk of
    `kind` and `width` makes of an h x w image."""
    if kind == TRUNK_VGG:
        # 3x3 / pad 1 convs keep the extent; a 2x2 / 2 pool in front of blocks 2..5 halves it
        # (floor).  (The library refuses an image too small for a level.)
        return [(width * m, h >> l, w >> l) for l, m in enumerate(synthetic.VGG_CHANNELS)]
    if kind in (TRUNK_ALEXNET, TRUNK_ALEXNET_PLACES):
        # conv1 11x11/4 pad 2 (Places: pad 0); pool1, pool2 3x3/2 before conv2, conv3; the
        # rest keep.  (The library refuses an image too small for a level: at least 1 then.)
        places = kind == TRUNK_ALEXNET_PLACES
        mult = PLACES_ALEXNET_CHANNELS if places else synthetic.ALEXNET_CHANNELS
        pad = 0 if places else 2
        extents = [((h + 2 * pad - 11) // 4 + 1, (w + 2 * pad - 11) // 4 + 1)]
        for _ in range(2):
            extents.append(tuple((x - 3) // 2 + 1 for x in extents[-1]))
        extents += extents[-1:] * 2
        return [(width * m, max(hl, 1), max(wl, 1)) for m, (hl, wl) in zip(mult, extents)]
    # conv1 7x7/2 pad 3, then the maxpool and every later stage 3x3/2 pad 1
    extents = [((h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1)]
    for _ in range(4):
        extents.append(tuple((x + 2 - 3) // 2 + 1 for x in extents[-1]))
    wide = width if kind == TRUNK_BASIC else width * 4
    return [(c, hl, wl) for c, (hl, wl) in zip([width] + [wide << l for l in range(4)], extents)]


_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_SZ = ctypes.c_size_t
_I64 = ctypes.c_int64

# name -> (restype, argtypes); must list every symbol include/milan_hip.h
# declares (tests/test_host.py checks the two against each other).
SIGNATURES = {
    'milan_abi_version': (_I, []),
    'milan_last_error': (ctypes.c_char_p, []),
    'milan_create': (_I, [ctypes.POINTER(_P), _I,
                          ctypes.POINTER(Dims)]),
    'milan_destroy': (None, [_P]),
    'milan_set_weight':
        (_I, [_P, ctypes.c_char_p, _P,
              ctypes.POINTER(ctypes.c_int64), _I]),
    'milan_finalize_weights': (_I, [_P, _P]),
    'milan_workspace_bytes': (_SZ, [_P, _I, _I, _I, _I, _I]),
    'milan_encode': (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    'milan_encode_spatial': (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    'milan_init_state': (_I, [_P, _P, _I, _I, _P, _P, _P, _SZ, _P]),
    'milan_step':
        (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _SZ,
              _P]),
    'milan_decode': (_I, [
        _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P,
        _SZ, _P
    ]),
    'milan_lm_score': (_I, [_P, _P, _I, _I, _P, _P, _P, _SZ, _P]),
    'milan_lm_logprobs': (_I, [_P, _P, _I, _I, _P, _P, _SZ, _P]),
    'milan_describe': (_I, [
        _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P,
        _P, _P, _P, _P, _P, _P, _SZ, _P
    ]),
    'milan_beam_merge': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _SZ,
                              _P]),
    'milan_row_select': (_I, [_P, _P, _F, _I, _I, _I, _P, _I, _P, _P, _I, _P]),
    'milan_set_beam_path': (_I, [_P, _I]),
    'milan_get_beam_path': (_I, [_P]),
    'milan_set_ablation': (_I, [_P, _P, _P, _I, _P]),
    'milan_classify_workspace_bytes': (_SZ, [_P, _I, _I, _I, _I]),
    'milan_classify': (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    'milan_classify_sweep':
        (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    'milan_activations_workspace_bytes': (_SZ, [_P, _I, _I, _I]),
    'milan_activations': (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P, _SZ, _P]),
    'milan_set_alexnet_head':
        (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _P]),
    'milan_set_alexnet_lrn': (_I, [_P, _I, _F, _F]),
    'milan_set_vgg_head':
        (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _I, _P]),
    'milan_vgg_trace': (_I, [_P, _P, _P]),
    'milan_lrn': (_I, [_P, ctypes.c_longlong, _I, _I, _I, _F, _F, _P, _P, _P]),
    'milan_linear_packed_bytes': (_SZ, [_I, _I]),
    'milan_linear_pack': (_I, [_P, _I, _I, _P, _P]),
    'milan_linear': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    'milan_linear_rowwise': (_I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    'milan_set_graph_capture': (_I, [_P, _I]),
    'milan_graph_stats': (_I, [
        _P, ctypes.POINTER(ctypes.c_longlong),
        ctypes.POINTER(ctypes.c_longlong)
    ]),
    'milan_set_fusion': (_I, [_P, _I]),
    'milan_set_image_sharing': (_I, [_P, _I]),
    'milan_get_image_sharing': (_I, [_P]),
    'milan_image_sharing_stats': (_I, [
        _P, ctypes.POINTER(ctypes.c_longlong),
        ctypes.POINTER(ctypes.c_longlong), _I, _P
    ]),
    'milan_set_precision': (_I, [_P, _I]),
    'milan_get_precision': (_I, [_P]),
    'milan_profile_enable': (_I, [_I]),
    'milan_profile_read': (_I, [
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_double),
        ctypes.POINTER(ctypes.c_longlong)
    ]),
    'milan_profile_read_stages': (_I, [ctypes.POINTER(ctypes.c_double)]),
    'milan_profile_read_kernels': (_I, [ctypes.POINTER(ctypes.c_double)]),
    'milan_status': (_I, [_P, ctypes.POINTER(ctypes.c_uint32), _I, _P]),
    'milan_set_act_scale_log2': (_I, [_P, _I, _P]),
    'milan_get_act_scale_log2': (_I, [_P]),
    'milan_set_feature_scale_log2': (_I, [_P, _I, _P]),
    'milan_get_feature_scale_log2': (_I, [_P]),
    'milan_get_feature_absmax': (_F, [_P]),
    'milan_set_embedding_scale_log2': (_I, [_P, _I, _P]),
    'milan_get_embedding_scale_log2': (_I, [_P]),
    'milan_get_embedding_absmax': (_F, [_P]),
    'milan_encoder_absmax':
        (_I, [_P, _P, _I, _I, _I, _I, ctypes.POINTER(_F), _P, _SZ, _P]),
    'milan_exemplar_topk_update':
        (_I, [_P, _I, _I, _I, _P, _I, _I64, _I, _I, _P, _P, _P, _P]),
    'milan_exemplar_sketch_append':
        (_I, [_P, _I, _I, _I, _P, _I, _I64, _I64, _P, _I64, _I64, _P]),
    'milan_exemplar_sort_workspace': (_SZ, [_I, _I64, _I]),
    'milan_exemplar_sketch_compact':
        (_I, [_P, _I64, _I64, _I, _I, _P, _I64, _I64, _P, _P, _SZ, _P]),
    'milan_exemplar_sketch_add_workspace':
        (_SZ, [_I, _I64, ctypes.POINTER(_I64), _I]),
    'milan_exemplar_sketch_add':
        (_I, [_P, _I, _I, _I, _P, _I, _I64, ctypes.POINTER(_I64),
              ctypes.POINTER(_P), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
              _I, _P, _I64, ctypes.POINTER(_I64), _P, _P, _SZ, _P]),
    'milan_exemplar_rows_extremes': (_I, [_P, _I64, _I, _P, _P]),
    'milan_exemplar_sketch_plan_shift':
        (_I, [_I64, _I64, _I, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64),
              _P, _P, _P, _I, ctypes.POINTER(_I), ctypes.POINTER(_I64),
              ctypes.POINTER(_I64), ctypes.POINTER(_I)]),
    'milan_exemplar_sketch_quantile':
        (_I, [ctypes.POINTER(_P), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
              _I, _I, _P, _F, _P, _P, _SZ, _P]),
    'milan_exemplar_render':
        (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P,
              ctypes.POINTER(_F), ctypes.POINTER(_F), _I, _I, _P, _P, _P, _P]),
    'milan_lm_train_workspace_bytes': (_SZ, [_P, _I, _I]),
    'milan_lm_nll': (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _P, _SZ, _P]),
    'milan_lm_train_step':
        (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _F, ctypes.c_uint64, _P, _P,
              _SZ, _P]),
    'milan_lm_grad_workspace_bytes': (_SZ, [_P, _I, _I]),
    'milan_lm_forward_train':
        (_I, [_P, _P, _I, _P, _I, _I, _F, ctypes.c_uint64, _P, _P, _P, _P, _SZ,
              _P]),
    'milan_lm_backward':
        (_I, [_P, _P, _P, _I, _P, _I, _I, _F, ctypes.c_uint64, _P, _P, _P, _P,
              _SZ, _P]),
    'milan_decoder_train_workspace_bytes': (_SZ, [_P, _I, _I, _I]),
    'milan_decoder_nll':
        (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    'milan_decoder_train_step':
        (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _F, ctypes.c_uint64, _F, _P,
              _P, _SZ, _P]),
    'milan_decoder_grad_workspace_bytes': (_SZ, [_P, _I, _I, _I]),
    'milan_decoder_forward_train':
        (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _F, ctypes.c_uint64, _P, _P, _P,
              _SZ, _P]),
    'milan_decoder_backward':
        (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _F, ctypes.c_uint64, _P, _P,
              _P, _P, _SZ, _P]),
    'milan_clip_create': (_I, [ctypes.POINTER(_P), _I,
                               ctypes.POINTER(ClipDims)]),
    'milan_clip_destroy': (None, [_P]),
    'milan_clip_set_weight':
        (_I, [_P, ctypes.c_char_p, _P,
              ctypes.POINTER(ctypes.c_int64), _I]),
    'milan_clip_finalize_weights': (_I, [_P, _P]),
    'milan_clip_image_workspace_bytes': (_SZ, [_P, _I, _I]),
    'milan_clip_encode_images':
        (_I, [_P, _P, _I, _I, _P, ctypes.c_uint64, _I,
              ctypes.POINTER(_F), _P, _P, _SZ, _P]),
    'milan_clip_text_workspace_bytes': (_SZ, [_P, _I, _I]),
    'milan_clip_encode_texts': (_I, [_P, _P, _I, _I, _P, _P, _SZ, _P]),
    'milan_clip_rerank_scores':
        (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P]),
    'milan_bert_create': (_I, [ctypes.POINTER(_P), _I,
                               ctypes.POINTER(BertDims)]),
    'milan_bert_destroy': (None, [_P]),
    'milan_bert_set_weight':
        (_I, [_P, ctypes.c_char_p, _P,
              ctypes.POINTER(ctypes.c_int64), _I]),
    'milan_bert_finalize_weights': (_I, [_P, _P]),
    'milan_bert_encode_workspace_bytes': (_SZ, [_P, _I, _I]),
    'milan_bert_encode': (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    'milan_bert_score_pairs': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
    'milan_conv2d_nhwc':
        (_I, [_P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I,
              _P]),
    'milan_gemm_probe': (_I, [_P, _P]),
    'milan_attention': (_I, [_P, _P, _I, _I, _I, _I, _P]),
    'milan_vit_create': (_I, [ctypes.POINTER(_P), _I,
                              ctypes.POINTER(VitDims)]),
    'milan_vit_destroy': (None, [_P]),
    'milan_vit_set_weight':
        (_I, [_P, ctypes.c_char_p, _P,
              ctypes.POINTER(ctypes.c_int64), _I]),
    'milan_vit_finalize_weights': (_I, [_P, _P]),
    'milan_vit_workspace_bytes': (_SZ, [_P, _I]),
    'milan_vit_run': (_I, [_P, _P, _I, _I, ctypes.POINTER(_P), _P, _P, _SZ, _P]),
    'milan_sagan_attention': (_I, [_P, ctypes.c_int64, _P, _P, _I, _I, _I, _I, _P]),
    'milan_gan_create': (_I, [ctypes.POINTER(_P), _I,
                              ctypes.POINTER(GanDims)]),
    'milan_gan_destroy': (None, [_P]),
    'milan_gan_set_weight':
        (_I, [_P, ctypes.c_char_p, _P,
              ctypes.POINTER(ctypes.c_int64), _I]),
    'milan_gan_finalize_weights': (_I, [_P, _P]),
    'milan_gan_taps': (_I, [_P]),
    'milan_gan_workspace_bytes': (_SZ, [_P, _I]),
    'milan_gan_run': (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(_P), _P, _P, _SZ, _P]),
}

# entry points added without a new ABI version: a library built before them
# (an older MILAN_LIB) still loads, and the calls that need them say so
PROBED = ('milan_lm_grad_workspace_bytes', 'milan_lm_forward_train',
          'milan_lm_backward', 'milan_beam_merge', 'milan_row_select', 'milan_set_beam_path',
          'milan_get_beam_path', 'milan_set_ablation',
          'milan_classify_workspace_bytes', 'milan_classify',
          'milan_classify_sweep', 'milan_activations_workspace_bytes',
          'milan_activations', 'milan_set_alexnet_head', 'milan_set_alexnet_lrn', 'milan_lrn',
          'milan_set_vgg_head', 'milan_vgg_trace',
          'milan_linear_packed_bytes',
          'milan_linear_pack', 'milan_linear', 'milan_linear_rowwise', 'milan_attention',
          'milan_vit_create', 'milan_vit_destroy', 'milan_vit_set_weight',
          'milan_vit_finalize_weights', 'milan_vit_workspace_bytes', 'milan_vit_run',
          'milan_sagan_attention', 'milan_gan_create', 'milan_gan_destroy',
          'milan_gan_set_weight', 'milan_gan_finalize_weights', 'milan_gan_taps',
          'milan_gan_workspace_bytes', 'milan_gan_run', 'milan_gemm_probe')

_lib = None


def load_library(path: Optional[os.PathLike] = None) -> ctypes.CDLL:
    """dlopen libmilan_hip.so and attach signatures.  Loud on failure."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = pathlib.Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise HipUnavailableError(
            f'{p} not found: build it with `python -c "import __graft_entry__ '
            'as g; g.build()"` (or `make -C neuron-descriptions_amd/csrc`). '
            'There is no CPU fallback for the MILAN hot path.')
    try:
        lib = ctypes.CDLL(str(p))
    except OSError as error:
        raise HipUnavailableError(f'cannot load {p}: {error}') from error
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in PROBED and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.milan_abi_version() != ABI_VERSION:
        raise HipUnavailableError(
            f'{p} has C-ABI version {lib.milan_abi_version()}, this binding '
            f'needs {ABI_VERSION} (struct milan_dims differs): rebuild it')
    if path is None:
        _lib = lib
    return lib


def require_device(device: torch.device) -> torch.device:
    device = torch.device(device)
    if device.type != 'cuda' or not torch.cuda.is_available():
        raise HipUnavailableError(
            'milan_amd computes only on an AMD GPU (torch device "cuda" under '
            f'ROCm); got device={device}, cuda.is_available()='
            f'{torch.cuda.is_available()}. There is no CPU fallback.')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def _check(code: int) -> None:
    if code == 0:
        return
    msg = load_library().milan_last_error().decode(errors='replace')
    if code in (ERR_ARG, ERR_SHAPE, ERR_NO_LM):
        raise ValueError(msg)  # the reference raises ValueError for these
    if code == ERR_INDEX:
        raise IndexError(msg)  # `mask[:, units] = 0` (src/utils/ablations.py:39)
    raise RuntimeError(f'libmilan_hip error {code}: {msg}')


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _dev(t: torch.Tensor, device: torch.device, dtype=None) -> torch.Tensor:
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


_LIVE_CONTEXTS: 'weakref.WeakSet' = weakref.WeakSet()


def release_workspaces() -> None:
    """Drop the activation workspace of every live Context (up to 154 GB each at
    chunk_size 640; the next call re-allocates it) and hand torch's cached
    blocks back to the device -- for a process that is about to share its GPU
    with another one."""
    for ctx in list(_LIVE_CONTEXTS):
        ctx._ws = None
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _kfd_gpuids(pid) -> set:
    """GPU ids (KFD topology ids) on which process `pid` has compute queues."""
    ids = set()
    try:
        base = f'/sys/class/kfd/kfd/proc/{pid}/queues'
        for q in os.listdir(base):
            try:
                with open(f'{base}/{q}/gpuid') as f:
                    ids.add(f.read().strip())
            except OSError:
                pass
    except OSError:
        pass
    return ids


def other_compute_processes() -> list:
    """PIDs of OTHER processes with compute queues on a GPU this process uses.  Every
    process with a KFD context has a directory /sys/class/kfd/kfd/proc/<pid> whose
    queues/*/gpuid name the devices it runs on; processes on other GPUs of the node (other
    jobs' ranks, other containers) do not count."""
    mine = _kfd_gpuids(os.getpid())
    if not mine:
        return []
    try:
        pids = [int(p) for p in os.listdir('/sys/class/kfd/kfd/proc') if p.isdigit()]
    except OSError:
        return []
    return sorted(p for p in pids if p != os.getpid() and _kfd_gpuids(p) & mine)


_SHARED_WARNED = False


def warn_if_gpu_is_shared() -> None:
    """The library's execution model is one process per GPU and one stream per process
    (INTEGRATION.md): co-resident workgroups of different kernels are not safe on this
    platform (profiles/r4_coresidency_minimal.txt -- a compiler-generated MFMA loop
    corrupts the vector registers of a small kernel sharing its CU).  Ranks of one job
    that were deliberately put on one GPU (tests) see this warning too."""
    global _SHARED_WARNED
    others = other_compute_processes()
    if others and not _SHARED_WARNED:
        _SHARED_WARNED = True
        import warnings
        warnings.warn(
            f'milan_amd: {len(others)} other process(es) have compute queues on a GPU '
            f'this process uses (pids {others[:4]}{"..." if len(others) > 4 else ""}): '
            'kernels of two processes can become co-resident on a CU, which is '
            'unsupported on this platform (see INTEGRATION.md, "One process per GPU")',
            RuntimeWarning, stacklevel=3)


class Context:
    """Owns one `milan_ctx` (packed weights on one GPU) plus a workspace."""

    def __init__(self, dims: Dims, state_dict: Dict[str, torch.Tensor],
                 device: torch.device, finalize: bool = True,
                 alexnet_head: Optional[Sequence[torch.Tensor]] = None,
                 vgg_head: Optional[Sequence[torch.Tensor]] = None):
        """`finalize=False`: a context that only carries `dims` (no weights,
        no packed arena) -- what the LM training calls need.  `alexnet_head`: the six
        tensors of `set_alexnet_head`, installed once the weights are finalized;
        `vgg_head`: those of `set_vgg_head`."""
        self.lib = load_library()
        self.device = require_device(device)
        self.dims = dims
        # a VGG's convs per block, as the `vgg.B.J` keys give them (`ablation_levels`)
        self.vgg_blocks = tuple(
            sum(f'encoder.encoder.model.vgg.{b}.{j}.weight' in state_dict for j in range(4))
            for b in range(1, 6))
        self._h = _P()
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_create(ctypes.byref(self._h), self.device.index,
                                      ctypes.byref(dims)))
            keep = []
            fc = state_dict.get('encoder.encoder.model.fc.weight')
            self.num_classes = int(fc.shape[0]) if fc is not None else 0
            for name, tensor in state_dict.items():
                if not tensor.dtype.is_floating_point:
                    continue  # e.g. num_batches_tracked
                t = _dev(tensor.detach(), self.device, torch.float32)
                keep.append(t)
                shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
                _check(
                    self.lib.milan_set_weight(self._h, name.encode(),
                                              t.data_ptr(), shape, t.dim()))
            if finalize:
                _check(
                    self.lib.milan_finalize_weights(self._h,
                                                    _stream(self.device)))
            del keep
        self._ws: Optional[torch.Tensor] = None
        # what a saturated split-f16 value does (see `_guarded`): 'raise' (default),
        # 'f32' (rerun the call in the exact-fp32 mode: Decoder.precision = 'auto') or
        # 'ignore' (the caller reads `status()` itself, e.g. once after a timed region)
        self.on_saturation = os.environ.get('MILAN_ON_SATURATION', 'raise')
        self.saturation_fallbacks = 0
        _LIVE_CONTEXTS.add(self)
        warn_if_gpu_is_shared()  # (after the context exists: this process has queues)
        if os.environ.get('MILAN_CHAIN'):  # A/B timing (tools/ab_env.sh): flag bits
            bits = int(os.environ['MILAN_CHAIN'])
            self.set_fusion(chain=bool(bits & 1), wide=bool(bits & 2), stem=bool(bits & 4),
                            conv3=bool(bits & 8), skip_empty=bool(bits & 16),
                            bneck=bool(bits & 32), sparse_tail=bool(bits & 64),
                            tail_lists=bool(bits & 128))
        if os.environ.get('MILAN_SHARE_IMAGES'):  # opt-in image sharing (set_image_sharing)
            self.set_image_sharing(bool(int(os.environ['MILAN_SHARE_IMAGES'])))
        default = os.environ.get('MILAN_PRECISION')
        if default == 'auto':
            self.set_precision('split_f16')
            self.on_saturation = 'f32'
        elif default:
            self.set_precision(default)
        if alexnet_head is not None:
            self.set_alexnet_head(*alexnet_head)
        if vgg_head is not None:
            self.set_vgg_head(*vgg_head)

    # -- hipGraph replay of the decode stage ------------------------------------
    def enable_graphs(self, enable: bool = True) -> None:
        """Capture each distinct decode pass into a hipGraph and replay it.

        Pays off for small interactive batches, where the ~450 launches of a
        beam search are latency-bound.  Needs pointer-stable buffers and a
        non-default stream, so outputs then live in per-shape pools (callers get
        clones) and the calls run on a private stream that is joined with the
        caller's stream before and after.
        """
        _check(self.lib.milan_set_graph_capture(self._h, int(enable)))
        self._graphs = bool(enable)
        if enable and getattr(self, '_gstream', None) is None:
            self._gstream = torch.cuda.Stream(device=self.device)
            self._pool = {}

    def graph_stats(self):
        cap, rep = ctypes.c_longlong(), ctypes.c_longlong()
        _check(self.lib.milan_graph_stats(self._h, ctypes.byref(cap),
                                          ctypes.byref(rep)))
        return cap.value, rep.value

    def _pooled(self, key, make):
        buf = self._pool.get(key)
        if buf is None:
            self._pool[key] = buf = make()
        return buf

    def set_precision(self, precision) -> None:
        """'f32' (exact fp32 MFMA, default) or 'split_f16' (3xf16 MFMA)."""
        if isinstance(precision, str):
            if precision not in PRECISIONS:
                raise ValueError(f'unknown precision: {precision}')
            precision = PRECISIONS[precision]
        _check(self.lib.milan_set_precision(self._h, int(precision)))

    def set_fusion(self, chain: bool = True, wide: Optional[bool] = None,
                   stem: bool = True, conv3: bool = True, skip_empty: bool = True,
                   bneck: bool = True, sparse_tail: bool = True,
                   tail_lists: Optional[bool] = None) -> None:
        """Cross-layer fusions of the trunk (bitwise-neutral scheduling knob):
        `chain` the expand -> reduce launches of layer1 / layer2, `wide` those of
        layer3 (default: as `chain`), `stem` conv1 + bn1 + ReLU + maxpool as one launch, `conv3` the
        register-resident-weight kernel for layer1's 3x3 convolutions, `skip_empty` exemplars
        with an all-zero mask (exact-zero features by the reference's rule) stay out of the trunk,
        `bneck` (round 6) layer1's 3x3 conv runs in front of its chain launch (needs `chain`),
        `sparse_tail` (round 6) the last two bottlenecks run only at the pixels the level-4 pooling
        -- and their 3x3 neighbourhoods -- read, `tail_lists` (needs `sparse_tail`) those pixel
        sets go to the GEMM tile as row lists -- no gather / scatter / im2col copies -- and reach
        down to the first block of the last stage and c2 / c3 of the last block before it
        (default: as `sparse_tail`; asking for it without `sparse_tail` is an error, here as in
        `milan_set_fusion` and for a MILAN_CHAIN value with bit 128 but not bit 64)."""
        tail_lists = sparse_tail if tail_lists is None else tail_lists
        wide = chain if wide is None else wide
        _check(self.lib.milan_set_fusion(
            self._h, (FUSE_CHAIN if chain else 0) | (FUSE_CHAIN_WIDE if wide else 0) |
            (FUSE_STEM if stem else 0) | (FUSE_CONV3 if conv3 else 0) |
            (FUSE_SKIP_EMPTY if skip_empty else 0) | (FUSE_BNECK if bneck else 0) |
            (FUSE_SPARSE_TAIL if sparse_tail else 0) |
            (FUSE_TAIL_LISTS if tail_lists else 0)))

    # -- image sharing (opt-in) ------------------------------------------------------
    def set_image_sharing(self, enable: bool = True) -> None:
        """Exemplar slots of one encoder pass that hold byte-identical uint8 images share one
        trunk pass (ResNet trunks, pooled encode; the features keep their bits).  Off by
        default; float images, `encode_spatial` and AlexNet ignore it."""
        _check(self.lib.milan_set_image_sharing(self._h, int(bool(enable))))

    def set_beam_path(self, mode: int) -> None:
        """Which selection kernels the beam search runs: 0 (default) by beam width -- the
        LDS merge while beam^2 candidates fit LDS (124 beams), the wide merge above, the wide
        per-row top-k above 256 -- or 1, the wide kernels at every beam_size >= 2.  An A/B and test knob: both
        paths select the same beams, bit for bit."""
        if not hasattr(self.lib, 'milan_set_beam_path'):
            raise HipUnavailableError('this build of libmilan_hip has no milan_set_beam_path')
        _check(self.lib.milan_set_beam_path(self._h, int(mode)))

    @property
    def beam_path(self) -> int:
        if not hasattr(self.lib, 'milan_get_beam_path'):
            return 0
        return int(self.lib.milan_get_beam_path(self._h))

    @property
    def image_sharing(self) -> bool:
        return bool(self.lib.milan_get_image_sharing(self._h))

    def image_sharing_stats(self, clear: bool = False) -> Tuple[int, int]:
        """(slots, trunk_images) summed over the encoder passes run with sharing enabled:
        exemplar slots seen and images that went through the trunk.  Synchronises."""
        slots, trunk = ctypes.c_longlong(), ctypes.c_longlong()
        with torch.cuda.device(self.device):
            _check(self.lib.milan_image_sharing_stats(self._h, ctypes.byref(slots),
                                                      ctypes.byref(trunk), int(clear),
                                                      _stream(self.device)))
        return int(slots.value), int(trunk.value)

    @property
    def precision(self) -> str:
        code = self.lib.milan_get_precision(self._h)
        return {v: k for k, v in PRECISIONS.items()}[code]

    # -- split-f16 fails loudly ------------------------------------------------------
    def status(self, clear: bool = True) -> int:
        """The context's device status word (STATUS_* bits), read back through a stream
        synchronisation; `clear` resets it."""
        flags = ctypes.c_uint32(0)
        with torch.cuda.device(self.device):
            _check(self.lib.milan_status(self._h, ctypes.byref(flags), int(clear),
                                         _stream(self.device)))
        return int(flags.value)

    @property
    def act_scale_log2(self) -> int:
        return int(self.lib.milan_get_act_scale_log2(self._h))

    def set_act_scale_log2(self, k: int) -> None:
        """Activation scale 2^k of the split-f16 trunk (0..10): `hi` saturates at
        65504 / 2^k, `lo` keeps full precision down to activations of 0.125 / 2^k."""
        with torch.cuda.device(self.device):
            _check(self.lib.milan_set_act_scale_log2(self._h, int(k),
                                                     _stream(self.device)))

    @property
    def feature_scale_log2(self) -> int:
        return int(self.lib.milan_get_feature_scale_log2(self._h))

    def set_feature_scale_log2(self, k: int) -> None:
        """Feature scale 2^k of the split-f16 decoder (default 0): its feature-carrying
        operands are converted as x * 2^k and the factor is undone exactly, so features
        down to 0.125 / 2^k keep full precision and features above 65504 / 2^k raise.  A
        property of the context: set it once (or let `calibrate` do it), never per call."""
        with torch.cuda.device(self.device):
            _check(self.lib.milan_set_feature_scale_log2(self._h, int(k),
                                                         _stream(self.device)))

    @property
    def embedding_scale_log2(self) -> int:
        return int(self.lib.milan_get_embedding_scale_log2(self._h))

    def set_embedding_scale_log2(self, k: int) -> None:
        """Embedding scale 2^k of the split-f16 decoder and LM (default 0): the embedding
        tables are gathered as e * 2^k, the LSTM weight columns they meet hold W / 2^k."""
        with torch.cuda.device(self.device):
            _check(self.lib.milan_set_embedding_scale_log2(self._h, int(k),
                                                           _stream(self.device)))

    @staticmethod
    def feature_scale_log2_for(absmax: float, headroom: float = 8.0) -> int:
        """The feature scale `calibrate` picks for features of magnitude up to `absmax`:
        the largest power of two that keeps `headroom` x that maximum below the f16 range
        (the rule of the activation scale, without its 0..10 limits)."""
        import math
        if not absmax > 0 or not math.isfinite(absmax):
            return 0
        k = int(math.floor(math.log2(65504.0 / (absmax * headroom))))
        return max(-FEATURE_SCALE_LOG2_MAX, min(FEATURE_SCALE_LOG2_MAX, k))

    def encoder_absmax(self, images: torch.Tensor) -> float:
        """Largest |activation| any tensor of the ResNet trunk holds for `images`
        ((M,3,H,W), uint8 or float), measured in the exact-fp32 mode."""
        m, ch, h, w = images.shape
        if ch != 3:
            raise ValueError(f'images must have 3 channels, got {ch}')
        idt = DTYPE_U8 if images.dtype == torch.uint8 else DTYPE_F32
        images = _dev(images, self.device, None if idt == DTYPE_U8 else torch.float32)
        ws = self.workspace(m or 1, 1, max(h, w), 1, 1)
        out = _F(0.0)
        with torch.cuda.device(self.device):
            _check(self.lib.milan_encoder_absmax(self._h, images.data_ptr(), idt, m, h, w,
                                                 ctypes.byref(out), ws.data_ptr(),
                                                 ws.numel(), _stream(self.device)))
        return float(out.value)

    def calibrate(self, images: torch.Tensor, headroom: float = 8.0) -> int:
        """Pick the split trunk's activation scale from a sample: the largest power of
        two that keeps `headroom` x the observed maximum below the f16 range.  Returns
        the chosen log2 scale.  (The default 2^5 suits activations up to 2047; a
        network whose residual stream grows beyond that needs a smaller scale, one
        whose activations sit at 1e-3 a larger one -- DESIGN.md section 4.2.)  A context
        with a decoder also gets its feature scale, by the same rule without the 0..10
        limit, from the largest value of the sample's five pyramid taps (which bounds every
        mask-weighted mean the pooling can produce, whatever the masks), and its embedding
        scale, from the largest entry of its embedding tables (`feature_scale_log2`, `embedding_scale_log2`; DESIGN.md section
        4.21)."""
        import math
        amax = self.encoder_absmax(images)
        if not math.isfinite(amax):
            raise FloatingPointError('calibration sample produced non-finite activations')
        k = 10 if amax <= 0 else int(math.floor(math.log2(65504.0 / (amax * headroom))))
        k = max(0, min(10, k))
        self.set_act_scale_log2(k)
        if self.dims.hidden_size > 0 and hasattr(self.lib, 'milan_get_feature_absmax'):
            # The sample's features were pooled without masks (global averages); under a small
            # mask a feature is a mean over few pixels and can be far larger.  Every pooled
            # feature is a convex combination of the values of its pyramid tap, so the largest
            # |value| of the five taps (the activations and the raw conv1 output) bounds it
            # under ANY mask: that is what milan_get_feature_absmax returns.
            fmax = max(amax, float(self.lib.milan_get_feature_absmax(self._h)))
            self.set_feature_scale_log2(self.feature_scale_log2_for(fmax, headroom))
            with torch.cuda.device(self.device):
                emax = float(self.lib.milan_get_embedding_absmax(self._h))
            self.set_embedding_scale_log2(self.feature_scale_log2_for(emax, headroom))
        return k

    def _guarded(self, what: str, run, check: bool = True, decoder: bool = False):
        """Run one computing call and act on the status word it leaves behind.

        MILAN_STATUS_SATURATED: a split-format value hit the +-65504 clamp -- the
        reference's fp32 would not have, so the result is NOT returned: raise
        FloatingPointError, or (on_saturation == 'f32') rerun the call in the exact-fp32
        mode.  MILAN_STATUS_NONFINITE_INPUT: a float input pixel was NaN / Inf; the
        features of its image are NaN as in the reference -- a RuntimeWarning says so.
        `decoder`: the call reads features, not images (init_state, step, decode, lm_*):
        what saturates there is a feature beyond 65504 / 2^feature_scale_log2.  A NaN
        feature is no saturation: it poisons its neuron as in the reference, silently."""
        out = run()
        if not check or self.on_saturation == 'ignore':
            return out
        flags = self.status(clear=True)
        if flags & STATUS_NONFINITE_INPUT:
            import warnings
            warnings.warn(f'milan_amd: {what}: an input image holds NaN / Inf pixels; its '
                          'features are NaN (as in the reference)', RuntimeWarning,
                          stacklevel=3)
        if flags & STATUS_SATURATED:
            if what == 'describe':
                msg = (f'milan_amd: {what}: a split-f16 value was clamped: a trunk activation '
                       f'beyond {65504.0 / 2 ** self.act_scale_log2:g} (65504 / '
                       f'2^{self.act_scale_log2}), or a decoder operand (a feature, an '
                       f'embedding) beyond {65504.0 / 2.0 ** self.feature_scale_log2:g} / '
                       f'{65504.0 / 2.0 ** self.embedding_scale_log2:g} (65504 / '
                       f'2^{self.feature_scale_log2}, 2^{self.embedding_scale_log2}); the '
                       "exact-fp32 mode (precision='f32'), Decoder.precision = 'auto' or "
                       'smaller scales (Context.calibrate) avoid it')
            elif decoder:
                limit = 65504.0 / 2.0 ** self.feature_scale_log2
                msg = (f'milan_amd: {what}: a split-f16 decoder operand (a feature, or what '
                       f'the step computes from it) exceeded {limit:g} (65504 / '
                       f'2^{self.feature_scale_log2}) and was clamped; the exact-fp32 mode '
                       "(precision='f32'), Decoder.precision = 'auto' or a smaller feature "
                       'scale (Context.set_feature_scale_log2, Context.calibrate) avoid it')
            else:
                limit = 65504.0 / 2 ** self.act_scale_log2
                msg = (f'milan_amd: {what}: a split-f16 activation exceeded {limit:g} '
                       f'(65504 / 2^{self.act_scale_log2}) and was clamped; the exact-fp32 '
                       "mode (precision='f32'), Decoder.precision = 'auto' or a smaller "
                       'activation scale (Context.calibrate) avoid it')
            if self.on_saturation != 'f32' or self.precision == 'f32':
                raise FloatingPointError(msg)
            import warnings
            warnings.warn(msg + ' -- rerunning this call in f32', RuntimeWarning,
                          stacklevel=3)
            self.saturation_fallbacks += 1
            saved = self.precision
            self.set_precision('f32')
            try:
                out = run()
                self.status(clear=True)
            finally:
                self.set_precision(saved)
        return out

    def close(self) -> None:
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.milan_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter teardown
            pass

    # -- workspace ---------------------------------------------------------
    def workspace(self, neurons: int, k: int, image_size: int, beam: int,
                  length: int) -> torch.Tensor:
        need = int(
            self.lib.milan_workspace_bytes(self._h, neurons, k, image_size,
                                           beam, length))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None  # free before growing
            try:
                self._ws = torch.empty(need, dtype=torch.uint8,
                                       device=self.device)
            except torch.cuda.OutOfMemoryError as error:
                free, total = torch.cuda.mem_get_info(self.device)
                raise torch.cuda.OutOfMemoryError(
                    f'the activation workspace for {neurons} neurons x {k} '
                    f'exemplars needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} '
                    f'of {total / 2**30:.1f} GiB are free: lower '
                    'Decoder.chunk_size (or use Context.fit_neurons)') from error
        return self._ws

    def fit_neurons(self, neurons: int, k: int, image_size: int, beam: int,
                    length: int, multiple: int = 16,
                    headroom: float = 0.9) -> int:
        """Largest neuron count <= `neurons` (a multiple of `multiple`) whose
        workspace fits into `headroom` of the memory this process can still
        get (free memory + what the current workspace already holds).  The
        default chunk of 640 neurons takes 154 GB: fine on an idle 288 GB
        MI355X, not when the GPU is shared."""
        free, _ = torch.cuda.mem_get_info(self.device)
        budget = headroom * (free + (self._ws.numel() if self._ws is not None
                                     else 0))

        def need(n):
            return int(self.lib.milan_workspace_bytes(self._h, n, k, image_size,
                                                      beam, length))

        n = max(1, neurons)
        if need(n) <= budget:
            return n
        lo, hi = 0, n  # need(lo) fits (or lo == 0), need(hi) does not
        while hi - lo > multiple:
            mid = (lo + hi) // 2 // multiple * multiple
            if mid <= lo:
                break
            if need(mid) <= budget:
                lo = mid
            else:
                hi = mid
        if lo <= 0:
            lo = min(multiple, n)
        return lo

    # -- operators ----------------------------------------------------------
    def encode(self, images: torch.Tensor,
               masks: Optional[torch.Tensor], check: bool = True) -> torch.Tensor:
        """(M,3,H,W) [+ (M,1,H,W)] -> (M,F).  uint8 or float inputs.  `check`: read the
        status word afterwards (one stream synchronisation; see `_guarded`)."""
        m, ch, h, w = images.shape
        if ch != 3:
            raise ValueError(f'images must have 3 channels, got {ch}')
        idt = DTYPE_U8 if images.dtype == torch.uint8 else DTYPE_F32
        images = _dev(images, self.device,
                      None if idt == DTYPE_U8 else torch.float32)
        mdt = DTYPE_U8
        if masks is not None:
            if masks.shape != (m, 1, h, w):
                raise ValueError(
                    f'masks shape {tuple(masks.shape)} != {(m, 1, h, w)}')
            mdt = DTYPE_U8 if masks.dtype == torch.uint8 else DTYPE_F32
            masks = _dev(masks, self.device,
                         None if mdt == DTYPE_U8 else torch.float32)
        out = torch.empty(m,
                          self.dims.feature_size,
                          dtype=torch.float32,
                          device=self.device)
        ws = self.workspace((m + 0) or 1, 1, max(h, w), 1, 1)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_encode(self._h, images.data_ptr(), idt,
                                          _ptr(masks), mdt, m, h, w,
                                          out.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream(self.device)))
            return out

        return self._guarded('encode', run, check)

    def encode_spatial(self, images: torch.Tensor,
                       masks: Optional[torch.Tensor], check: bool = True) -> torch.Tensor:
        """SpatialConvEncoder: (M,3,H,W) [+ (M,1,H,W)] -> (M, h4*w4, C4)."""
        m, ch, h, w = images.shape
        if ch != 3:
            raise ValueError(f'images must have 3 channels, got {ch}')
        idt = DTYPE_U8 if images.dtype == torch.uint8 else DTYPE_F32
        images = _dev(images, self.device,
                      None if idt == DTYPE_U8 else torch.float32)
        mdt = DTYPE_U8
        if masks is not None:
            if masks.shape != (m, 1, h, w):
                raise ValueError(
                    f'masks shape {tuple(masks.shape)} != {(m, 1, h, w)}')
            mdt = DTYPE_U8 if masks.dtype == torch.uint8 else DTYPE_F32
            masks = _dev(masks, self.device,
                         None if mdt == DTYPE_U8 else torch.float32)

        def down(x, k, s, p):
            return (x + 2 * p - k) // s + 1

        h4, w4 = down(h, 7, 2, 3), down(w, 7, 2, 3)
        for _ in range(4):  # maxpool + the three stride-2 stages
            h4, w4 = down(h4, 3, 2, 1), down(w4, 3, 2, 1)
        mult = 8 if self.dims.trunk_kind == TRUNK_BASIC else 32
        out = torch.empty(m, h4 * w4, mult * self.dims.trunk_width,
                          dtype=torch.float32, device=self.device)
        ws = self.workspace(m or 1, 1, max(h, w), 1, 1)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_encode_spatial(self._h, images.data_ptr(), idt,
                                                  _ptr(masks), mdt, m, h, w,
                                                  out.data_ptr(), ws.data_ptr(),
                                                  ws.numel(), _stream(self.device)))
            return out

        return self._guarded('encode_spatial', run, check)

    # -- unit ablation and classification (ResNet trunks with an `fc` head; AlexNet once
    # `set_alexnet_head` has installed fc6 / fc7 / linear8) ----------------------------
    ABLATION_LEVELS = ('conv1', 'layer1', 'layer2', 'layer3', 'layer4')
    ALEXNET_LEVELS = ('conv1', 'conv2', 'conv3', 'conv4', 'conv5')

    @property
    def ablation_levels(self) -> Tuple[str, ...]:
        """The names of levels 0..4 on this context's trunk."""
        if self.dims.trunk_kind in (TRUNK_ALEXNET, TRUNK_ALEXNET_PLACES):
            return self.ALEXNET_LEVELS
        if self.dims.trunk_kind == TRUNK_VGG:
            return vgg_level_names(self.vgg_blocks)
        return self.ABLATION_LEVELS

    def set_alexnet_lrn(self, local_size: int = 5, alpha: float = 1e-4,
                        beta: float = 0.75) -> None:
        """Switch the Places365 AlexNet's across-channel LRN after pool1 and pool2 on
        (`local_size` odd, at most 17: the kernel reads one 8-channel neighbour each side) or off (0): y = x / (1 + alpha * S / local_size) ** beta, S the sum
        of squares over the `local_size` neighbouring channels, zero-padded."""
        fn = self._need('milan_set_alexnet_lrn')
        _check(fn(self._h, int(local_size), float(alpha), float(beta)))

    def set_alexnet_head(self, fc6_weight, fc6_bias, fc7_weight, fc7_bias, linear8_weight,
                         linear8_bias) -> None:
        """Install `alexnet_seq`'s three Linear layers on an AlexNet context (weights (out, in),
        biases (out,)): from then on `set_ablation`, `classify`, `classify_sweep` and
        `activations` accept it, with levels 'conv1'..'conv5'.  The library keeps packed
        copies.  The widths must chain from conv5's channels x 36 (ValueError)."""
        self._set_head('milan_set_alexnet_head', (fc6_weight, fc6_bias, fc7_weight, fc7_bias,
                                                  linear8_weight, linear8_bias))

    def set_vgg_head(self, fc0_weight, fc0_bias, fc3_weight, fc3_bias, fc6_weight,
                     fc6_bias) -> None:
        """Install torchvision's `classifier.0 / .3 / .6` on a VGG context (weights (out, in),
        biases (out,)): `classify` and `classify_sweep` need it, `set_ablation` and
        `activations` do not.  The library keeps packed copies.  The widths must chain from
        the last block's channels x 49 (ValueError)."""
        self._set_head('milan_set_vgg_head', (fc0_weight, fc0_bias, fc3_weight, fc3_bias,
                                              fc6_weight, fc6_bias))

    def vgg_trace(self):
        """What the walks of the last `classify` / `classify_sweep` / `activations` call
        launched on a VGG context: {(block 1..5, conv 0..3): (launches, 1 if the conv's last
        launch multiplied split operands else 0)} for the convs the context has."""
        fn = self._need('milan_vgg_trace')
        launches, split = (ctypes.c_int32 * 20)(), (ctypes.c_int32 * 20)()
        _check(fn(self._h, launches, split))
        return {(b + 1, j): (int(launches[4 * b + j]), int(split[4 * b + j]))
                for b, count in enumerate(self.vgg_blocks) for j in range(count)}

    def _set_head(self, entry: str, six) -> None:
        fn = self._need(entry)
        tensors = [_dev(t.detach(), self.device, torch.float32) for t in six]
        args = []
        for weight, bias in zip(tensors[0::2], tensors[1::2]):
            if weight.dim() != 2 or tuple(bias.shape) != (weight.shape[0],):
                raise ValueError(f'a Linear layer needs weight (out, in) and bias (out,), got '
                                 f'{tuple(weight.shape)} and {tuple(bias.shape)}')
            args += [weight.data_ptr(), bias.data_ptr(), weight.shape[0], weight.shape[1]]
        with torch.cuda.device(self.device):
            _check(fn(self._h, *args, _stream(self.device)))
        self.num_classes = int(tensors[4].shape[0])

    def _need(self, name: str):
        if not hasattr(self.lib, name):
            raise HipUnavailableError(f'this build of libmilan_hip has no {name}')
        return getattr(self.lib, name)

    def _unit_arrays(self, pairs):
        """[(level, unit), ...] -> two host int32 arrays; a level is 0..4 or its layer name."""
        levels, units = [], []
        for level, unit in pairs:
            if isinstance(level, str):
                if level not in self.ablation_levels:
                    raise ValueError(f'layer {level!r} cannot be ablated natively; the '
                                     f'layers are {self.ablation_levels}')
                level = self.ablation_levels.index(level)
            levels.append(int(level))
            units.append(int(unit))
        count = len(levels)
        return ((ctypes.c_int32 * max(1, count))(*levels),
                (ctypes.c_int32 * max(1, count))(*units), count)

    def set_ablation(self, pairs=()) -> None:
        """Install the set of (level, unit) pairs the classify calls zero (level 0..4 or its
        name in `ablation_levels`: 'conv1', 'layer1'..'layer4' on a ResNet, 'conv1'..'conv5'
        on AlexNet, the five `features.N` of the blocks' last convs on a VGG); an empty
        sequence clears it.  Duplicates and order do
        not matter.  `encode*` / `describe` never read it.  Synchronises the stream."""
        fn = self._need('milan_set_ablation')
        levels, units, count = self._unit_arrays(pairs)
        with torch.cuda.device(self.device):
            _check(fn(self._h, levels, units, count, _stream(self.device)))

    def _classify_ws(self, n: int, h: int, w: int, sweep: int = 0,
                     need: Optional[int] = None) -> torch.Tensor:
        """The scratch the classify family shares (`need`: bytes asked for by the caller)."""
        if need is None:
            need = int(self._need('milan_classify_workspace_bytes')(self._h, n, h, w, sweep))
        ws = getattr(self, '_cls_ws', None)
        if ws is None or ws.numel() < need:
            self._cls_ws = None  # free before growing
            self._cls_ws = ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def _classify_images(self, images: torch.Tensor) -> torch.Tensor:
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'images must be (n,3,H,W), got {tuple(images.shape)}')
        if images.shape[0] < 1:
            raise ValueError('classify needs at least one image')
        return _dev(images.detach(), self.device, torch.float32)

    def classify(self, images: torch.Tensor, return_logits: bool = True,
                 check: bool = True) -> torch.Tensor:
        """(n,3,H,W) float images, fed as they are (normalised by the caller), through the
        trunk and its `fc` head under the current ablation set: the (n, classes) logits, or
        with `return_logits=False` the (n,) int64 argmax (torch's tie / NaN rule)."""
        fn = self._need('milan_classify')
        images = self._classify_images(images)
        n, _, h, w = images.shape
        ws = self._classify_ws(n, h, w, 0)
        classes = max(1, self.num_classes)
        logits = (torch.empty(n, classes, dtype=torch.float32, device=self.device)
                  if return_logits else None)
        preds = (None if return_logits else
                 torch.empty(n, dtype=torch.int64, device=self.device))

        def run():
            with torch.cuda.device(self.device):
                _check(fn(self._h, images.data_ptr(), n, h, w, _ptr(logits), _ptr(preds),
                          ws.data_ptr(), ws.numel(), _stream(self.device)))
            return logits if return_logits else preds

        return self._guarded('classify', run, check)

    def classify_sweep(self, images: torch.Tensor, pairs,
                       targets: Optional[torch.Tensor] = None, check: bool = True):
        """For every (level, unit) of `pairs` the predictions of `classify` under the current
        set plus that one unit, bit for bit, sharing the forward pass up to the unit's level.
        Returns predictions (len(pairs), n) int64, or with `targets` (n,) the pair
        (predictions, correct) where correct[j] counts predictions[j] == targets."""
        fn = self._need('milan_classify_sweep')
        images = self._classify_images(images)
        n, _, h, w = images.shape
        levels, units, count = self._unit_arrays(pairs)
        preds = torch.empty(count, n, dtype=torch.int64, device=self.device)
        correct = None
        if targets is not None:
            if tuple(targets.shape) != (n,):
                raise ValueError(f'targets shape {tuple(targets.shape)} != {(n,)}')
            targets = _dev(targets, self.device, torch.int64)
            correct = torch.zeros(count, dtype=torch.int32, device=self.device)
        ws = self._classify_ws(n, h, w, max(1, count))

        def run():
            with torch.cuda.device(self.device):
                _check(fn(self._h, images.data_ptr(), n, h, w, levels, units, count,
                          _ptr(targets), _ptr(correct), preds.data_ptr(), ws.data_ptr(),
                          ws.numel(), _stream(self.device)))
            return preds if targets is None else (preds, correct)

        return self._guarded('classify_sweep', run, check)

    def activations(self, images: torch.Tensor, levels, check: bool = True) -> dict:
        """The tensors of the requested edit points under the current ablation set, after
        its masks: {level as given: (n, C, h, w) float32 NCHW}.  `levels`: distinct entries,
        each 0..4 or a name of `ablation_levels`, in any order.  One walk of the trunk up to
        the highest level; no head runs (a state dict without `fc` will do).  Level 0 is the
        raw conv1 output, before bn1 / ReLU / maxpool, on a ResNet; on AlexNet every level
        is relu(conv + bias) x mask."""
        fn = self._need('milan_activations')
        images = self._classify_images(images)
        n, _, h, w = images.shape
        keys = list(levels)
        if not keys:
            raise ValueError('activations needs at least one level')
        idx = []
        for level in keys:
            if isinstance(level, str):
                if level not in self.ablation_levels:
                    raise ValueError(f'layer {level!r} has no native tap; the layers are '
                                     f'{self.ablation_levels}')
                level = self.ablation_levels.index(level)
            idx.append(int(level))
        ws = self._classify_ws(
            n, h, w, need=int(self._need('milan_activations_workspace_bytes')(self._h, n, h, w)))
        shapes = level_shapes(self.dims.trunk_kind, self.dims.trunk_width, h, w)
        # (a level out of range: the library reports it; the shape is a placeholder)
        outs = [torch.empty((n,) + shapes[level] if 0 <= level <= 4 else 1, dtype=torch.float32,
                            device=self.device) for level in idx]
        c_levels = (ctypes.c_int32 * len(idx))(*idx)
        c_outs = (ctypes.c_void_p * len(idx))(*[o.data_ptr() for o in outs])

        def run():
            with torch.cuda.device(self.device):
                _check(fn(self._h, images.data_ptr(), n, h, w, c_levels, len(idx), c_outs,
                          ws.data_ptr(), ws.numel(), _stream(self.device)))
            return dict(zip(keys, outs))

        return self._guarded('activations', run, check)

    def init_state(self, features: torch.Tensor, check: bool = True):
        """(n, k, F) features -> (h, c).  `check` (here and in `step`, `decode`, `lm_score`,
        `lm_logprobs`): read the status word afterwards, as `encode` does (`_guarded`)."""
        n, k, _ = features.shape
        features = _dev(features, self.device, torch.float32)
        h = torch.empty(n, self.dims.hidden_size, device=self.device)
        c = torch.empty_like(h)
        ws = self.workspace(n, k, 0, 1, 1)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_init_state(self._h, features.data_ptr(), n, k,
                                              h.data_ptr(), c.data_ptr(),
                                              ws.data_ptr(), ws.numel(),
                                              _stream(self.device)))
            return h, c

        return self._guarded('init_state', run, check, decoder=True)

    def step(self, features, tokens, h, c, h_lm, c_lm, temperature, check: bool = True):
        rows, k, _ = features.shape
        features = _dev(features, self.device, torch.float32)
        tokens = _dev(tokens, self.device, torch.long)
        h = _dev(h, self.device, torch.float32)
        c = _dev(c, self.device, torch.float32)
        if h_lm is not None:
            h_lm = _dev(h_lm, self.device, torch.float32)
            c_lm = _dev(c_lm, self.device, torch.float32)
        pred = torch.empty(rows, self.dims.vocab_size, device=self.device)
        att = torch.empty(rows, k, device=self.device)
        h2, c2 = torch.empty_like(h), torch.empty_like(c)
        ws = self.workspace(rows, k, 0, 1, 1)

        def run():
            # (the LM state is updated in place: every run starts from the caller's)
            hl = None if h_lm is None else h_lm.clone()
            cl = None if c_lm is None else c_lm.clone()
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_step(self._h, features.data_ptr(), rows, k,
                                        tokens.data_ptr(), h.data_ptr(),
                                        c.data_ptr(), _ptr(hl), _ptr(cl),
                                        float(temperature), pred.data_ptr(),
                                        att.data_ptr(), h2.data_ptr(),
                                        c2.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _stream(self.device)))
            return pred, att, h2, c2, hl, cl

        return self._guarded('step', run, check, decoder=True)

    def _alloc_outputs(self, n, k, strategy, length, beam, want_full,
                       forced=None):
        dev = self.device
        if strategy == FORCED:
            # teacher forcing: `tokens` is the INPUT of milan_decode
            if forced is None or tuple(forced.shape) != (n, length):
                raise ValueError('FORCED decoding needs forced tokens of shape '
                                 f'({n}, {length})')
            tokens = forced.to(device=dev, dtype=torch.long).contiguous().clone()
            want_full = True
        else:
            tokens = torch.empty(n, length, dtype=torch.long, device=dev)
        out = dict(tokens=tokens,
                   scores=torch.empty(n, device=dev),
                   predictions=None,
                   attentions=None,
                   beam_tokens=None,
                   beam_scores=None,
                   out_len=None)
        if strategy in (GREEDY, FORCED):
            if want_full:
                out['predictions'] = torch.empty(n,
                                                 length,
                                                 self.dims.vocab_size,
                                                 device=dev)
                out['attentions'] = torch.empty(n, length, k, device=dev)
        else:
            out['beam_tokens'] = torch.empty(n,
                                             beam,
                                             length,
                                             dtype=torch.long,
                                             device=dev)
            out['beam_scores'] = torch.empty(n, beam, device=dev)
        return out

    def decode(self,
               features: torch.Tensor,
               strategy: int,
               length: int,
               beam: int,
               mi: bool,
               temperature: float,
               group_size: int = 0,
               want_full: bool = True,
               forced: Optional[torch.Tensor] = None,
               check: bool = True):
        n, k, _ = features.shape
        features = _dev(features, self.device, torch.float32)
        if getattr(self, '_graphs', False) and strategy != FORCED:
            # (the status word is read after the replay; an f32 rerun is a call of its own,
            # outside any capture)
            return self._guarded(
                'decode', lambda: self._decode_graphed(features, strategy, length, beam, mi,
                                                       temperature, group_size, want_full),
                check, decoder=True)
        groups = (n + group_size - 1) // group_size if group_size > 0 else 1
        ws = self.workspace(n, k, 0, beam, length)

        def run():
            out = self._alloc_outputs(n, k, strategy, length, beam, want_full,
                                      forced)
            out['out_len'] = torch.full((groups,),
                                        length,
                                        dtype=torch.int32,
                                        device=self.device)
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_decode(
                        self._h, features.data_ptr(), n, k, strategy, length, beam,
                        int(bool(mi)), float(temperature), group_size,
                        out['tokens'].data_ptr(), out['scores'].data_ptr(),
                        _ptr(out['predictions']), _ptr(out['attentions']),
                        _ptr(out['beam_tokens']), _ptr(out['beam_scores']),
                        out['out_len'].data_ptr(), ws.data_ptr(), ws.numel(),
                        _stream(self.device)))
            return out

        return self._guarded('decode', run, check, decoder=True)

    def _decode_graphed(self, features, strategy, length, beam, mi, temperature,
                        group_size, want_full):
        n, k, fsz = features.shape
        sig = (n, k, strategy, length, beam, bool(mi), group_size, want_full)
        groups = (n + group_size - 1) // group_size if group_size > 0 else 1

        def make():
            out = self._alloc_outputs(n, k, strategy, length, beam, want_full)
            out['out_len'] = torch.empty(groups, dtype=torch.int32,
                                         device=self.device)
            out['_features'] = torch.empty(n, k, fsz, device=self.device)
            return out

        cur = torch.cuda.current_stream(self.device)
        gs = self._gstream
        gs.wait_stream(cur)
        with torch.cuda.device(self.device), torch.cuda.stream(gs):
            pool = self._pooled(sig, make)
            ws = self.workspace(n, k, 0, beam, length)
            pool['_features'].copy_(features)
            _check(
                self.lib.milan_decode(
                    self._h, pool['_features'].data_ptr(), n, k, strategy,
                    length, beam, int(bool(mi)), float(temperature), group_size,
                    pool['tokens'].data_ptr(), pool['scores'].data_ptr(),
                    _ptr(pool['predictions']), _ptr(pool['attentions']),
                    _ptr(pool['beam_tokens']), _ptr(pool['beam_scores']),
                    pool['out_len'].data_ptr(), ws.data_ptr(), ws.numel(),
                    gs.cuda_stream))
            out = {key: (v.clone() if isinstance(v, torch.Tensor) else v)
                   for key, v in pool.items() if key != '_features'}
        cur.wait_stream(gs)
        for v in out.values():
            if isinstance(v, torch.Tensor):
                v.record_stream(cur)
        return out

    def lm_score(self, seqs: torch.Tensor, check: bool = True) -> torch.Tensor:
        rows, length = seqs.shape
        seqs = _dev(seqs, self.device, torch.long)
        out = torch.empty(rows, device=self.device)
        ws = self.workspace(rows, 1, 0, 1, 1)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_lm_score(self._h, seqs.data_ptr(), rows, length,
                                            None, out.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _stream(self.device)))
            return out

        return self._guarded('lm_score', run, check, decoder=True)

    def lm_logprobs(self, seqs: torch.Tensor, check: bool = True) -> torch.Tensor:
        """(rows, L) token ids -> (rows, L, V) next-token log-probs."""
        rows, length = seqs.shape
        seqs = _dev(seqs, self.device, torch.long)
        out = torch.empty(rows, length, self.dims.vocab_size,
                          device=self.device)
        ws = self.workspace(rows, 1, 0, 1, 1)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_lm_logprobs(self._h, seqs.data_ptr(), rows,
                                               length, out.data_ptr(),
                                               ws.data_ptr(), ws.numel(),
                                               _stream(self.device)))
            return out

        return self._guarded('lm_logprobs', run, check, decoder=True)

    # -- what the LM and decoder training calls share --
    def _f32_ptrs(self, tensors, expected, what, like=None):
        """`tensors` (`what`: 'LM parameters', 'gradients', ...) as an array
        of pointers, once there are `expected` of them and each is contiguous
        float32 on this device (and shaped as its partner in `like`, when
        given)."""
        if len(tensors) != expected:
            raise ValueError(f'{len(tensors)} {what}, expected {expected}')
        for i, t in enumerate(tensors):
            if (t.device != self.device or t.dtype != torch.float32
                    or not t.is_contiguous()
                    or (like is not None and t.shape != like[i].shape)):
                raise ValueError(
                    f'{what} must be contiguous float32 on {self.device}' +
                    ('' if like is None else ', shaped like the parameters'))
        return (_P * len(tensors))(*[t.data_ptr() for t in tensors])

    def _grad_ptrs(self, params, grads):
        return self._f32_ptrs(grads, len(params), 'gradients', like=params)

    def _check_ids(self, name, ids):
        v = self.dims.vocab_size
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= v):
            raise ValueError(f'{name} hold ids outside [0, {v})')

    def _check_upstream(self, wanted):
        """`wanted`: (upstream gradient or None, the shape it must have)."""
        for t, shape in wanted:
            if t is not None and (tuple(t.shape) != shape
                                  or t.device != self.device
                                  or t.dtype != torch.float32
                                  or not t.is_contiguous()):
                raise ValueError(f'gradient {tuple(t.shape)} must be a '
                                 f'contiguous float32 {shape} on {self.device}')

    def _train_workspace(self, need):
        """The context's training workspace, grown to `need` bytes (0: the
        library refused the shape)."""
        if need == 0:
            _check(ERR_SHAPE)
        ws = getattr(self, '_train_ws', None)
        if ws is None or ws.numel() < need:
            self._train_ws = None
            ws = self._train_ws = torch.empty(need, dtype=torch.uint8,
                                              device=self.device)
        return ws

    # -- LanguageModel training (include/milan_hip.h, milan_lm_train_step) --
    def _lm_train_call(self, params, inputs, targets):
        rows, length = inputs.shape
        if targets.shape != inputs.shape:
            raise ValueError(f'targets {tuple(targets.shape)} != inputs '
                             f'{tuple(inputs.shape)}')
        self._check_ids('inputs', inputs)
        self._check_ids('targets', targets)
        ptrs = self._f32_ptrs(params, 3 + 4 * self.dims.lm_layers,
                              'LM parameters')
        inputs = _dev(inputs, self.device, torch.long)
        targets = _dev(targets, self.device, torch.long)
        ws = self._train_workspace(
            int(self.lib.milan_lm_train_workspace_bytes(self._h, rows,
                                                        length)))
        loss = torch.empty(2, device=self.device)
        return inputs, targets, ptrs, ws, loss

    def lm_nll(self, params, inputs: torch.Tensor,
               targets: torch.Tensor) -> torch.Tensor:
        """NLLLoss(ignore_index=pad) of the LM in eval mode: device tensor
        [sum of -log p over the non-pad targets, their count].  `params`:
        LanguageModel.state_dict() values in order.  Does not synchronise."""
        inputs, targets, ptrs, ws, loss = self._lm_train_call(
            params, inputs, targets)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_lm_nll(self._h, ptrs, len(params),
                                      inputs.data_ptr(), targets.data_ptr(),
                                      inputs.shape[0], inputs.shape[1],
                                      loss.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(self.device)))
        return loss

    def lm_train_step(self, params, grads, inputs: torch.Tensor,
                      targets: torch.Tensor, dropout: float = 0.,
                      seed: int = 0) -> torch.Tensor:
        """Train-mode loss (as `lm_nll`) and the gradient of the mean loss
        with respect to every parameter, OVERWRITTEN into `grads` (same order
        and shapes as `params`).  Does not synchronise."""
        inputs, targets, ptrs, ws, loss = self._lm_train_call(
            params, inputs, targets)
        gptrs = self._grad_ptrs(params, grads)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_lm_train_step(
                    self._h, ptrs, gptrs, len(params), inputs.data_ptr(),
                    targets.data_ptr(), inputs.shape[0], inputs.shape[1],
                    float(dropout), int(seed) & (2**64 - 1), loss.data_ptr(),
                    ws.data_ptr(), ws.numel(), _stream(self.device)))
        return loss

    # -- LanguageModel.forward in training mode (milan_lm_forward_train) --
    def _lm_grad_args(self, params, inputs, targets, check_ids=True):
        for name in PROBED:
            if not hasattr(self.lib, name):
                raise HipUnavailableError(
                    f'the loaded libmilan_hip has no {name}: it was built '
                    'before the differentiable LanguageModel.forward; rebuild '
                    'it (or unset MILAN_LIB)')
        if inputs.dim() != 2:
            raise ValueError('inputs must be (rows, L), got '
                             f'{tuple(inputs.shape)}')
        if targets is not None and targets.shape != inputs.shape:
            raise ValueError(f'targets {tuple(targets.shape)} != inputs '
                             f'{tuple(inputs.shape)}')
        for name, ids in (('inputs', inputs), ('targets', targets)):
            if check_ids and ids is not None:
                self._check_ids(name, ids)  # (the backward takes its forward's)
        ptrs = self._f32_ptrs(params, 3 + 4 * self.dims.lm_layers,
                              'LM parameters')
        inputs = _dev(inputs, self.device, torch.long)
        if targets is not None:
            targets = _dev(targets, self.device, torch.long)
        need = int(self.lib.milan_lm_grad_workspace_bytes(
            self._h, inputs.shape[0], inputs.shape[1]))
        if need == 0:
            _check(ERR_SHAPE)
        return inputs, targets, ptrs, need

    def lm_forward_train(self, params, inputs: torch.Tensor,
                         dropout: float = 0., seed: int = 0,
                         targets: Optional[torch.Tensor] = None,
                         want_logprobs: bool = True):
        """The LM in train mode (milan_lm_forward_train): returns (log-probs
        (rows, L, V) or None, picked (rows, L) or None, workspace).  `targets`
        (rows, L): picked[r, t] = logprobs[r, t, targets[r, t]]; with
        `want_logprobs=False` the (rows, L, V) tensor is never written.  The
        workspace is a fresh uint8 device tensor holding the activations that
        ONE `lm_backward` consumes; it is not `_train_ws`, so other calls on
        this context leave it alone.  Does not synchronise."""
        if targets is None and not want_logprobs:
            raise ValueError('nothing to compute: no targets and no log-probs')
        inputs, targets, ptrs, need = self._lm_grad_args(params, inputs,
                                                         targets)
        rows, length = inputs.shape
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        logprobs = picked = None
        if want_logprobs:
            logprobs = torch.empty(rows, length, self.dims.vocab_size,
                                   device=self.device)
        if targets is not None:
            picked = torch.empty(rows, length, device=self.device)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_lm_forward_train(
                    self._h, ptrs, len(params), inputs.data_ptr(), rows,
                    length, float(dropout), int(seed) & (2**64 - 1),
                    _ptr(logprobs), _ptr(picked), _ptr(targets),
                    ws.data_ptr(), ws.numel(), _stream(self.device)))
        return logprobs, picked, ws

    def lm_backward(self, params, grads, inputs: torch.Tensor, dropout: float,
                    seed: int, dlogprobs: Optional[torch.Tensor],
                    dpicked: Optional[torch.Tensor],
                    targets: Optional[torch.Tensor], ws: torch.Tensor) -> None:
        """Backward of `lm_forward_train` (milan_lm_backward) from upstream
        gradients of its log-probs and picked log-probs (None: zero; not both),
        with the forward's params, inputs, targets, dropout and seed.  The
        gradients of every parameter are OVERWRITTEN into `grads`.  Consumes
        `ws`: a second backward from the same workspace is wrong.  Does not
        synchronise."""
        if dlogprobs is None and dpicked is None:
            raise ValueError('neither dlogprobs nor dpicked given')
        if dpicked is not None and targets is None:
            raise ValueError('dpicked needs the targets of the forward')
        inputs, targets, ptrs, need = self._lm_grad_args(params, inputs,
                                                         targets, False)
        rows, length = inputs.shape
        self._check_upstream(
            ((dlogprobs, (rows, length, self.dims.vocab_size)),
             (dpicked, (rows, length))))
        if ws.numel() < need:
            raise ValueError('workspace does not come from lm_forward_train '
                             'at these dims')
        gptrs = self._grad_ptrs(params, grads)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_lm_backward(
                    self._h, ptrs, gptrs, len(params), inputs.data_ptr(), rows,
                    length, float(dropout), int(seed) & (2**64 - 1),
                    _ptr(dlogprobs), _ptr(dpicked),
                    _ptr(targets) if dpicked is not None else None,
                    ws.data_ptr(), ws.numel(), _stream(self.device)))

    # -- Decoder training (include/milan_hip.h, milan_decoder_train_step) --
    DECODER_TRAIN_PARAMS = 19

    def _decoder_args(self, params, features, targets):
        if features.dim() != 3:
            raise ValueError('features must be (rows, k, feature_size), got '
                             f'{tuple(features.shape)}')
        if targets.dim() != 2 or len(targets) != len(features):
            raise ValueError(f'targets {tuple(targets.shape)} must be (rows, L) '
                             f'for features {tuple(features.shape)}')
        rows, k, f = features.shape
        length = targets.shape[1]
        if f != self.dims.feature_size:
            raise ValueError(f'feature size {f} != the decoder\'s '
                             f'{self.dims.feature_size}')
        self._check_ids('targets', targets)
        ptrs = self._f32_ptrs(params, self.DECODER_TRAIN_PARAMS,
                              'decoder parameters')
        features = _dev(features, self.device, torch.float32)
        targets = _dev(targets, self.device, torch.long)
        return features, targets, ptrs

    def _decoder_train_call(self, params, features, targets):
        features, targets, ptrs = self._decoder_args(params, features,
                                                     targets)
        rows, k, _ = features.shape
        ws = self._train_workspace(
            int(self.lib.milan_decoder_train_workspace_bytes(
                self._h, rows, k, targets.shape[1])))
        loss = torch.empty(3, device=self.device)
        return features, targets, ptrs, ws, loss

    def decoder_nll(self, params, features: torch.Tensor,
                    targets: torch.Tensor) -> torch.Tensor:
        """Teacher-forced decoder in eval mode: device tensor [sum of -log p
        over the non-pad targets, their count, sum of (1 - sum_t alpha)^2].
        `params`: the decoder's 19 own state-dict tensors in the reference's
        order; `features` (rows, k, F); `targets` (rows, L) without <start>.
        Does not synchronise."""
        features, targets, ptrs, ws, loss = self._decoder_train_call(
            params, features, targets)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_decoder_nll(
                    self._h, ptrs, len(params), features.data_ptr(),
                    targets.data_ptr(), features.shape[0], features.shape[1],
                    targets.shape[1], loss.data_ptr(), ws.data_ptr(),
                    ws.numel(), _stream(self.device)))
        return loss

    def decoder_train_step(self, params, grads, features: torch.Tensor,
                           targets: torch.Tensor, dropout: float = 0.,
                           seed: int = 0,
                           regularization_weight: float = 1.) -> torch.Tensor:
        """Train-mode loss terms (as `decoder_nll`) and the gradient of
        [0] / [1] + regularization_weight * [2] / (rows * k) with respect to
        every parameter, OVERWRITTEN into `grads` (same order and shapes as
        `params`).  Does not synchronise."""
        features, targets, ptrs, ws, loss = self._decoder_train_call(
            params, features, targets)
        gptrs = self._grad_ptrs(params, grads)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_decoder_train_step(
                    self._h, ptrs, gptrs, len(params), features.data_ptr(),
                    targets.data_ptr(), features.shape[0], features.shape[1],
                    targets.shape[1], float(dropout), int(seed) & (2**64 - 1),
                    float(regularization_weight), loss.data_ptr(),
                    ws.data_ptr(), ws.numel(), _stream(self.device)))
        return loss

    def decoder_forward_train(self, params, features: torch.Tensor,
                              targets: torch.Tensor, dropout: float = 0.,
                              seed: int = 0):
        """Teacher-forced decoder in train mode (milan_decoder_forward_train):
        returns (log-probs (rows, L, V), attentions (rows, L, k), workspace).
        The workspace is a fresh uint8 device tensor holding the activations
        that ONE `decoder_backward` consumes; it is not `_train_ws`, so other
        calls on this context leave it alone.  Does not synchronise."""
        features, targets, ptrs = self._decoder_args(params, features, targets)
        rows, k, _ = features.shape
        length = targets.shape[1]
        need = int(self.lib.milan_decoder_grad_workspace_bytes(
            self._h, rows, k, length))
        if need == 0:
            _check(ERR_SHAPE)
        ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        logprobs = torch.empty(rows, length, self.dims.vocab_size,
                               device=self.device)
        attentions = torch.empty(rows, length, k, device=self.device)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_decoder_forward_train(
                    self._h, ptrs, len(params), features.data_ptr(),
                    targets.data_ptr(), rows, k, length, float(dropout),
                    int(seed) & (2**64 - 1), logprobs.data_ptr(),
                    attentions.data_ptr(), ws.data_ptr(), ws.numel(),
                    _stream(self.device)))
        return logprobs, attentions, ws

    def decoder_backward(self, params, grads, features: torch.Tensor,
                         targets: torch.Tensor, dropout: float, seed: int,
                         dlogprobs: Optional[torch.Tensor],
                         dattentions: Optional[torch.Tensor],
                         dfeatures: Optional[torch.Tensor],
                         ws: torch.Tensor) -> None:
        """Backward of `decoder_forward_train` (milan_decoder_backward) from
        upstream gradients of its log-probs and attentions (None: zero), with
        the forward's params, features, targets, dropout and seed.  The
        gradients of the 19 parameters are OVERWRITTEN into `grads`, the
        feature gradient into `dfeatures` (None: not computed).  Consumes
        `ws`: a second backward from the same workspace is wrong.  Does not
        synchronise."""
        ptrs = self._f32_ptrs(params, self.DECODER_TRAIN_PARAMS,
                              'decoder parameters')
        rows, k, f = features.shape
        length = targets.shape[1]
        self._check_upstream(
            ((dlogprobs, (rows, length, self.dims.vocab_size)),
             (dattentions, (rows, length, k)), (dfeatures, (rows, k, f))))
        need = int(self.lib.milan_decoder_grad_workspace_bytes(
            self._h, rows, k, length))
        if need == 0 or ws.numel() < need:
            raise ValueError('workspace does not come from decoder_forward_train '
                             'at these dims')
        gptrs = self._grad_ptrs(params, grads)
        with torch.cuda.device(self.device):
            _check(
                self.lib.milan_decoder_backward(
                    self._h, ptrs, gptrs, len(params), features.data_ptr(),
                    targets.data_ptr(), rows, k, length, float(dropout),
                    int(seed) & (2**64 - 1), _ptr(dlogprobs), _ptr(dattentions),
                    _ptr(dfeatures), ws.data_ptr(), ws.numel(),
                    _stream(self.device)))

    def describe(self,
                 images: torch.Tensor,
                 masks: Optional[torch.Tensor],
                 strategy: int,
                 length: int,
                 beam: int,
                 mi: bool,
                 temperature: float,
                 group_size: int = 0,
                 want_full: bool = False,
                 want_features: bool = False,
                 forced: Optional[torch.Tensor] = None,
                 check: bool = True):
        """Fused hot path on (n,k,3,H,W) images (+ (n,k,1,H,W) masks).  `check=False`
        skips the status read (a stream synchronisation) -- the caller then reads
        `status()` itself, as bench.py does once after its timed region."""
        n, k, ch, h, w = images.shape
        idt = DTYPE_U8 if images.dtype == torch.uint8 else DTYPE_F32
        images = _dev(images, self.device,
                      None if idt == DTYPE_U8 else torch.float32)
        mdt = DTYPE_U8
        if masks is not None:
            mdt = DTYPE_U8 if masks.dtype == torch.uint8 else DTYPE_F32
            masks = _dev(masks, self.device,
                         None if mdt == DTYPE_U8 else torch.float32)
        out = self._alloc_outputs(n, k, strategy, length, beam, want_full,
                                  forced)
        groups = (n + group_size - 1) // group_size if group_size > 0 else 1
        out['out_len'] = torch.full((groups,),
                                    length,
                                    dtype=torch.int32,
                                    device=self.device)
        feats = None
        if want_features:
            feats = torch.empty(n,
                                k,
                                self.dims.feature_size,
                                device=self.device)
        out['features'] = feats
        ws = self.workspace(n, k, max(h, w), beam, length)

        def run():
            with torch.cuda.device(self.device):
                _check(
                    self.lib.milan_describe(
                        self._h, images.data_ptr(), idt, _ptr(masks), mdt, n, k, h,
                        w, strategy, length, beam, int(bool(mi)),
                        float(temperature), group_size, _ptr(feats),
                        out['tokens'].data_ptr(), out['scores'].data_ptr(),
                        _ptr(out['predictions']), _ptr(out['attentions']),
                        _ptr(out['beam_tokens']), _ptr(out['beam_scores']),
                        out['out_len'].data_ptr(), ws.data_ptr(), ws.numel(),
                        _stream(self.device)))
            return out

        return self._guarded('describe', run, check)


class _TowerContext:
    """Owns one `milan_<prefix>_ctx` (the weights of one transformer tower model on one GPU)
    and a grow-only workspace.  Subclasses set `_prefix` and add their calls."""

    _prefix = ''

    def __init__(self, dims, state_dict: Dict[str, torch.Tensor], device: torch.device):
        self.lib = load_library()
        if not hasattr(self.lib, f'milan_{self._prefix}_create'):
            raise HipUnavailableError(
                f'this build of libmilan_hip has no milan_{self._prefix}_create')
        self.device = require_device(device)
        self.dims = dims
        self._h = _P()
        with torch.cuda.device(self.device):
            _check(self._fn('create')(ctypes.byref(self._h), self.device.index,
                                      ctypes.byref(dims)))
            keep = []
            for name, tensor in state_dict.items():
                if not tensor.dtype.is_floating_point:
                    continue
                t = _dev(tensor.detach(), self.device, torch.float32)
                keep.append(t)
                shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
                _check(self._fn('set_weight')(self._h, name.encode(), t.data_ptr(), shape,
                                              t.dim()))
            _check(self._fn('finalize_weights')(self._h, _stream(self.device)))
            del keep
        self._ws: Optional[torch.Tensor] = None

    def _fn(self, name: str):
        return getattr(self.lib, f'milan_{self._prefix}_{name}')

    def close(self) -> None:
        if getattr(self, '_h', None):
            self._fn('destroy')(self._h)
            self._h = None
        self._ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def _workspace(self, need: int) -> torch.Tensor:
        if need == 0:
            _check(ERR_ARG)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws


class ClipContext(_TowerContext):
    """Owns one `milan_clip_ctx`: the weights of a ViT CLIP on one GPU and a
    workspace.  Every call computes in exact fp32 on torch's current stream and
    does not synchronise."""

    _prefix = 'clip'

    def encode_images(self, images: torch.Tensor,
                      masks: Optional[torch.Tensor] = None,
                      mask_layers: int = 0, both: bool = False,
                      mul_add: Optional[Sequence[float]] = None) -> torch.Tensor:
        """(n, 3, R, R) [+ (n, 1, R, R) masks] -> L2-normalised (n, embed), or
        (2, n, embed) = (masked, unmasked) when `both`."""
        images = _dev(images, self.device, torch.float32)
        n, res = images.shape[0], images.shape[-1]
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != res:
            raise ValueError(f'images must be (n, 3, R, R), got {tuple(images.shape)}')
        if masks is not None:
            masks = _dev(masks, self.device, torch.float32)
            if masks.numel() != n * res * res:
                raise ValueError(f'masks {tuple(masks.shape)} do not match '
                                 f'images {tuple(images.shape)}')
        e = self.dims.embed_dim
        out = torch.empty((2, n, e) if both else (n, e), device=self.device)
        if n == 0:
            return out
        ma = None if mul_add is None else (_F * 6)(*mul_add)
        with torch.cuda.device(self.device):
            ws = self._workspace(int(self.lib.milan_clip_image_workspace_bytes(
                self._h, n, int(both))))
            _check(self.lib.milan_clip_encode_images(
                self._h, images.data_ptr(), n, res, _ptr(masks), mask_layers,
                int(both), ma, out.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream(self.device)))
        return out

    def encode_texts(self, tokens: torch.Tensor, positions: int) -> torch.Tensor:
        """(rows, context) token ids -> L2-normalised (rows, embed), the towers
        run over the first `positions` positions."""
        tokens = _dev(tokens, self.device, torch.long)
        if tokens.dim() != 2 or tokens.shape[1] != self.dims.context_length:
            raise ValueError(f'tokens must be (rows, {self.dims.context_length}), '
                             f'got {tuple(tokens.shape)}')
        rows = tokens.shape[0]
        out = torch.empty((rows, self.dims.embed_dim), device=self.device)
        if rows == 0:
            return out
        with torch.cuda.device(self.device):
            ws = self._workspace(int(self.lib.milan_clip_text_workspace_bytes(
                self._h, rows, positions)))
            _check(self.lib.milan_clip_encode_texts(
                self._h, tokens.data_ptr(), rows, positions, out.data_ptr(),
                ws.data_ptr(), ws.numel(), _stream(self.device)))
        return out

    def rerank_scores(self, masked: torch.Tensor, unmasked: torch.Tensor,
                      texts: torch.Tensor, neuron_of: Optional[torch.Tensor],
                      candidates: int, lam: float) -> torch.Tensor:
        """masked / unmasked (neurons, k, embed), texts (rows, embed) -> (rows,)."""
        neurons, k, e = masked.shape
        rows = texts.shape[0]
        masked = _dev(masked, self.device, torch.float32)
        unmasked = _dev(unmasked, self.device, torch.float32)
        texts = _dev(texts, self.device, torch.float32)
        if neuron_of is not None:
            neuron_of = _dev(neuron_of, self.device, torch.int32)
        out = torch.empty(rows, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.milan_clip_rerank_scores(
                masked.data_ptr(), unmasked.data_ptr(), texts.data_ptr(),
                _ptr(neuron_of), neurons, k, rows, candidates, e, float(lam),
                out.data_ptr(), _stream(self.device)))
        return out


class BertContext(_TowerContext):
    """Owns one `milan_bert_ctx`: the weights of a BERT-family encoder on one
    GPU and a workspace.  Every call computes in exact fp32 on torch's current
    stream and does not synchronise."""

    _prefix = 'bert'

    def encode(self, ids: torch.Tensor, offsets: torch.Tensor, max_len: int,
               normalize: bool = True,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids (total,) int64 and offsets (n + 1,) int32 of n ragged sentences
        (DEVICE tensors; `max_len` = the longest, known to the host) -> (total,
        width) token embeddings, L2-normalised when `normalize`; written to
        `out` when given."""
        total, n = ids.numel(), offsets.numel() - 1
        if (ids.dtype != torch.long or offsets.dtype != torch.int32 or
                ids.device != self.device or offsets.device != self.device or
                not ids.is_contiguous() or not offsets.is_contiguous()):
            raise ValueError('ids must be int64 and offsets int32, contiguous, '
                             f'on {self.device}')
        if out is None:
            out = torch.empty((total, self.dims.width), device=self.device)
        if (out.shape != (total, self.dims.width) or out.dtype != torch.float32
                or out.device != self.device or not out.is_contiguous()):
            raise ValueError(f'out must be float32 ({total}, {self.dims.width})')
        if n <= 0 or total == 0:
            return out
        with torch.cuda.device(self.device):
            ws = self._workspace(int(self.lib.milan_bert_encode_workspace_bytes(
                self._h, n, total)))
            _check(self.lib.milan_bert_encode(
                self._h, ids.data_ptr(), offsets.data_ptr(), n, total,
                int(max_len), int(normalize), out.data_ptr(), ws.data_ptr(),
                ws.numel(), _stream(self.device)))
        return out

    def score_pairs(self, emb: torch.Tensor, offsets: torch.Tensor,
                    weights: torch.Tensor, cand: torch.Tensor,
                    ref: torch.Tensor) -> torch.Tensor:
        """emb (rows, width) normalised, offsets (n + 1,) int32, weights (rows,),
        cand / ref (pairs,) int32 sentence numbers -> (pairs, 3) = P, R, F."""
        emb = _dev(emb, self.device, torch.float32)
        offsets = _dev(offsets, self.device, torch.int32)
        weights = _dev(weights, self.device, torch.float32)
        cand = _dev(cand, self.device, torch.int32)
        ref = _dev(ref, self.device, torch.int32)
        if (weights.numel() != emb.shape[0] or cand.numel() != ref.numel() or
                emb.shape[1] != self.dims.width):
            raise ValueError('score_pairs: emb / weights / cand / ref disagree')
        pairs = cand.numel()
        out = torch.empty((pairs, 3), device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib.milan_bert_score_pairs(
                emb.data_ptr(), offsets.data_ptr(), weights.data_ptr(),
                cand.data_ptr(), ref.data_ptr(), pairs, offsets.numel() - 1,
                emb.shape[1], out.data_ptr(), _stream(self.device)))
        return out


class VitContext(_TowerContext):
    """Owns one `milan_vit_ctx`: the weights of a DINO-style vision transformer on one GPU
    and a workspace.  Every call computes in exact fp32 on torch's current stream and does
    not synchronise."""

    _prefix = 'vit'

    @property
    def tokens(self) -> int:
        return (self.dims.resolution // self.dims.patch)**2 + 1

    def run(self, images: torch.Tensor, taps: Sequence[int] = (),
            want_output: bool = False):
        """images (n, 3, R, R) -> ({block: (n, tokens, hidden) output of blocks.<block>.mlp.fc1},
        the (n, width) CLS row after the final norm or None).  The walk ends after fc1 of the
        deepest block in `taps` unless `want_output`."""
        d = self.dims
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
            raise ValueError(f'images must be (n, 3, R, R), got {tuple(images.shape)}')
        images = _dev(images.detach(), self.device, torch.float32)
        n = images.shape[0]
        taps = sorted(set(int(t) for t in taps))
        if any(t < 0 or t >= d.layers for t in taps):
            raise ValueError(f'taps {taps} outside the {d.layers} blocks')
        if not taps and not want_output:
            raise ValueError('neither a tap nor the output is asked for')
        outs = {t: torch.empty((n, self.tokens, d.hidden), device=self.device) for t in taps}
        cls = torch.empty((n, d.width), device=self.device) if want_output else None
        if n == 0:
            return outs, cls
        pointers = (_P * d.layers)(*[_ptr(outs.get(l)) for l in range(d.layers)])
        with torch.cuda.device(self.device):
            ws = self._workspace(int(self.lib.milan_vit_workspace_bytes(self._h, n)))
            _check(self.lib.milan_vit_run(self._h, images.data_ptr(), n, images.shape[2],
                                          pointers, _ptr(cls), ws.data_ptr(), ws.numel(),
                                          _stream(self.device)))
        return outs, cls


# channel multipliers (out) of a BigGAN generator's blocks per resolution; block i doubles the
# side from bottom_width << i
_GAN_OUT = {512: (16, 8, 8, 4, 2, 1, 1), 256: (16, 8, 8, 4, 2, 1), 128: (16, 8, 4, 2, 1),
            64: (16, 8, 4, 2), 32: (4, 4, 4)}


def gan_tap_shapes(dims: GanDims):
    """[(channels, side)] of a generator's taps in walk order: layer0, .., layerK, attnK, .."""
    shapes = []
    for i, mult in enumerate(_GAN_OUT[dims.resolution]):
        shapes.append((dims.ch * mult, dims.bottom_width << (i + 1)))
        if dims.attn_resolution == 8 << i:
            shapes.append(shapes[-1])
    return shapes


def gan_image_side(dims: GanDims) -> int:
    """Side of a generator's images: every block doubles bottom_width.  `resolution` names the
    block table; it is the side only at bottom_width 4."""
    return dims.bottom_width << len(_GAN_OUT[dims.resolution])


class GanContext(_TowerContext):
    """Owns one `milan_gan_ctx`: the weights of a BigGAN generator on one GPU (spectral norm
    already folded: `state_dict` holds weight / sv and no u0 / sv0) and a workspace.  Every
    call computes in exact fp32 on torch's current stream and does not synchronise."""

    _prefix = 'gan'

    @property
    def tap_shapes(self):
        """[(channels, side)] of the taps in walk order: layer0, .., layerK, attnK, .."""
        return gan_tap_shapes(self.dims)

    @property
    def image_side(self) -> int:
        """R of the (n, 3, R, R) images."""
        return gan_image_side(self.dims)

    def run(self, z: torch.Tensor, y: torch.Tensor, embedded: bool = False,
            taps: Sequence[int] = (), want_images: bool = False):
        """z (n, dim_z); y: class indices (n,) int64, soft labels (n, n_classes), or with
        `embedded` the embedded classes (n, shared_dim) -> ({tap: (n, C, H, W) output of that
        block}, the (n, 3, R, R) images or None), R = `image_side` = bottom_width << blocks.
        The walk ends after the deepest block in `taps` unless `want_images`."""
        d = self.dims
        if z.dim() != 2 or z.shape[1] != d.dim_z:
            raise ValueError(f'z must be (n, {d.dim_z}), got {tuple(z.shape)}')
        n = z.shape[0]
        z = _dev(z.detach(), self.device, torch.float32)
        classes = None
        if y.dim() == 1 and not embedded:
            if y.shape[0] != n or y.dtype.is_floating_point:
                raise ValueError(f'y must be ({n},) class indices, got {tuple(y.shape)} '
                                 f'{y.dtype}')
            classes = _dev(y.detach(), self.device, torch.int64)
            if n and bool(((classes < 0) | (classes >= d.n_classes)).any()):
                raise IndexError(f'class index outside 0 .. {d.n_classes - 1}')
            y = None
        else:
            columns = d.shared_dim if embedded else d.n_classes
            if y.dim() != 2 or y.shape[0] != n or y.shape[1] != columns:
                raise ValueError(f'y must be ({n}, {columns}), got {tuple(y.shape)}')
            y = _dev(y.detach(), self.device, torch.float32)
        shapes = self.tap_shapes
        taps = sorted(set(int(t) for t in taps))
        if any(t < 0 or t >= len(shapes) for t in taps):
            raise ValueError(f'taps {taps} outside the {len(shapes)} taps')
        if not taps and not want_images:
            raise ValueError('neither a tap nor the images are asked for')
        outs = {t: torch.empty((n, shapes[t][0], shapes[t][1], shapes[t][1]), device=self.device)
                for t in taps}
        side = self.image_side
        images = torch.empty((n, 3, side, side), device=self.device) if want_images else None
        if n == 0:
            return outs, images
        pointers = (_P * len(shapes))(*[_ptr(outs.get(t)) for t in range(len(shapes))])
        with torch.cuda.device(self.device):
            ws = self._workspace(int(self.lib.milan_gan_workspace_bytes(self._h, n)))
            _check(self.lib.milan_gan_run(self._h, z.data_ptr(), _ptr(classes), _ptr(y),
                                          int(embedded), n, pointers, _ptr(images),
                                          ws.data_ptr(), ws.numel(), _stream(self.device)))
        return outs, images


def attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(head)) v per (sequence, head) by the streaming fp32-MFMA kernel
    (milan_attention).  qkv (seqs, T, 3 * width) float32 on the GPU: q | k | v, the heads
    contiguous inside each; returns (seqs, T, width).  Any T >= 1; head = width / heads a
    multiple of 16 up to 128, anything else raises ValueError."""
    device = require_device(qkv.device)
    if qkv.dim() != 3 or qkv.shape[1] < 1 or qkv.shape[2] % 3 or heads < 1:
        raise ValueError(f'qkv must be (seqs, T >= 1, 3 * width), got {tuple(qkv.shape)}')
    qkv = _dev(qkv.detach(), device, torch.float32)
    seqs, tokens, width = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    out = torch.empty((seqs, tokens, width), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _check(_need_export('milan_attention')(qkv.data_ptr(), out.data_ptr(), seqs, tokens,
                                               width, int(heads), _stream(device)))
    return out


def sagan_attention(theta: torch.Tensor, phi_g: torch.Tensor, height: int,
                    width: int) -> torch.Tensor:
    """The attention of a BigGAN / SAGAN non-local block by the streaming fp32-MFMA kernel
    (milan_sagan_attention): out_i = sum_j softmax_j(theta_i . phi_j) g_j, no scale factor,
    without the (height * width) x (height * width / 4) scores ever reaching memory.

    Pixel-major, float32, on the GPU.  theta (n, height * width, dk): the queries; a column
    slice of a wider tensor (the first dk columns of a fused theta | phi | g conv output) is
    read in place.  phi_g (n, height * width / 4, dk + dv): the 2 x 2 max-pooled keys | values.
    Returns (n, height * width, dv).  With C the block's channel count, dk = C / 8 and dv =
    C / 2; C a multiple of 32 up to 384 and even height and width, anything else raises
    ValueError."""
    device = require_device(theta.device)
    if theta.dim() != 3 or phi_g.dim() != 3 or phi_g.shape[0] != theta.shape[0]:
        raise ValueError(f'theta must be (n, H W, dk) and phi_g (n, H W / 4, dk + dv), got '
                         f'{tuple(theta.shape)} and {tuple(phi_g.shape)}')
    n, dk = theta.shape[0], theta.shape[2]
    channels = 8 * dk
    if phi_g.shape[2] != 5 * dk:
        raise ValueError(f'phi_g has {phi_g.shape[2]} columns: with dk = {dk} query columns '
                         f'(C = {channels}) it needs dk + dv = {5 * dk}')
    if theta.shape[1] != height * width or phi_g.shape[1] * 4 != theta.shape[1]:
        raise ValueError(f'{theta.shape[1]} queries and {phi_g.shape[1]} keys are not '
                         f'height x width = {height} x {width} and a quarter of it')
    theta = theta.detach()
    if (theta.dtype != torch.float32 or theta.stride(2) != 1 or n > 1 and
            theta.stride(0) != theta.shape[1] * theta.stride(1) or theta.stride(1) % 2 or
            theta.stride(1) < dk or theta.data_ptr() % 8):
        theta = theta.to(torch.float32).contiguous()
    phi_g = _dev(phi_g.detach(), device, torch.float32)
    out = torch.empty((n, height * width, 4 * dk), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _check(_need_export('milan_sagan_attention')(
            theta.data_ptr(), theta.stride(1), phi_g.data_ptr(), out.data_ptr(), n, int(height),
            int(width), channels, _stream(device)))
    return out


def profile_enable(enable: bool) -> None:
    _check(load_library().milan_profile_enable(int(enable)))


def profile_read():
    """-> (gemm_ms, gemm_flops, gemm_launches) since profile_enable(True)."""
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_longlong()
    _check(load_library().milan_profile_read(ctypes.byref(ms), ctypes.byref(fl),
                                             ctypes.byref(n)))
    return ms.value, fl.value, n.value


STAGES = ('other', 'enc_input', 'enc_stem', 'enc_stem_tail', 'enc_layer1',
          'enc_layer2', 'enc_layer3', 'enc_layer4', 'enc_pool', 'dec_init',
          'dec_search', 'dec_lm')  # enum milan_stage


def profile_read_stages() -> Dict[str, Dict[str, float]]:
    """Per-stage HIP-event timings since profile_enable(True): region ms and
    count, plus the GEMM ms / algorithmic FLOPs / launches / algorithmic HBM
    bytes inside the stage."""
    table = (ctypes.c_double * (len(STAGES) * 6))()
    _check(load_library().milan_profile_read_stages(table))
    keys = ('region_ms', 'regions', 'gemm_ms', 'gemm_flops', 'gemm_launches',
            'gemm_bytes')
    return {name: dict(zip(keys, table[i * 6:i * 6 + 6]))
            for i, name in enumerate(STAGES)}


def profile_read_kernels() -> Dict[str, Dict[str, float]]:
    """The same records by kernel family (enum milan_kernel_family): summed launch ms,
    algorithmic FLOPs, launches, algorithmic HBM bytes."""
    table = (ctypes.c_double * (len(KERNEL_FAMILIES) * 4))()
    _check(load_library().milan_profile_read_kernels(table))
    keys = ('ms', 'flops', 'launches', 'bytes')
    return {name: dict(zip(keys, table[i * 4:i * 4 + 4]))
            for i, name in enumerate(KERNEL_FAMILIES)}


def conv2d_nhwc(x: torch.Tensor,
                weight: torch.Tensor,
                bias: Optional[torch.Tensor] = None,
                stride: int = 1,
                padding: int = 0,
                relu: bool = False,
                residual: Optional[torch.Tensor] = None,
                precision: str = 'f32',
                lib: Optional[ctypes.CDLL] = None) -> torch.Tensor:
    """Test hook for the implicit-GEMM kernel (milan_conv2d_nhwc); `lib`: another
    loaded build of the library (load_library(EXP_LIB_PATH)) instead of the default."""
    lib = lib if lib is not None else load_library()
    device = require_device(x.device)
    n, h, w, cin = x.shape
    cout, cin_w, kh, kw = weight.shape
    assert cin_w == cin
    ho = (h + 2 * padding - kh) // stride + 1
    wo = (w + 2 * padding - kw) // stride + 1
    y = torch.empty(n, ho, wo, cout, device=device)
    x, weight = x.contiguous(), weight.contiguous()
    with torch.cuda.device(device):
        _check(
            lib.milan_conv2d_nhwc(x.data_ptr(), n, h, w, cin,
                                  weight.data_ptr(), _ptr(bias), cout, kh, kw,
                                  stride, padding, int(relu), _ptr(residual),
                                  y.data_ptr(), _CONV_PRECISIONS[precision],
                                  _stream(device)))
    return y


class GemmProbeArgs(ctypes.Structure):
    """`milan_gemm_probe_args` (include/milan_hip.h)."""
    POINTERS = ('A', 'A2', 'aux', 'C', 'weight', 'bias', 'm_live', 'row_list', 'status')
    _fields_ = ([(name, ctypes.c_void_p) for name in POINTERS] +
                [(name, ctypes.c_int64) for name in (
                    'a_pix_stride', 'a_img_stride', 'a2_pix_stride', 'a2_img_stride',
                    'a_grp', 'bias_grp', 'c_grp', 'aux_grp')] +
                [(name, ctypes.c_int32) for name in (
                    'M', 'N', 'K', 'ldc', 'ldaux',
                    'H', 'Wd', 'Cin', 'Ho', 'Wo', 'KH', 'KW', 'stride', 'pad',
                    'aniso', 'stride_w', 'pad_w',
                    'epilogue', 'a_split', 'out_split', 'aux_split', 'f16',
                    'K1', 'H2', 'W2d', 'stride2',
                    'm_live_mul', 'groups', 'tap_ncls', 'no_wt')])


def gemm_probe(device=None, **fields) -> None:
    """Test hook: one launch of the implicit GEMM with every launcher argument given
    (milan_gemm_probe).  `fields` are the members of `milan_gemm_probe_args`; a pointer is a
    GPU tensor, a device address (an int: a tensor's data_ptr() plus a byte offset, to place an
    operand inside a wider buffer) or None.  The buffers, their formats and their sizes are the
    caller's; nothing is allocated or checked here.  Synchronises.  A launch the library's plan
    refuses raises ValueError with the plan's text."""
    fn = _need_export('milan_gemm_probe')
    args = GemmProbeArgs()
    known = {name for name, _ in GemmProbeArgs._fields_}
    for name, value in fields.items():
        if name not in known:
            raise TypeError(f'gemm_probe: no field {name!r} in milan_gemm_probe_args')
        if name in GemmProbeArgs.POINTERS:
            if isinstance(value, torch.Tensor):
                device = device if device is not None else value.device
                value = value.data_ptr()
            setattr(args, name, value)
        else:
            setattr(args, name, int(value))
    device = require_device(device if device is not None else 'cuda')
    with torch.cuda.device(device):
        _check(fn(ctypes.byref(args), _stream(device)))


def beam_merge(cand_v: torch.Tensor,
               cand_i: torch.Tensor,
               last_lp: Optional[torch.Tensor] = None,
               wide: bool = False,
               lib: Optional[ctypes.CDLL] = None):
    """One merge step of the beam search (milan_beam_merge): per neuron the `beam`
    best of cand_v[n, p, j] + last_lp[n, p].  cand_v (n, beam_prev, beam) float32 with
    every list sorted descending, cand_i the same shape int32, last_lp (n, beam_prev)
    or None (zeros).  Returns (new_lp, new_tok, new_bp), each (n, beam).  `wide`: the
    wide kernel whatever the beam (default: the kernel `Context.decode` runs)."""
    lib = lib if lib is not None else load_library()
    if not hasattr(lib, 'milan_beam_merge'):
        raise HipUnavailableError('this build of libmilan_hip has no milan_beam_merge')
    device = require_device(cand_v.device)
    n, beam_prev, beam = cand_v.shape
    if tuple(cand_i.shape) != (n, beam_prev, beam):
        raise ValueError(f'cand_i shape {tuple(cand_i.shape)} != {(n, beam_prev, beam)}')
    if last_lp is not None and tuple(last_lp.shape) != (n, beam_prev):
        raise ValueError(f'last_lp shape {tuple(last_lp.shape)} != {(n, beam_prev)}')
    cand_v = _dev(cand_v, device, torch.float32)
    cand_i = _dev(cand_i, device, torch.int32)
    if last_lp is not None:
        last_lp = _dev(last_lp, device, torch.float32)
    new_lp = torch.empty(n, beam, device=device)
    new_tok = torch.empty(n, beam, dtype=torch.int32, device=device)
    new_bp = torch.empty(n, beam, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(
            lib.milan_beam_merge(cand_v.data_ptr(), cand_i.data_ptr(), _ptr(last_lp),
                                 n, beam_prev, beam, int(bool(wide)),
                                 new_lp.data_ptr(), new_tok.data_ptr(),
                                 new_bp.data_ptr(), None, 0, _stream(device)))
    return new_lp, new_tok, new_bp


ROW_SELECT_PATHS = {'auto': 0, 'wide': 1, 'threshold': 2, 'legacy': 3}


def row_select(logits: torch.Tensor,
               k: int,
               lm_logits: Optional[torch.Tensor] = None,
               lam: float = 0.,
               last_tok: Optional[torch.Tensor] = None,
               stop: int = 0,
               path: str = 'auto',
               lib: Optional[ctypes.CDLL] = None):
    """One per-row top-k of the beam search (milan_row_select): per row the `k` best of
    log_softmax(logits) - lam * log_softmax(lm_logits), logits (rows, V) float32.  A row
    with last_tok[row] == stop gets the forced candidates of a finished beam.  Returns
    (cand_v, cand_i), each (rows, k), sorted by (value descending, index ascending).
    `path`: 'auto' (the kernel `Context.decode` runs), 'wide', 'threshold' or 'legacy';
    a shape the path does not take raises ValueError.  Every path gives the same bits."""
    lib = lib if lib is not None else load_library()
    if not hasattr(lib, 'milan_row_select'):
        raise HipUnavailableError('this build of libmilan_hip has no milan_row_select')
    device = require_device(logits.device)
    rows, V = logits.shape
    if lm_logits is not None and tuple(lm_logits.shape) != (rows, V):
        raise ValueError(f'lm_logits shape {tuple(lm_logits.shape)} != {(rows, V)}')
    if last_tok is not None and tuple(last_tok.shape) != (rows,):
        raise ValueError(f'last_tok shape {tuple(last_tok.shape)} != {(rows,)}')
    logits = _dev(logits, device, torch.float32)
    if lm_logits is not None:
        lm_logits = _dev(lm_logits, device, torch.float32)
    if last_tok is not None:
        last_tok = _dev(last_tok, device, torch.int64)
    cand_v = torch.empty(rows, k, device=device)
    cand_i = torch.empty(rows, k, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(
            lib.milan_row_select(logits.data_ptr(), _ptr(lm_logits), float(lam), rows, V,
                                 int(k), _ptr(last_tok), int(stop), cand_v.data_ptr(),
                                 cand_i.data_ptr(), ROW_SELECT_PATHS[path],
                                 _stream(device)))
    return cand_v, cand_i


# -- the Linear kernel of the AlexNet head on caller-supplied operands -----------------------
def _need_export(name: str):
    lib = load_library()
    if not hasattr(lib, name):
        raise HipUnavailableError(f'this build of libmilan_hip has no {name}')
    return getattr(lib, name)


def _linear_args(x, bias, n_in, n_out, device):
    x = _dev(x.detach(), device, torch.float32)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != n_in:
        raise ValueError(f'x must be (rows >= 1, {n_in}), got {tuple(x.shape)}')
    if bias is not None:
        bias = _dev(bias.detach(), device, torch.float32)
        if tuple(bias.shape) != (n_out,):
            raise ValueError(f'bias must be ({n_out},), got {tuple(bias.shape)}')
    return x, bias, torch.empty(x.shape[0], n_out, dtype=torch.float32, device=device)


def linear_pack(weight: torch.Tensor):
    """The packed copy of a GPU (n_out, n_in) weight that `linear` reads, made once per
    weight: (packed, n_out, n_in)."""
    device = require_device(weight.device)
    weight = _dev(weight.detach(), device, torch.float32)
    if weight.dim() != 2 or min(weight.shape) < 1:
        raise ValueError(f'weight must be (n_out, n_in), got {tuple(weight.shape)}')
    n_out, n_in = weight.shape
    nbytes = int(_need_export('milan_linear_packed_bytes')(n_out, n_in))
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _check(_need_export('milan_linear_pack')(weight.data_ptr(), n_out, n_in,
                                                 packed.data_ptr(), _stream(device)))
    return packed, n_out, n_in


def linear(x: torch.Tensor, packed, bias: Optional[torch.Tensor] = None,
           relu: bool = False) -> torch.Tensor:
    """act(x W^T + bias) by the fp32-MFMA kernel of the AlexNet head; `packed` from
    `linear_pack`.  A row's bits depend on neither the other rows nor their number."""
    weight, n_out, n_in = packed
    device = weight.device
    x, bias, y = _linear_args(x, bias, n_in, n_out, device)
    with torch.cuda.device(device):
        _check(_need_export('milan_linear')(x.data_ptr(), weight.data_ptr(), _ptr(bias),
                                            x.shape[0], n_in, n_out, int(relu), y.data_ptr(),
                                            _stream(device)))
    return y


def linear_rowwise(x: torch.Tensor, weight: torch.Tensor,
                   bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x W^T + bias by the ResNet head's kernel, one wavefront per output and row: the
    baseline `tools/bench_alexnet.py` measures `linear` against."""
    device = require_device(weight.device)
    weight = _dev(weight.detach(), device, torch.float32)
    n_out, n_in = weight.shape
    x, bias, y = _linear_args(x, bias, n_in, n_out, device)
    with torch.cuda.device(device):
        _check(_need_export('milan_linear_rowwise')(x.data_ptr(), weight.data_ptr(), _ptr(bias),
                                                    x.shape[0], n_in, n_out, y.data_ptr(),
                                                    _stream(device)))
    return y


def lrn(x: torch.Tensor, local_size: int, alpha: float, beta: float,
        split: bool = False) -> torch.Tensor:
    """The across-channel LRN kernel alone on a device tensor (pixels, channels) with a
    pixel's channels contiguous: fp32, or with `split` the split-f16 groups at scale 1 (a
    float32 tensor of the same shape that holds them), in and out."""
    device = require_device(x.device)
    x = _dev(x.detach(), device, torch.float32)
    if x.dim() != 2:
        raise ValueError(f'lrn takes (pixels, channels), got {tuple(x.shape)}')
    y = torch.empty_like(x)
    with torch.cuda.device(device):
        _check(_need_export('milan_lrn')(x.data_ptr(), x.shape[0], x.shape[1], int(split),
                                         int(local_size), float(alpha), float(beta),
                                         y.data_ptr(), None, _stream(device)))
    return y


def vgg_level_names(blocks: Sequence[int]) -> Tuple[str, ...]:
    """torchvision's names of the last conv of each VGG block: `features.N` with a ReLU
    behind every conv and a pool behind every block ((2, 2, 3, 3, 3) -> features.2 / 7 / 14 /
    21 / 28, the reference's LAYERS.VGG16)."""
    names, at = [], 0
    for count in blocks:
        names.append(f'features.{at + 2 * (count - 1)}')
        at += 2 * count + 1
    return tuple(names)


def make_dims(state_dict: Dict[str, torch.Tensor],
              n_vocab_tokens: int,
              blocks: Sequence[int] = (3, 4, 23, 3)) -> Dims:
    """Derive `milan_dims` from a reference state dict + vocabulary size."""
    d = Dims()
    sd = state_dict
    pre = 'encoder.encoder.model.'
    width = kind = None
    if pre + 'features.0.weight' in sd:  # 'alexnet' config
        kind, width = TRUNK_ALEXNET, sd[pre + 'features.0.weight'].shape[0]
    elif pre + 'vgg.1.0.weight' in sd:  # a VGG, its `features.N` renamed to `vgg.B.J`
        kind, width = TRUNK_VGG, sd[pre + 'vgg.1.0.weight'].shape[0]
    elif pre + 'conv5.weight' in sd:  # the Places365 AlexNet (conv1..conv5 by name)
        kind = TRUNK_ALEXNET_PLACES
        if sd[pre + 'conv1.weight'].shape[0] % 3:
            raise ValueError('conv1 of the Places365 AlexNet has 3 x width channels')
        width = sd[pre + 'conv1.weight'].shape[0] // 3
    elif pre + 'conv1.weight' in sd:
        width = sd[pre + 'conv1.weight'].shape[0]
        kind = (TRUNK_BOTTLENECK if pre + 'layer1.0.conv3.weight' in sd else
                TRUNK_BASIC)
    if 'lstm.weight_hh' in sd:
        hidden = sd['lstm.weight_hh'].shape[1]
        emb = sd['embedding.weight'].shape[1]
        feat = sd['lstm.weight_ih'].shape[1] - emb
        att = sd['attend.query_to_hidden.weight'].shape[0]
        vocab = sd['output.1.weight'].shape[0]
    else:
        hidden, emb, att, vocab = 4, 4, 4, n_vocab_tokens + 4
        # encoder-only context, or a standalone LanguageModel (no trunk either)
        feat = _FEATURE_MULT[kind] * width if kind is not None else 4
    if width is None:
        # decoder-only context (foreign Encoder, like the reference accepts any
        # `feature_shape`): no trunk, feature size only GEMM-aligned
        if feat % 4:
            raise ValueError(f'feature size {feat} must be a multiple of 4')
        kind, width = TRUNK_NONE, 0
    d.trunk_kind = kind
    if vocab != n_vocab_tokens + 4:
        raise ValueError(
            f'output layer has {vocab} classes but the indexer has '
            f'{n_vocab_tokens} tokens + 4 specials')
    d.trunk_width = width
    for i, b in enumerate(blocks):
        d.trunk_blocks[i] = b
    d.feature_size, d.hidden_size, d.embedding_size = feat, hidden, emb
    d.attention_size, d.vocab_size = att, vocab
    d.start_index = n_vocab_tokens
    d.stop_index = n_vocab_tokens + 1
    d.pad_index = n_vocab_tokens + 2
    d.has_lm = int('lm.lstm.weight_hh_l0' in sd)
    if d.has_lm:
        d.lm_hidden_size = sd['lm.lstm.weight_hh_l0'].shape[1]
        d.lm_embedding_size = sd['lm.embedding.weight'].shape[1]
        layers = 0
        while f'lm.lstm.weight_hh_l{layers}' in sd:
            layers += 1
        d.lm_layers = layers
    return d
