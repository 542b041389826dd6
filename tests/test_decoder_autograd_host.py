"""Host-side pieces of the differentiable training-mode forward (no GPU): the
C ABI of milan_decoder_forward_train / milan_decoder_backward as the binding
declares it, and the training-mode argument rules of `Decoder.forward`."""
import re

import pytest
import torch

from conftest import REPO
from milan_amd import decoders, encoders, hip, lang, lms, synthetic

NEW_CALLS = ('milan_decoder_grad_workspace_bytes', 'milan_decoder_forward_train',
             'milan_decoder_backward')


class IdentityEncoder(encoders.Encoder):
    def __init__(self, feature_size):
        super().__init__()
        self.feature_shape = (feature_size,)

    def forward(self, images, masks=None, **_):
        return images.reshape(len(images), -1)

    def properties(self):
        return {'feature_size': self.feature_shape[0]}


def make_decoder(lm=False):
    idx = lang.Indexer(lang.Vocab(synthetic.vocab_tokens(20)), str.split, True, True,
                       True, True)
    model = lms.LanguageModel(idx, 8, 16, layers=1, dropout=0.) if lm else None
    return decoders.Decoder(idx, IdentityEncoder(12), model, embedding_size=8,
                            hidden_size=16, length=5, dropout=.5)


def test_abi_11_declares_the_autograd_pair():
    assert hip.ABI_VERSION == 11
    header = (REPO / 'include' / 'milan_hip.h').read_text()
    for name in NEW_CALLS:
        proto = re.search(r'\b' + name + r'\(([^;]*)\);', header)
        assert proto, name
        n_args = len(proto.group(1).split(','))
        assert len(hip.SIGNATURES[name][1]) == n_args, name
    # the same leading parameter list as milan_decoder_train_step
    fwd, bwd = (hip.SIGNATURES[n][1] for n in NEW_CALLS[1:])
    step = hip.SIGNATURES['milan_decoder_train_step'][1]
    assert bwd[:11] == step[:11] and fwd[:8] == [step[0], step[1]] + step[3:9]


def test_training_teacher_forcing_reaches_the_hip_path():
    model = make_decoder()
    model.train()
    feats = torch.rand(2, 3, 12)
    targets = torch.randint(0, 20, (2, 5))
    # no NotImplementedError any more: the HIP path is taken, and a CPU model has
    # no CPU fallback
    with pytest.raises(hip.HipUnavailableError):
        model(feats, strategy=targets, mi=False)


def test_training_mode_decoding_strategies_still_raise():
    model = make_decoder()
    model.train()
    feats = torch.rand(2, 3, 12)
    for strategy in ('greedy', 'sample', 'beam'):
        with pytest.raises(NotImplementedError):
            model(feats, strategy=strategy, mi=False)


def test_training_mode_mi_and_rerank_still_raise():
    model = make_decoder(lm=True)
    model.train()
    feats = torch.rand(2, 3, 12)
    targets = torch.randint(0, 20, (2, 5))
    with pytest.raises(ValueError, match='while training'):
        model(feats, strategy=targets, mi=True)
    with pytest.raises(ValueError, match='while training'):
        model(feats, strategy='rerank')
    with pytest.raises(ValueError, match='length'):  # argument checks come first
        model(feats, strategy=targets[:, :3], mi=False)
