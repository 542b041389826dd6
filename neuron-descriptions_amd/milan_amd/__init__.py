"""MI355X-native MILAN inference path (drop-in for `src.milan`).

    from milan_amd import pretrained, Decoder
    decoder = pretrained('base').to('cuda')
    captions = decoder.predict(dataset, strategy='rerank', temperature=.2,
                               beam_size=50, device='cuda')
"""
from milan_amd import ablations, classifiers, generators, vits
from milan_amd.ablations import ImageClassifier
from milan_amd.classifiers import ResNetClassifier
from milan_amd.decoders import (STRATEGIES, STRATEGY_BEAM, STRATEGY_GREEDY,
                                STRATEGY_RERANK, STRATEGY_SAMPLE, Decoder,
                                DecoderOutput, DecoderState, DecoderStep,
                                DecoderWithCLIP, decoder)
from milan_amd.encoders import Encoder, PyramidConvEncoder, encoder
from milan_amd.lms import LanguageModel
from milan_amd.loaders import pretrained, pretrained_sharded
from milan_amd.rerankers import (CLIPWithMasks, CLIPWithMasksReranker,
                                 RerankerOutput, reranker)

__all__ = [
    'ablations', 'classifiers', 'generators', 'vits', 'ImageClassifier',
    'ResNetClassifier',
    'Decoder', 'DecoderOutput', 'DecoderState', 'DecoderStep',
    'DecoderWithCLIP', 'CLIPWithMasks', 'CLIPWithMasksReranker',
    'RerankerOutput', 'reranker', 'Encoder',
    'PyramidConvEncoder', 'LanguageModel', 'decoder', 'encoder', 'pretrained',
    'pretrained_sharded',
    'STRATEGIES', 'STRATEGY_BEAM', 'STRATEGY_GREEDY', 'STRATEGY_RERANK',
    'STRATEGY_SAMPLE'
]
