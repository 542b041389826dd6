"""tests/bertref.py's encoder in float64 against `transformers.BertModel` and
`transformers.RobertaModel` built offline from a config: random weights, no
pooler, dropout 0, the layer list cut to num_layers, ragged sentences padded
with an attention mask.  Agreement at float64 round-off on the real tokens pins
the post-LN order, the erf GELU, RoBERTa's position offset, the token-type row
and the eps from the config.
"""
import pathlib
import sys

import pytest
import torch

import bertref

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
sys.path.insert(0, str(GOLDEN))
import bert_standin  # noqa: E402


def hf_model(kind, cfg, sd):
    transformers = pytest.importorskip('transformers')
    special = bert_standin.ids_of(cfg)
    common = dict(vocab_size=len(bert_standin.vocab(cfg)), hidden_size=cfg['width'],
                  num_hidden_layers=cfg['layers'], num_attention_heads=cfg['heads'],
                  intermediate_size=cfg['intermediate'],
                  max_position_embeddings=cfg['max_positions'],
                  type_vocab_size=cfg['type_vocab'], layer_norm_eps=cfg['eps'],
                  hidden_act='gelu', hidden_dropout_prob=0., attention_probs_dropout_prob=0.,
                  pad_token_id=special['pad_id'])
    if kind == 'roberta':
        model = transformers.RobertaModel(transformers.RobertaConfig(**common),
                                          add_pooling_layer=False)
    else:
        model = transformers.BertModel(transformers.BertConfig(**common),
                                       add_pooling_layer=False)
    own = {k: v for k, v in bert_standin.strip(sd).items() if not k.startswith('pooler.')}
    result = model.load_state_dict(own, strict=False)
    assert not result.unexpected_keys, result
    assert all('position_ids' in k or 'token_type_ids' in k for k in result.missing_keys), result
    model.encoder.layer = model.encoder.layer[:cfg['num_layers']]
    return model.double().eval()


@pytest.mark.parametrize('kind', ['bert', 'roberta'])
def test_tower_matches_transformers_on_ragged_sentences(kind):
    cfg = bert_standin.CONFIGS[kind]
    sd = bert_standin.state_dict(cfg, seed=5)
    model = hf_model(kind, cfg, sd)
    tok = bert_standin.tokenizer(cfg)
    special = bert_standin.ids_of(cfg)
    g = torch.Generator().manual_seed(3)
    sents = bert_standin.sentences(g, 7, 14) + ['dog']
    ids = [tok.encode(s).ids for s in sents] + [[special['cls_id'], special['sep_id']]]
    assert len({len(i) for i in ids}) > 3
    longest = max(len(i) for i in ids)
    padded = torch.full((len(ids), longest), special['pad_id'], dtype=torch.long)
    mask = torch.zeros(len(ids), longest, dtype=torch.long)
    for row, i in enumerate(ids):
        padded[row, :len(i)] = torch.tensor(i)
        mask[row, :len(i)] = 1
    with torch.no_grad():
        want = model(input_ids=padded, attention_mask=mask).last_hidden_state
    got = bertref.encode(bertref.cast(bert_standin.strip(sd), torch.float64), ids,
                         **bert_standin.ref_cfg(cfg))
    worst = 0.
    for row, emb in enumerate(got):
        assert emb.dtype == torch.float64 and emb.shape == (len(ids[row]), cfg['width'])
        worst = max(worst, (emb - want[row, :len(ids[row])]).abs().max().item())
    print(kind, 'max |bertref - transformers| in float64', worst)
    assert worst < 1e-12


def test_cutting_the_layers_matters():
    """The golden models run one layer fewer than they hold: the cut is visible."""
    cfg = bert_standin.CONFIGS['bert']
    sd = bertref.cast(bert_standin.strip(bert_standin.state_dict(cfg, seed=5)), torch.float64)
    rc = bert_standin.ref_cfg(cfg)
    ids = [2, 7, 9, 11, 3]
    cut = bertref.encode_one(sd, ids, **rc)
    full = bertref.encode_one(sd, ids, **dict(rc, num_layers=cfg['layers']))
    assert (cut - full).abs().max() > 1e-3
