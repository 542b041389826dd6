"""Small stand-ins for the BERTScore goldens and tests: a BERT-shaped and a
RoBERTa-shaped encoder with seeded random weights under their HuggingFace
state-dict names (model prefix included), and a word-level tokenizer built with
the `tokenizers` package.  No checkpoint, nothing fetched.
"""
import torch

WORDS = ('a', 'the', 'dog', 'sky', 'blue', 'red', 'grass', 'tree', 'edge', 'of', 'and',
         'stripes', 'round', 'things', 'water', 'face', 'animal', 'fur', 'green', 'text',
         'lines', 'top', 'buildings', 'wheels', 'eyes', 'plants')

CONFIGS = {
    'bert': dict(model_type='bert', specials=('[PAD]', '[UNK]', '[CLS]', '[SEP]'), cls='[CLS]',
                 sep='[SEP]', pad='[PAD]', unk='[UNK]', width=48, heads=3, layers=4,
                 num_layers=3, intermediate=64, max_positions=40, type_vocab=2, eps=1e-12),
    'roberta': dict(model_type='roberta', specials=('<s>', '<pad>', '</s>', '<unk>'), cls='<s>',
                    sep='</s>', pad='<pad>', unk='<unk>', width=48, heads=4, layers=3,
                    num_layers=2, intermediate=80, max_positions=42, type_vocab=1, eps=1e-5),
}


def vocab(cfg, words=WORDS):
    return {token: i for i, token in enumerate(tuple(cfg['specials']) + tuple(words))}


def ids_of(cfg, words=WORDS):
    v = vocab(cfg, words)
    return dict(cls_id=v[cfg['cls']], sep_id=v[cfg['sep']], pad_id=v[cfg['pad']])


def tokenizer(cfg, words=WORDS):
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    v = vocab(cfg, words)
    tok = Tokenizer(models.WordLevel(v, unk_token=cfg['unk']))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    tok.post_processor = processors.TemplateProcessing(
        single=f'{cfg["cls"]} $A {cfg["sep"]}',
        special_tokens=[(cfg['cls'], v[cfg['cls']]), (cfg['sep'], v[cfg['sep']])])
    return tok


def position_offset(cfg, words=WORDS):
    return ids_of(cfg, words)['pad_id'] + 1 if cfg['model_type'] == 'roberta' else 0


def state_dict(cfg, seed, vocab_size=None, std=.3, prefix=True):
    """Every matrix and bias N(0, std), LayerNorm weights 1 + N(0, .1); with the pooler a
    real checkpoint has and the encoder does not read."""
    g = torch.Generator().manual_seed(seed)
    w, i = cfg['width'], cfg['intermediate']
    v = vocab_size or len(vocab(cfg))
    sd = {}

    def put(name, *shape, norm=False):
        t = torch.randn(*shape, generator=g)
        sd[name] = 1 + .1 * t if norm else std * t

    put('embeddings.word_embeddings.weight', v, w)
    put('embeddings.position_embeddings.weight', cfg['max_positions'], w)
    put('embeddings.token_type_embeddings.weight', cfg['type_vocab'], w)
    put('embeddings.LayerNorm.weight', w, norm=True)
    put('embeddings.LayerNorm.bias', w)
    for layer in range(cfg['layers']):
        p = f'encoder.layer.{layer}.'
        for name in ('attention.self.query', 'attention.self.key', 'attention.self.value',
                     'attention.output.dense'):
            put(p + name + '.weight', w, w)
            put(p + name + '.bias', w)
        put(p + 'attention.output.LayerNorm.weight', w, norm=True)
        put(p + 'attention.output.LayerNorm.bias', w)
        put(p + 'intermediate.dense.weight', i, w)
        put(p + 'intermediate.dense.bias', i)
        put(p + 'output.dense.weight', w, i)
        put(p + 'output.dense.bias', w)
        put(p + 'output.LayerNorm.weight', w, norm=True)
        put(p + 'output.LayerNorm.bias', w)
    put('pooler.dense.weight', 4, 4)
    if prefix:
        sd = {cfg['model_type'] + '.' + key: value for key, value in sd.items()}
    return sd


def strip(sd):
    return {key.split('.', 1)[1]: value for key, value in sd.items()}


def ref_cfg(cfg, words=WORDS):
    """The keyword arguments bertref's encoder takes."""
    return dict(heads=cfg['heads'], num_layers=cfg['num_layers'],
                position_offset=position_offset(cfg, words), eps=cfg['eps'])


def sentences(generator, count, longest, words=WORDS, shortest=1):
    out = []
    for _ in range(count):
        n = int(torch.randint(shortest, longest + 1, (1,), generator=generator))
        picks = torch.randint(0, len(words), (n,), generator=generator).tolist()
        out.append(' '.join(words[i] for i in picks))
    return out
