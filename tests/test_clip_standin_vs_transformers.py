"""tests/golden/clip_standin.py against an independent statement of CLIP that is
installed here: HuggingFace transformers' `CLIPModel`, built offline from a
`CLIPConfig` with random weights, the stand-in's weights copied across.  The
goldens come from the reference run over the stand-in, and tests/clipref.py was
written by the same hand: this removes the possibility that both share a
mistake (pre-LN order, QuickGELU's constant, the q / k / v split, the position
of `ln_pre` / `ln_post`, where the text embedding is read)."""
import pathlib
import sys

import pytest
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / 'golden'))
import clip_standin  # noqa: E402

transformers = pytest.importorskip('transformers')

DIMS = dict(resolution=48, patch=12, vision_width=40, vision_layers=3, vision_heads=5,
            embed_dim=24, context_length=20, vocab_size=70, text_width=36, text_layers=2,
            text_heads=4)


def hf_clip(dims, sd):
    common = dict(hidden_act='quick_gelu', layer_norm_eps=1e-5, attention_dropout=0.,
                  projection_dim=dims['embed_dim'])
    text = dict(vocab_size=dims['vocab_size'], hidden_size=dims['text_width'],
                intermediate_size=4 * dims['text_width'],
                num_hidden_layers=dims['text_layers'],
                num_attention_heads=dims['text_heads'],
                max_position_embeddings=dims['context_length'],
                # (the stand-in reads the row of the largest id; transformers reads the
                # first eos_token_id: the stand-in's end-of-text id is the largest)
                eos_token_id=dims['vocab_size'] - 1, bos_token_id=dims['vocab_size'] - 2,
                pad_token_id=0, **common)
    vision = dict(hidden_size=dims['vision_width'], intermediate_size=4 * dims['vision_width'],
                  num_hidden_layers=dims['vision_layers'],
                  num_attention_heads=dims['vision_heads'], image_size=dims['resolution'],
                  patch_size=dims['patch'], **common)
    config = transformers.CLIPConfig(text_config=text, vision_config=vision,
                                     projection_dim=dims['embed_dim'])
    model = transformers.CLIPModel(config).eval()
    mapped = {
        'vision_model.embeddings.class_embedding': sd['visual.class_embedding'],
        'vision_model.embeddings.patch_embedding.weight': sd['visual.conv1.weight'],
        'vision_model.embeddings.position_embedding.weight': sd['visual.positional_embedding'],
        'vision_model.pre_layrnorm.weight': sd['visual.ln_pre.weight'],
        'vision_model.pre_layrnorm.bias': sd['visual.ln_pre.bias'],
        'vision_model.post_layernorm.weight': sd['visual.ln_post.weight'],
        'vision_model.post_layernorm.bias': sd['visual.ln_post.bias'],
        'visual_projection.weight': sd['visual.proj'].T,
        'text_model.embeddings.token_embedding.weight': sd['token_embedding.weight'],
        'text_model.embeddings.position_embedding.weight': sd['positional_embedding'],
        'text_model.final_layer_norm.weight': sd['ln_final.weight'],
        'text_model.final_layer_norm.bias': sd['ln_final.bias'],
        'text_projection.weight': sd['text_projection'].T,
    }
    for ours, theirs, layers, width in (
            ('visual.transformer.', 'vision_model.', dims['vision_layers'],
             dims['vision_width']),
            ('transformer.', 'text_model.', dims['text_layers'], dims['text_width'])):
        for layer in range(layers):
            a, b = f'{ours}resblocks.{layer}.', f'{theirs}encoder.layers.{layer}.'
            w, bias = sd[a + 'attn.in_proj_weight'], sd[a + 'attn.in_proj_bias']
            for i, name in enumerate(('q_proj', 'k_proj', 'v_proj')):
                mapped[b + f'self_attn.{name}.weight'] = w[i * width:(i + 1) * width]
                mapped[b + f'self_attn.{name}.bias'] = bias[i * width:(i + 1) * width]
            for kind in ('weight', 'bias'):
                mapped[b + 'self_attn.out_proj.' + kind] = sd[a + 'attn.out_proj.' + kind]
                mapped[b + 'layer_norm1.' + kind] = sd[a + 'ln_1.' + kind]
                mapped[b + 'layer_norm2.' + kind] = sd[a + 'ln_2.' + kind]
                mapped[b + 'mlp.fc1.' + kind] = sd[a + 'mlp.c_fc.' + kind]
                mapped[b + 'mlp.fc2.' + kind] = sd[a + 'mlp.c_proj.' + kind]
    missing, unexpected = model.load_state_dict(mapped, strict=False)
    assert not unexpected, unexpected
    assert all('position_ids' in m or m == 'logit_scale' for m in missing), missing
    return model


def features(out):
    # (transformers 5 returns an output object, 4 the tensor)
    return out if isinstance(out, torch.Tensor) else out.pooler_output


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_standin_matches_transformers_clip(dtype):
    clip_standin.configure(seed=21, **DIMS)
    ours = clip_standin.load()[0].to(dtype)
    theirs = hf_clip(DIMS, ours.state_dict()).to(dtype)
    g = torch.Generator().manual_seed(4)
    images = torch.randn(3, 3, DIMS['resolution'], DIMS['resolution'], generator=g).to(dtype)
    tokens = clip_standin.tokenize(['a dog', 'the blue sky over grass', 'x'])
    with torch.no_grad():
        a, b = ours.encode_image(images), features(theirs.get_image_features(pixel_values=images))
        c, d = ours.encode_text(tokens), features(theirs.get_text_features(input_ids=tokens))
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    print(dtype, 'image', (a - b).abs().max().item(), 'text', (c - d).abs().max().item(),
          'scale', a.abs().max().item(), c.abs().max().item())
    assert a.shape == b.shape == (3, DIMS['embed_dim']) and c.shape == d.shape
    assert (a - b).abs().max() <= tol * max(1., a.abs().max().item())
    assert (c - d).abs().max() <= tol * max(1., c.abs().max().item())
