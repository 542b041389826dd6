"""CPU tests of milan_amd.vits: DINO's module tree and key names, the dims inferred from a
state dict, and the eager path (forward, activations, hooks, errors) against tests/vitref.py
in float64 within vitref's bound.  The native path is tests/test_gpu_vit.py's.
"""
import pytest
import torch

import vitref
from milan_amd import exemplars, vits

TOY = vitref.make_dims(res=24, patch=8, width=32, heads=2, depth=2, hidden=64)


def dino_vits8_keys():
    """Names and shapes of dino_vits8's state dict, as facebookresearch/dino saves it."""
    keys = [('cls_token', (1, 1, 384)), ('pos_embed', (1, 785, 384)),
            ('patch_embed.proj.weight', (384, 3, 8, 8)), ('patch_embed.proj.bias', (384,))]
    for i in range(12):
        b = f'blocks.{i}.'
        keys += [(b + 'norm1.weight', (384,)), (b + 'norm1.bias', (384,)),
                 (b + 'attn.qkv.weight', (1152, 384)), (b + 'attn.qkv.bias', (1152,)),
                 (b + 'attn.proj.weight', (384, 384)), (b + 'attn.proj.bias', (384,)),
                 (b + 'norm2.weight', (384,)), (b + 'norm2.bias', (384,)),
                 (b + 'mlp.fc1.weight', (1536, 384)), (b + 'mlp.fc1.bias', (1536,)),
                 (b + 'mlp.fc2.weight', (384, 1536)), (b + 'mlp.fc2.bias', (384,))]
    keys += [('norm.weight', (384,)), ('norm.bias', (384,))]
    return keys


def toy_model(dims=TOY, seed=3):
    sd = vitref.cast(vitref.weights(dims, seed), torch.float32)
    model = vits.from_state_dict(sd, num_heads=dims['heads'])
    return model, sd


def test_state_dict_keys_are_dinos():
    model = vits.dino_vits8()
    got = sorted((k, tuple(v.shape)) for k, v in model.state_dict().items())
    assert got == sorted(dino_vits8_keys())
    assert model.tokens == 785 and model.hidden == 1536
    assert vits.dino_vits16().pos_embed.shape == (1, 197, 384)


def test_layers_are_the_references_twelve():
    assert vits.dino_vits8().layers == (
        'blocks.0.mlp.fc1', 'blocks.1.mlp.fc1', 'blocks.2.mlp.fc1', 'blocks.3.mlp.fc1',
        'blocks.4.mlp.fc1', 'blocks.5.mlp.fc1', 'blocks.6.mlp.fc1', 'blocks.7.mlp.fc1',
        'blocks.8.mlp.fc1', 'blocks.9.mlp.fc1', 'blocks.10.mlp.fc1', 'blocks.11.mlp.fc1')


def test_load_state_dict_round_trip():
    model, sd = toy_model()
    other = vits.VisionTransformer(img_size=24, patch_size=8, embed_dim=32, depth=2,
                                   num_heads=2, mlp_ratio=2.)
    other.load_state_dict(model.state_dict(), strict=True)
    assert sorted(other.state_dict()) == sorted(sd)
    for key, value in other.state_dict().items():
        assert torch.equal(value, sd[key]), key


def test_from_state_dict_recovers_the_dims():
    model, _ = toy_model()
    assert (model.img_size, model.patch_size, model.embed_dim, model.depth, model.num_heads,
            model.hidden) == (24, 8, 32, 2, 2, 64)
    assert not model.training
    # heads default to width // 64
    sd = vitref.cast(vitref.weights(vitref.make_dims(16, 8, 128, 2, 1, 256), 1), torch.float32)
    assert vits.from_state_dict(sd).num_heads == 2
    full = vits.infer_dims({k: torch.empty(s) for k, s in dino_vits8_keys()})
    assert full == dict(img_size=224, patch_size=8, embed_dim=384, depth=12, num_heads=6,
                        mlp_ratio=4.)
    with pytest.raises(ValueError):
        vits.from_state_dict({'norm.weight': torch.zeros(4)})


def test_eager_forward_and_activations_match_vitref():
    model, sd = toy_model()
    x64 = vitref.images(TOY, 3, seed=8)
    taps64, out64 = vitref.forward(vitref.weights(TOY, 3), x64, TOY)
    taps32, out32 = vitref.forward(sd, x64.float(), TOY)
    with torch.no_grad():
        out = model(x64.float())
    assert out.shape == (3, 32)
    vitref.check('host forward', out, out64, out32)
    acts = model.activations(x64.float(), model.layers)
    assert list(acts) == list(model.layers)
    for i, name in enumerate(model.layers):
        assert acts[name].shape == (3, vitref.tokens(TOY), 64)
        vitref.check(f'host {name}', acts[name], taps64[i], taps32[i])
    # a single name, and a layer outside `layers`
    one = model.activations(x64.float(), 'blocks.1.mlp.fc1')
    assert torch.equal(one['blocks.1.mlp.fc1'], acts['blocks.1.mlp.fc1'])
    assert model.activations(x64.float(), 'blocks.0.attn.qkv')['blocks.0.attn.qkv'].shape == (
        3, vitref.tokens(TOY), 96)
    assert sum(len(m._forward_hooks) for m in model.modules()) == 0


def test_a_forward_hook_fires_and_keeps_the_eager_path():
    model, _ = toy_model()
    x = vitref.images(TOY, 2, seed=1).float()
    seen = []
    handle = model.blocks[1].mlp.fc1.register_forward_hook(
        lambda module, inputs, output: seen.append(output.detach()))
    try:
        with torch.no_grad():
            assert not model.runs_natively(x)
            model(x)
    finally:
        handle.remove()
    assert len(seen) == 1
    assert torch.equal(seen[0], model.activations(x, 'blocks.1.mlp.fc1')['blocks.1.mlp.fc1'])


def test_eager_forward_is_differentiable():
    model, _ = toy_model()
    model.train()
    x = vitref.images(TOY, 2, seed=2).float()
    model(x).sum().backward()
    assert model.blocks[0].mlp.fc1.weight.grad.abs().sum() > 0
    assert model.pos_embed.grad.abs().sum() > 0


def test_errors():
    model, _ = toy_model()
    with pytest.raises(NotImplementedError, match='interpolation'):
        model(torch.zeros(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match='interpolation'):
        model.activations(torch.zeros(1, 3, 16, 16), 'blocks.0.mlp.fc1')
    with pytest.raises(KeyError):
        model.activations(torch.zeros(1, 3, 24, 24), 'blocks.2.mlp.fc1')
    with pytest.raises(KeyError):
        model.activations(torch.zeros(1, 3, 24, 24), ['blocks.0.mlp.fc1', 'nope'])


def test_spatialize_vit_mlp_of_a_tap():
    model, _ = toy_model()
    x = vitref.images(TOY, 2, seed=4).float()
    tap = model.activations(x, 'blocks.0.mlp.fc1')['blocks.0.mlp.fc1']
    spatial = exemplars.spatialize_vit_mlp(tap)
    assert spatial.shape == (2, 64, 3, 3)
    # unit u at grid cell (gy, gx) is token 1 + gy * G + gx
    assert torch.equal(spatial[1, 5, 2, 1], tap[1, 1 + 2 * 3 + 1, 5])
