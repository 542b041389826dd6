"""Digests of what the sequential nets (the two AlexNets and the VGGs) compute on the HIP trunk,
for a bit-for-bit comparison of two builds of libmilan_hip, in the style of
tools/tower_digests.py.  One line per case: the first 16 hex digits of the sha256 of each result
tensor's bytes, the status word, and the workspace byte counts (milan_classify_workspace_bytes,
milan_activations_workspace_bytes; milan_workspace_bytes for the encoder); a VGG line adds
milan_vgg_trace after each call.  Refusals are printed as the error code and its message.
Fixed seeds, small shapes.

    MILAN_LIB=<one build>     python tools/seq_digests.py > a.txt
    MILAN_LIB=<another build> python tools/seq_digests.py > b.txt
    diff a.txt b.txt

One library per process.  The torchvision AlexNet's and the VGGs' classifier sides run a second
time in a child process with MILAN_ENC_SUB=3 (the knob is read once per process): 7 images in
passes of 3 + 3 + 1.  The records: profiles/alexnet_unify.txt (the two AlexNets on one trunk)
and profiles/seq_trunk.txt (the AlexNets and the VGGs on one).
"""
import hashlib
import os
import pathlib
import subprocess
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / 'neuron-descriptions_amd'), str(REPO), str(REPO / 'tests')]

import alexref  # noqa: E402
import placesref  # noqa: E402
import vggref  # noqa: E402
import test_gpu_alexnet as A  # noqa: E402
import test_gpu_places as P  # noqa: E402
import test_gpu_vgg as V  # noqa: E402
from milan_amd import hip, synthetic  # noqa: E402

PRECISIONS = ('f32', 'split_f16')
SUB = os.environ.get('MILAN_ENC_SUB', 'unset')


def dg(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def sweep_units(ch):
    return [(level, u) for level in range(5) for u in sorted({0, 5, ch[level] - 1})]


def workspace(tag, ctx, h, w):
    for n in (1, 7, 200):
        for sweep in (0, 1, 15):
            print(tag, f'workspace n={n} sweep={sweep}',
                  int(ctx.lib.milan_classify_workspace_bytes(ctx._h, n, h, w, sweep)),
                  int(ctx.lib.milan_activations_workspace_bytes(ctx._h, n, h, w)))


def trace_of(ctx):
    """milan_vgg_trace flattened: block.conv:launches/split of the convs the context has."""
    return ','.join(f'{b}.{j}:{n}/{s}' for (b, j), (n, s) in sorted(ctx.vgg_trace().items()))


def classifier_line(tag, ctx, images, base, ch, classes, trace=False):
    """logits, predictions, the five taps, taps [3, 1], a sweep with targets, the status word;
    `trace`: milan_vgg_trace after the classify, the two taps calls and the sweep."""
    traces = []
    ctx.set_ablation(base)
    logits = ctx.classify(images)
    preds = ctx.classify(images, return_logits=False)
    traces.append(trace_of(ctx) if trace else '')
    taps = ctx.activations(images, range(5))
    traces.append(trace_of(ctx) if trace else '')
    two = ctx.activations(images, [3, 1])
    traces.append(trace_of(ctx) if trace else '')
    targets = torch.arange(len(images)) % classes
    swept, correct = ctx.classify_sweep(images, sweep_units(ch), targets)
    traces.append(trace_of(ctx) if trace else '')
    print(tag, 'logits', dg(logits), 'preds', dg(preds),
          ' '.join(f'L{l} {dg(taps[l])}' for l in range(5)), 'L3,1', dg(two[3]), dg(two[1]),
          'sweep', dg(swept), 'correct', dg(correct), 'status', ctx.status(),
          *(['trace', *traces] if trace else []))
    ctx.set_ablation([])


LAST_CODE = []
_check = hip._check


def _recording_check(code):
    LAST_CODE.append(code)
    _check(code)


hip._check = _recording_check


def refusal(tag, call):
    """The error code and the message with which the library refuses `call`."""
    del LAST_CODE[:]
    try:
        call()
    except (ValueError, RuntimeError, IndexError) as error:
        print(tag, 'code', LAST_CODE[-1] if LAST_CODE else 'python', type(error).__name__,
              str(error))
    else:
        print(tag, 'was not refused')


def alexnet_classifier():
    for width in (8, 32):
        ctx = A.make_context(alexref.make_state_dict(61, width, 72, 10))
        for geo in ((63, 63), (95, 127)):
            tag = f'alexnet.w{width}.{geo[0]}x{geo[1]} sub={SUB}'
            images = alexref.make_images(61, 7, geo)
            for precision in PRECISIONS:
                ctx.set_precision(precision)
                classifier_line(f'{tag} {precision}', ctx, images, [(0, 1), (2, 5)],
                                alexref.channels(width), 10)
            workspace(tag, ctx, *geo)
        ctx.close()


def alexnet_encoder():
    g = torch.Generator().manual_seed(9)
    images = torch.randint(256, (6, 3, 96, 96), generator=g, dtype=torch.uint8)
    masks = (torch.rand(6, 1, 96, 96, generator=g) > 0.6).to(torch.uint8)
    for width in (8, 32):
        ctx = A.make_context(alexref.make_state_dict(61, width, 72, 10), head=False)
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            features = ctx.encode(images, masks)
            print(f'alexnet.w{width} {precision} encode', tuple(features.shape), dg(features),
                  'status', ctx.status())
        print(f'alexnet.w{width} encoder workspace',
              *[int(ctx.lib.milan_workspace_bytes(ctx._h, n, 1, 96, 1, 1)) for n in (1, 7)])
        ctx.close()


def places():
    base = [(1, 3), (3, 5)]
    for width, lrn, groups, n in ((8, False, True, 5), (8, True, True, 5), (16, False, True, 5),
                                  (16, True, True, 5), (64, False, True, 2), (8, False, False, 5)):
        ctx = P.make_context(P.model_sd(width, groups), lrn=lrn)
        ch = placesref.channels(width)
        tag = f'places.w{width}.lrn{int(lrn)}.groups{int(groups)}'
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            classifier_line(f'{tag}.227x227 {precision}', ctx, P.pictures((227, 227), n), base,
                            ch, P.CLASSES)
            ctx.set_ablation(base)
            for geo in ((99, 131), (35, 38)):
                taps = ctx.activations(P.pictures(geo, n), range(5))
                print(f'{tag}.{geo[0]}x{geo[1]} {precision}',
                      ' '.join(f'L{l} {dg(taps[l])}' for l in range(5)), 'status', ctx.status())
            ctx.set_ablation([])
        workspace(f'{tag}.227x227', ctx, 227, 227)
        ctx.close()
    bare = P.make_context(P.model_sd(8), head=False)
    for precision in PRECISIONS:
        bare.set_precision(precision)
        print(f'places.w8.headless.227x227 {precision} L4',
              dg(bare.activations(P.pictures((227, 227)), [4])[4]), 'status', bare.status())
    workspace('places.w8.headless.227x227', bare, 227, 227)
    bare.close()


VGG_BASES = ([], [(0, 1), (2, 5), (4, 3)])
IRREGULAR = (1, 2, 3, 4, 1)


def irregular_vgg(width):
    """(trunk under `vgg.B.J`, head) of a net with IRREGULAR convs per block, which no
    torchvision config has."""
    g = torch.Generator().manual_seed(V.SEED + 7)
    trunk, cin = {}, 3
    for b, count in enumerate(IRREGULAR):
        cout = vggref.CHANNELS[b] * width
        for j in range(count):
            trunk[f'{V.PREFIX}vgg.{b + 1}.{j}.weight'] = (
                torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9))**0.5)
            trunk[f'{V.PREFIX}vgg.{b + 1}.{j}.bias'] = 0.05 * torch.randn(cout, generator=g)
            cin = cout
    head = []
    for fan, out in ((cin * 49, V.HIDDEN), (V.HIDDEN, V.HIDDEN), (V.HIDDEN, V.CLASSES)):
        head += [torch.randn(out, fan, generator=g) * (2.0 / fan)**0.5,
                 0.05 * torch.randn(out, generator=g)]
    return trunk, head


def vgg_contexts():
    for config, width in (('vgg11', 8), ('vgg11', 32), ('vgg16', 16), ('vgg19', 8), ('vgg19', 32)):
        yield f'{config}.w{width}', width, V.make_context(V.model_sd(config, width), config)
    trunk, head = irregular_vgg(16)
    yield 'vgg12345.w16', 16, hip.Context(hip.make_dims(trunk, 1), trunk, torch.device('cuda'),
                                           vgg_head=head)


def vgg():
    for name, width, ctx in vgg_contexts():
        ch = vggref.channels(width)
        for geo in ((32, 32), (45, 38)):
            tag = f'{name}.{geo[0]}x{geo[1]} sub={SUB}'
            images = V.pictures(geo, 7)
            for precision in PRECISIONS:
                ctx.set_precision(precision)
                for base in VGG_BASES:
                    classifier_line(f'{tag} {precision} base={len(base)}', ctx, images, base, ch,
                                    V.CLASSES, trace=True)
            workspace(tag, ctx, *geo)
        # 17x9 reaches level 3 (2x1 pixels) and no further
        tag = f'{name}.17x9 sub={SUB}'
        small = V.pictures((17, 9), 7)
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            for base in VGG_BASES:
                ctx.set_ablation(base)
                taps = ctx.activations(small, range(4))
                two = ctx.activations(small, [3, 1])
                print(f'{tag} {precision} base={len(base)}',
                      ' '.join(f'L{l} {dg(taps[l])}' for l in range(4)), 'L3,1', dg(two[3]),
                      dg(two[1]), 'status', ctx.status(), 'trace', trace_of(ctx))
                refusal(f'{tag} {precision} base={len(base)} L4',
                        lambda: ctx.activations(small, [4]))
                refusal(f'{tag} {precision} base={len(base)} L0,4',
                        lambda: ctx.activations(small, [0, 4]))
                ctx.set_ablation([])
        workspace(tag, ctx, 17, 9)
        ctx.close()


def vgg_headless():
    bare = V.make_context(V.model_sd('vgg16', 16), 'vgg16', head=False)
    for geo in ((32, 32), (45, 38), (17, 9)):
        images = V.pictures(geo, 7)
        for precision in PRECISIONS:
            bare.set_precision(precision)
            for base in VGG_BASES:
                bare.set_ablation(base)
                taps = bare.activations(images, range(4))
                print(f'vgg16.w16.headless.{geo[0]}x{geo[1]} sub={SUB} {precision} '
                      f'base={len(base)}', ' '.join(f'L{l} {dg(taps[l])}' for l in range(4)),
                      'status', bare.status(), 'trace', trace_of(bare))
                bare.set_ablation([])
        workspace(f'vgg16.w16.headless.{geo[0]}x{geo[1]}', bare, *geo)
    bare.close()


def narrowed(head):
    """the six tensors with the first layer one input short: a head of wrong widths"""
    return [head[0][:, :-1].contiguous(), *head[1:]]


def other_widths(head):
    """a head that chains, with one hidden unit fewer than `head`"""
    return [head[0][:-1].contiguous(), head[1][:-1].contiguous(),
            head[2][:, :-1].contiguous(), *head[3:]]


def refusals():
    """What the three families say to a too-small image, a missing head, a head of wrong
    widths, a second head of other widths and the other family's head setter."""
    asd = alexref.make_state_dict(61, 8, 72, 10)
    psd = P.model_sd(8)
    vsd = V.model_sd('vgg16', 8)
    phead = [psd[f'{fc}.{part}'] for fc in ('fc6', 'fc7', 'fc8') for part in ('weight', 'bias')]
    families = (
        ('alexnet', lambda head: A.make_context(asd, head=head), A.head_of(asd),
         alexref.make_images(61, 2, (62, 63)), alexref.make_images(61, 2, (63, 63))),
        ('places', lambda head: P.make_context(psd, head=head), phead,
         P.pictures((226, 227), 2), P.pictures((227, 227), 2)),
        ('vgg', lambda head: V.make_context(vsd, 'vgg16', head=head), V.head_of(vsd),
         V.pictures((31, 32), 2), V.pictures((32, 32), 2)))
    tiny, mid = torch.zeros(2, 3, 10, 12), torch.zeros(2, 3, 18, 18)
    for name, make, head, small, fits in families:
        ctx = make(True)
        setter = ctx.set_vgg_head if name == 'vgg' else ctx.set_alexnet_head
        other = ctx.set_alexnet_head if name == 'vgg' else ctx.set_vgg_head
        for precision in PRECISIONS:
            ctx.set_precision(precision)
            tag = f'refusal {name} {precision}'
            refusal(f'{tag} classify small', lambda: ctx.classify(small))
            refusal(f'{tag} classify tiny', lambda: ctx.classify(tiny))
            refusal(f'{tag} sweep small', lambda: ctx.classify_sweep(small, [(0, 0), (3, 1)]))
            refusal(f'{tag} sweep of nothing small', lambda: ctx.classify_sweep(small, []))
            refusal(f'{tag} activations small', lambda: ctx.activations(small, [4]))
            refusal(f'{tag} activations tiny', lambda: ctx.activations(tiny, [4]))
            refusal(f'{tag} activations tiny L0,1', lambda: ctx.activations(tiny, [0, 1]))
            refusal(f'{tag} activations 18x18 L1', lambda: ctx.activations(mid, [1]))
            refusal(f'{tag} activations 18x18 L4,0', lambda: ctx.activations(mid, [4, 0]))
            refusal(f'{tag} activations level 5', lambda: ctx.activations(fits, [5]))
            refusal(f'{tag} activations twice', lambda: ctx.activations(fits, [2, 2]))
            refusal(f'{tag} ablation level 5', lambda: ctx.set_ablation([(5, 0)]))
            refusal(f'{tag} ablation unit', lambda: ctx.set_ablation([(4, 1 << 20)]))
            refusal(f'{tag} sweep level 5', lambda: ctx.classify_sweep(fits, [(5, 0)]))
        ctx.set_precision('f32')
        before = dg(ctx.classify(fits))
        refusal(f'refusal {name} head of wrong widths', lambda: setter(*narrowed(head)))
        refusal(f'refusal {name} second head of other widths', lambda: setter(*other_widths(head)))
        refusal(f'refusal {name} the other setter', lambda: other(*head))
        setter(*head)   # (the same widths again: accepted)
        print(f'refusal {name} the head is as it was', before == dg(ctx.classify(fits)))
        ctx.close()
        bare = make(False)
        bare.set_precision('f32')
        refusal(f'refusal {name} headless classify', lambda: bare.classify(fits))
        refusal(f'refusal {name} headless sweep', lambda: bare.classify_sweep(fits, [(0, 0)]))
        refusal(f'refusal {name} headless ablation', lambda: bare.set_ablation([(0, 0)]))
        refusal(f'refusal {name} headless activations', lambda: bare.activations(fits, [0]))
        refusal(f'refusal {name} headless head of wrong widths',
                lambda: (bare.set_vgg_head if name == 'vgg' else
                         bare.set_alexnet_head)(*narrowed(head)))
        bare.close()
    sd = {A.PREFIX + k: v
          for k, v in synthetic.resnet_state_dict('resnet18', seed=1, width=8).items()}
    resnet = hip.Context(hip.make_dims(sd, 1, blocks=(2, 2, 2, 2)), sd, torch.device('cuda'))
    refusal('refusal resnet milan_set_alexnet_head', lambda: resnet.set_alexnet_head(*phead))
    refusal('refusal resnet milan_set_vgg_head', lambda: resnet.set_vgg_head(*phead))
    resnet.close()


def resnet_workspace():
    sd = {A.PREFIX + k: v
          for k, v in synthetic.resnet_state_dict('resnet18', seed=1, width=8).items()}
    ctx = hip.Context(hip.make_dims(sd, 1, blocks=(2, 2, 2, 2)), sd, torch.device('cuda'))
    workspace('resnet18.w8.33x47', ctx, 33, 47)
    ctx.close()


def main():
    hip.require_device(torch.device('cuda:0'))
    alexnet_classifier()
    vgg()
    vgg_headless()
    if '--child' in sys.argv:
        torch.cuda.synchronize()
        return
    alexnet_encoder()
    places()
    refusals()
    resnet_workspace()
    torch.cuda.synchronize()
    print('done sub=' + SUB, flush=True)
    child = subprocess.run(['timeout', '-k', '10', '300', sys.executable, __file__, '--child'],
                           env=dict(os.environ, MILAN_ENC_SUB='3'))
    if child.returncode != 0:
        sys.exit(f'the MILAN_ENC_SUB=3 child ended with {child.returncode}')
    print('done sub=3')


if __name__ == '__main__':
    main()
