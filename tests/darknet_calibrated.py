"""A test Darknet-53 detector whose folded BatchNorm is not the identity (test infrastructure: nothing under the package imports this).

``Darknet.init_random`` draws BN statistics that fold to biases of ~0.1 and a narrow spread of channel scales, and biases the objectness
logits so far down that the detector emits few boxes.  The network here draws gamma and beta per channel and then calibrates the running
statistics on a seeded batch (one train-mode forward with ``momentum=None``), so that every folded conv gets its own per-channel scale and
a clearly non-zero bias while the activations stay bounded through all 75 convolutions.  The three heads' objectness biases are then set
from the same batch so that a 416 x 416 image gives a few tens of boxes at score 0.5.

Inputs are random images in the detector's own range (RGB / 255, i.e. U[0, 1]): what ``pam_resize_frames`` hands the network.
CPU work, deterministic for a seed, built once per process."""
import numpy as np
import torch

from oracle import yolo_ref as Y
from pam import yolov3

SEED = 23
CALIB_SHAPE = (2, 3, 256, 256)        # the calibration batch: seeded U[0, 1] images at a CPU-cheap size
GAMMA = (0.5, 1.5)                    # gamma ~ U[0.5, 1.5] on every BN ...
RESIDUAL_DAMP = 0.3                   # ... times this on the conv just before each [shortcut]
BETA_STD = 0.3                        # beta ~ N(0, 0.3)
PASS_FRAC = 0.003                     # fraction of (cell, anchor) pairs of each head whose person score passes SCORE on the batch
SCORE = 0.5
PERSON_LOGIT = 2.0                    # class-0 logit bias: the person probability mostly ~0.9, so objectness decides

_CACHE = {}


def images(shape, seed):
    """Seeded random images in [0, 1], (n, 3, h, w) float32."""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _build(seed):
    g = torch.Generator().manual_seed(seed)
    model = yolov3.Darknet(yolov3.default_cfg()).init_random(seed)     # He-normal convs; BN and heads replaced below
    layers = model.layers
    with torch.no_grad():
        for i, (m, b) in enumerate(zip(model.mods, layers)):
            if b['type'] != 'convolutional':
                continue
            if hasattr(m, 'bn'):
                gamma = GAMMA[0] + (GAMMA[1] - GAMMA[0]) * torch.rand(b['filters'], generator=g)
                if i + 1 < len(layers) and layers[i + 1]['type'] == 'shortcut':
                    gamma = gamma * RESIDUAL_DAMP
                m.bn.weight.copy_(gamma)
                m.bn.bias.copy_(BETA_STD * torch.randn(b['filters'], generator=g))
                m.bn.momentum = None                  # cumulative average: after ONE forward the running stats are that batch's
                m.bn.reset_running_stats()
            else:                                     # a head: bias N(0, 0.3) everywhere, then the person logit and objectness below
                m.conv.bias.copy_(BETA_STD * torch.randn(m.conv.out_channels, generator=g))
        model.train()
        model(images(CALIB_SHAPE, seed + 1))
        model.eval()
        for m in model.conv_modules():
            if hasattr(m, 'bn'):
                m.bn.momentum = 0.1
        # objectness: per head and anchor, the shift that lets PASS_FRAC of the batch's cells score above SCORE
        heads = model(images(CALIB_SHAPE, seed + 1))
        nc = model.yolo_layers()[0]['classes']
        st = 5 + nc
        for m, h in zip([m for m, b in zip(model.mods, layers) if b['type'] == 'convolutional' and not b['batch_normalize']], heads):
            for a in range(3):
                m.conv.bias[a * st + 5] += PERSON_LOGIT
                v = h[:, a * st:(a + 1) * st]
                cls = torch.sigmoid(v[:, 5] + PERSON_LOGIT).flatten()
                obj = v[:, 4].flatten()
                # score > SCORE  <=>  obj + shift > logit(SCORE / cls): the PASS_FRAC quantile of obj - logit(SCORE / cls)
                need = torch.where(cls > SCORE, torch.logit((SCORE / cls).clamp(max=1 - 1e-6)), torch.full_like(cls, 1e4))
                margin = obj - need
                k = max(1, int(round(PASS_FRAC * margin.numel())))
                m.conv.bias[a * st + 4] -= float(torch.topk(margin, k).values[-1]) - 1e-3
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def calibrated(seed=SEED, width=416, height=416):
    """The calibrated Darknet (BN unfolded, eval mode) for a cfg of that input size, the same object for every call of a process.
    Callers must not modify it.  The weights do not depend on the input size (the cfg's convolutions are the same); the objectness
    calibration runs at CALIB_SHAPE for every size."""
    key = (seed, width, height)
    if key not in _CACHE:
        base = _CACHE.get((seed, 416, 416))
        if base is None and (width, height) != (416, 416):
            base = calibrated(seed)
        if base is None:
            _CACHE[key] = _build(seed)
        else:
            m = yolov3.Darknet(yolov3.default_cfg(width, height))
            m.load_state_dict(base.state_dict())
            for p in m.parameters():
                p.requires_grad_(False)
            _CACHE[key] = m.eval()
    return _CACHE[key]


def folded_convs(model, bf16=True):
    """{layer index: the folded nn.Conv2d (BN inside weight and bias)} of every [convolutional] layer; bf16=True rounds the weights to
    bf16 as PackedConv does (biases stay fp32)."""
    out = {}
    for i, (m, b) in enumerate(zip(model.mods, model.layers)):
        if b['type'] == 'convolutional':
            c = yolov3.fold_conv(m)
            if bf16:
                with torch.no_grad():
                    c.weight.copy_(c.weight.to(torch.bfloat16).float())
            for p in c.parameters():
                p.requires_grad_(False)
            out[i] = c
    return out


def storage_forward(model, x, bf16_weights=True, bf16_store=True):
    """The folded network on x (N, 3, H, W) in fp32 arithmetic, with bf16 conv weights and every stored layer output (each conv with its
    activation and fused shortcut, each upsample + route) rounded to bf16 when asked: -> the three heads (N, 255, g, g), fp32.  With
    both flags set this is the bf16 floor of the executor: what bf16 weights and bf16 storage alone cost a whole forward."""
    F = torch.nn.functional
    convs = {i: c.to(x.device) for i, c in folded_convs(model, bf16_weights).items()}
    rnd = (lambda t: t.to(torch.bfloat16).float()) if bf16_store else (lambda t: t)
    outs, heads = [], []
    with torch.no_grad():
        for i, b in enumerate(model.layers):
            t = b['type']
            if t == 'convolutional':
                x = convs[i](x)
                if b['activation'] == 'leaky':
                    x = F.leaky_relu(x, 0.1)
                x = x if i + 1 < len(model.layers) and model.layers[i + 1]['type'] == 'shortcut' else rnd(x)
            elif t == 'shortcut':
                x = rnd(outs[i - 1] + outs[i + b['from']])
            elif t == 'route':
                xs = [outs[l if l >= 0 else i + l] for l in b['layers']]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, 1)
            elif t == 'upsample':
                x = F.interpolate(x, scale_factor=b['stride'], mode='nearest')
            else:
                heads.append(x)
            outs.append(x)
    return heads


def boxes_per_image(model, heads, score=SCORE, nms=0.45, max_det=1024):
    """(boxes after NMS, candidates) per image of fp32 heads [(N, C, g, g)] through the oracle's decode + NMS."""
    anchors = np.array([[yl['anchors'][k] for k in yl['mask']] for yl in model.yolo_layers()], dtype=np.float32)
    hs = [h.permute(0, 2, 3, 1).float().cpu().numpy() for h in heads]
    res = []
    for i in range(hs[0].shape[0]):
        kept, cand = Y.detect([h[i] for h in hs], anchors, model.width, model.height, 80, 0, score, nms, model.width, model.height, max_det)
        res.append((len(kept), cand))
    return res
