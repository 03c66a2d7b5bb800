"""Test YOLOv4 and YOLOv4-tiny detectors whose folded BatchNorm is not the identity: the counterpart of darknet_calibrated.py /
darknet_tiny_calibrated.py for the networks of pam.yolov4 (test infrastructure: nothing under the package imports this).

Same recipe and the same constants (imported): gamma and beta drawn per channel (gamma damped on the convolution in front of each
[shortcut]), the running statistics calibrated on a seeded batch (one train-mode forward with ``momentum=None``), the heads' biases
N(0, BETA_STD), the person logit raised and the objectness of every head and anchor shifted so that a fixed fraction of the batch's
(cell, anchor) pairs passes SCORE.  The calibration batch is 416 x 416 for both networks: the tiny one as in darknet_tiny_calibrated.py
(and the same four-fold passing fraction for its 2 535 candidates), YOLOv4 as in darknet_spp_calibrated.py (on the 8 x 8 map of a
256 x 256 image the SPP block's 9- and 13-windows are the global maximum: statistics of another network).

``storage_forward`` knows what these cfgs add: mish, group routes, routes anywhere, max-pools and shortcuts.  Data layers move stored
bf16 values without rounding.  CPU work, deterministic for a seed, built once per process."""
import torch
import torch.nn.functional as F

from darknet_calibrated import BETA_STD, GAMMA, PASS_FRAC, PERSON_LOGIT, RESIDUAL_DAMP, SCORE, SEED, folded_convs, images  # noqa: F401
from pam import yolov3, yolov4

ARCH = {'yolov4': (yolov4.yolov4_cfg, (2, 3, 416, 416), PASS_FRAC), 'yolov4-tiny': (yolov4.yolov4_tiny_cfg, (2, 3, 416, 416), 4 * PASS_FRAC)}

_CACHE = {}


def _build(arch, seed):
    cfg, calib_shape, pass_frac = ARCH[arch]
    g = torch.Generator().manual_seed(seed)
    model = yolov4.Darknet4(cfg()).init_random(seed)                   # He-normal convs; BN and heads replaced below
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
            else:
                m.conv.bias.copy_(BETA_STD * torch.randn(m.conv.out_channels, generator=g))
        model.train()
        model(images(calib_shape, seed + 1))
        model.eval()
        for m in model.conv_modules():
            if hasattr(m, 'bn'):
                m.bn.momentum = 0.1
        heads = model(images(calib_shape, seed + 1))
        st = 5 + model.yolo_layers()[0]['classes']
        for m, h in zip([m for m, b in zip(model.mods, layers) if b['type'] == 'convolutional' and not b['batch_normalize']], heads):
            for a in range(3):
                m.conv.bias[a * st + 5] += PERSON_LOGIT
                v = h[:, a * st:(a + 1) * st]
                cls = torch.sigmoid(v[:, 5] + PERSON_LOGIT).flatten()
                obj = v[:, 4].flatten()
                # score > SCORE  <=>  obj + shift > logit(SCORE / cls): the pass_frac quantile of obj - logit(SCORE / cls)
                need = torch.where(cls > SCORE, torch.logit((SCORE / cls).clamp(max=1 - 1e-6)), torch.full_like(cls, 1e4))
                margin = obj - need
                k = max(1, int(round(pass_frac * margin.numel())))
                m.conv.bias[a * st + 4] -= float(torch.topk(margin, k).values[-1]) - 1e-3
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def calibrated(arch, seed=SEED, width=416, height=416):
    """The calibrated Darknet4 of that architecture ('yolov4' | 'yolov4-tiny'; BN unfolded, eval mode) for a cfg of that input size, the
    same object for every call of a process.  Callers must not modify it.  The weights do not depend on the input size."""
    key = (arch, seed, width, height)
    if key not in _CACHE:
        if (width, height) == (416, 416):
            _CACHE[key] = _build(arch, seed)
        else:
            m = yolov4.Darknet4(ARCH[arch][0](width, height))
            m.load_state_dict(calibrated(arch, seed).state_dict())
            for p in m.parameters():
                p.requires_grad_(False)
            _CACHE[key] = m.eval()
    return _CACHE[key]


def storage_forward(model, x, bf16_weights=True, bf16_store=True):
    """The folded network on x (N, 3, H, W) in fp32 arithmetic, with bf16 conv weights and every stored layer output (each convolution
    with its activation and fused shortcut) rounded to bf16 when asked -> the heads in cfg order, fp32.  With both flags set this is the
    bf16 floor of the executor."""
    convs = {i: c.to(x.device) for i, c in folded_convs(model, bf16_weights).items()}
    rnd = (lambda t: t.to(torch.bfloat16).float()) if bf16_store else (lambda t: t)
    outs, heads = [], []
    with torch.no_grad():
        for i, b in enumerate(model.layers):
            t = b['type']
            if t == 'convolutional':
                x = convs[i](x)
                x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else (F.mish(x) if b['activation'] == 'mish' else x)
                x = x if i + 1 < len(model.layers) and model.layers[i + 1]['type'] == 'shortcut' else rnd(x)
            elif t == 'shortcut':
                x = rnd(outs[i - 1] + outs[i + b['from']])
            elif t == 'maxpool':
                x = yolov3.darknet_maxpool(x, b['size'], b['stride'])
            elif t == 'route':
                xs = [outs[l if l >= 0 else i + l] for l in b['layers']]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, 1)
                if b['groups'] > 1:
                    x = torch.chunk(x, b['groups'], 1)[b['group_id']]
            elif t == 'upsample':
                x = F.interpolate(x, scale_factor=b['stride'], mode='nearest')
            elif t == 'yolo':
                heads.append(x)
            else:
                raise NotImplementedError(t)
            outs.append(x)
    return heads
