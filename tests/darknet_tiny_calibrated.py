"""A test YOLOv3-tiny detector whose folded BatchNorm is not the identity: the tiny counterpart of darknet_calibrated.py (test
infrastructure: nothing under the package imports this).

Same recipe and the same constants (imported): gamma and beta drawn per channel, the running statistics calibrated on a seeded batch
(one train-mode forward with ``momentum=None``), the heads' biases N(0, BETA_STD), the person logit raised and the objectness of every
head and anchor shifted so that a fixed fraction of the batch's (cell, anchor) pairs passes SCORE.  Two things differ:

* the network has 2 535 candidates per 416 x 416 image where Darknet-53 has 10 647, so the passing fraction is 4 x PASS_FRAC: the same
  few tens of boxes per image;
* the calibration batch is 416 x 416 (the network is cheap on a CPU; at 256 x 256 the coarse head would have 128 cells per anchor and the
  quantile would be its second-best cell).

``storage_forward`` is this file's own: it knows ``maxpool`` (the Darknet-53 one would take a pool for a head).  A max-pool selects one
of its bf16 inputs, so it adds no rounding and stores nothing new.  CPU work, deterministic for a seed, built once per process."""
import torch
import torch.nn.functional as F

from darknet_calibrated import BETA_STD, GAMMA, PASS_FRAC, PERSON_LOGIT, SCORE, SEED, boxes_per_image, folded_convs, images  # noqa: F401
from pam import yolov3

CALIB_SHAPE = (2, 3, 416, 416)
TINY_PASS_FRAC = 4 * PASS_FRAC

_CACHE = {}


def _build(seed):
    g = torch.Generator().manual_seed(seed)
    model = yolov3.Darknet(yolov3.tiny_cfg()).init_random(seed)        # He-normal convs; BN and heads replaced below
    layers = model.layers
    with torch.no_grad():
        for m, b in zip(model.mods, layers):
            if b['type'] != 'convolutional':
                continue
            if hasattr(m, 'bn'):
                m.bn.weight.copy_(GAMMA[0] + (GAMMA[1] - GAMMA[0]) * torch.rand(b['filters'], generator=g))
                m.bn.bias.copy_(BETA_STD * torch.randn(b['filters'], generator=g))
                m.bn.momentum = None                  # cumulative average: after ONE forward the running stats are that batch's
                m.bn.reset_running_stats()
            else:
                m.conv.bias.copy_(BETA_STD * torch.randn(m.conv.out_channels, generator=g))
        model.train()
        model(images(CALIB_SHAPE, seed + 1))
        model.eval()
        for m in model.conv_modules():
            if hasattr(m, 'bn'):
                m.bn.momentum = 0.1
        heads = model(images(CALIB_SHAPE, seed + 1))
        st = 5 + model.yolo_layers()[0]['classes']
        for m, h in zip([m for m, b in zip(model.mods, layers) if b['type'] == 'convolutional' and not b['batch_normalize']], heads):
            for a in range(3):
                m.conv.bias[a * st + 5] += PERSON_LOGIT
                v = h[:, a * st:(a + 1) * st]
                cls = torch.sigmoid(v[:, 5] + PERSON_LOGIT).flatten()
                obj = v[:, 4].flatten()
                # score > SCORE  <=>  obj + shift > logit(SCORE / cls): the TINY_PASS_FRAC quantile of obj - logit(SCORE / cls)
                need = torch.where(cls > SCORE, torch.logit((SCORE / cls).clamp(max=1 - 1e-6)), torch.full_like(cls, 1e4))
                margin = obj - need
                k = max(1, int(round(TINY_PASS_FRAC * margin.numel())))
                m.conv.bias[a * st + 4] -= float(torch.topk(margin, k).values[-1]) - 1e-3
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def calibrated(seed=SEED, width=416, height=416):
    """The calibrated tiny Darknet (BN unfolded, eval mode) for a cfg of that input size, the same object for every call of a process.
    Callers must not modify it.  The weights do not depend on the input size."""
    key = (seed, width, height)
    if key not in _CACHE:
        if (width, height) == (416, 416):
            _CACHE[key] = _build(seed)
        else:
            m = yolov3.Darknet(yolov3.tiny_cfg(width, height))
            m.load_state_dict(calibrated(seed).state_dict())
            for p in m.parameters():
                p.requires_grad_(False)
            _CACHE[key] = m.eval()
    return _CACHE[key]


def storage_forward(model, x, bf16_weights=True, bf16_store=True, trace=None):
    """The folded network on x (N, 3, H, W) in fp32 arithmetic, with bf16 conv weights and every stored conv output rounded to bf16 when
    asked -> the heads, fp32.  Max-pools, routes and the upsample move stored values without rounding.  With both flags set this is
    the bf16 floor of the executor.  trace: a list that receives (layer index, output) of every convolution."""
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
                x = rnd(x)
                if trace is not None:
                    trace.append((i, x))
            elif t == 'maxpool':
                x = yolov3.darknet_maxpool(x, b['size'], b['stride'])
            elif t == 'route':
                xs = [outs[l if l >= 0 else i + l] for l in b['layers']]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, 1)
            elif t == 'upsample':
                x = F.interpolate(x, scale_factor=b['stride'], mode='nearest')
            elif t == 'yolo':
                heads.append(x)
            else:
                raise NotImplementedError(t)
            outs.append(x)
    return heads
