"""A test YOLOv3-SPP detector whose folded BatchNorm is not the identity: the SPP counterpart of darknet_calibrated.py (test
infrastructure: nothing under the package imports this).

The recipe and its constants are darknet_calibrated.py's (imported): gamma and beta drawn per channel, damped in front of each shortcut,
the running statistics calibrated on a seeded batch (one train-mode forward with ``momentum=None``), the heads' biases N(0, BETA_STD), the
person logit raised and the objectness of every head and anchor shifted so that PASS_FRAC of the batch's (cell, anchor) pairs passes SCORE
-- the head geometry is Darknet-53's, so the fraction is too.  One thing differs: the calibration batch is 416 x 416, not 256 x 256.  At
256 the SPP block sees an 8 x 8 map, on which the 9- and 13-windows are (nearly) the global maximum: 1536 of layer 84's 2048 inputs are then
constant over the image, the batch statistics and the objectness quantile are those of another network than the one a 416 x 416 image
runs (13 x 13 map, local windows), and that one gives 68 .. 212 boxes per test image for every seed tried (23 .. 30).  Calibrated at the
size it is used at, seed 23, as there, gives 61 / 41 / 28 / 37 / 40 boxes on the five 416 x 416 test images (``check_box_counts`` asserts
5 .. 63: inside max_det = 64 and never empty).

``storage_forward`` is this file's own: Darknet-53's knows no ``maxpool`` and the tiny one no ``shortcut``.  A max-pool selects one of its
bf16 inputs and a route moves them, so the SPP block adds no rounding and stores nothing new.  CPU work, deterministic for a seed, built
once per process."""
import numpy as np
import torch
import torch.nn.functional as F

from darknet_calibrated import (BETA_STD, GAMMA, PASS_FRAC, PERSON_LOGIT, RESIDUAL_DAMP, SCORE, SEED,  # noqa: F401
                                boxes_per_image, folded_convs, images)
from oracle import yolo_ref as Y
from pam import yolov3

CALIB_SHAPE = (2, 3, 416, 416)        # see above: the SPP windows must be local on the calibration batch
_CACHE = {}


def _build(seed):
    g = torch.Generator().manual_seed(seed)
    model = yolov3.Darknet(yolov3.spp_cfg()).init_random(seed)         # He-normal convs; BN and heads replaced below
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
                # score > SCORE  <=>  obj + shift > logit(SCORE / cls): the PASS_FRAC quantile of obj - logit(SCORE / cls)
                need = torch.where(cls > SCORE, torch.logit((SCORE / cls).clamp(max=1 - 1e-6)), torch.full_like(cls, 1e4))
                margin = obj - need
                k = max(1, int(round(PASS_FRAC * margin.numel())))
                m.conv.bias[a * st + 4] -= float(torch.topk(margin, k).values[-1]) - 1e-3
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def calibrated(seed=SEED, width=416, height=416):
    """The calibrated SPP Darknet (BN unfolded, eval mode) for a cfg of that input size, the same object for every call of a process.
    Callers must not modify it.  The weights do not depend on the input size."""
    key = (seed, width, height)
    if key not in _CACHE:
        if (width, height) == (416, 416):
            _CACHE[key] = _build(seed)
        else:
            m = yolov3.Darknet(yolov3.spp_cfg(width, height))
            m.load_state_dict(calibrated(seed).state_dict())
            for p in m.parameters():
                p.requires_grad_(False)
            _CACHE[key] = m.eval()
    return _CACHE[key]


def storage_forward(model, x, bf16_weights=True, bf16_store=True):
    """darknet_calibrated.storage_forward with the [maxpool] layers: the folded network on x (N, 3, H, W) in fp32 arithmetic, with bf16
    conv weights and every stored layer output (each conv with its activation and fused shortcut) rounded to bf16 when asked -> the three
    heads, fp32.  Max-pools, routes and upsamples move stored values without rounding."""
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


def test_images(n=5, seed=21):
    """The n 416 x 416 BGR uint8 views the GPU detector test runs."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (416, 416, 3), dtype=np.uint8) for _ in range(n)]


def check_box_counts(views=5):
    """The fp32 network on the first `views` test images (as the detector sees them: RGB / 255): 5 .. 63 boxes each after NMS at SCORE, so a
    detector with max_det = 64 returns a real, uncut, non-empty list.  -> [(kept, candidates)]."""
    model = calibrated()
    x = torch.from_numpy(Y.resize_frames(np.stack(test_images()[:views]), 416, 416)).permute(0, 3, 1, 2)[:, :3].float().contiguous()
    heads = storage_forward(model, x, bf16_weights=False, bf16_store=False)
    per = boxes_per_image(model, heads)
    assert all(5 <= kept <= 63 and cand < 1024 for kept, cand in per), per
    return per
