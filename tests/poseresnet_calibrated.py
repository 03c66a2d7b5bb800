"""The calibrated-BN PoseResNet test network (test infrastructure: nothing under the package imports this), built as hrnet_calibrated.py
builds HRNet's: gamma ~ U[0.5, 1.5] (x 0.3 on bn3 of every residual branch), beta ~ N(0, 0.3) on every BN (the deconvolutions' too),
running statistics from one seeded 256 x 192 batch, a non-zero head bias, BN folded (poseresnet.fold_batchnorm)."""
import copy

import torch
import torch.nn as nn

from pam import hrnet, poseresnet
from hrnet_calibrated import SEED, CALIB_SHAPE, GAMMA, RESIDUAL_DAMP, BETA_STD

_CACHE = {}


def _build(depth, seed):
    g = torch.Generator().manual_seed(seed)
    model = poseresnet.init_random(poseresnet.PoseResNet(depth, 17), seed=seed)
    residual = {id(m.bn3) for m in model.modules() if isinstance(m, hrnet.Bottleneck)}
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                gamma = GAMMA[0] + (GAMMA[1] - GAMMA[0]) * torch.rand(m.num_features, generator=g)
                if id(m) in residual:
                    gamma = gamma * RESIDUAL_DAMP
                m.weight.copy_(gamma)
                m.bias.copy_(BETA_STD * torch.randn(m.num_features, generator=g))
                m.momentum = None
                m.reset_running_stats()
        model.final_layer.bias.copy_(0.1 * torch.randn(model.final_layer.out_channels, generator=g))
        x = torch.randn(CALIB_SHAPE, generator=torch.Generator().manual_seed(seed + 1))
        model.train()
        model(x)
    model.eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 0.1
    state = {k: v.clone() for k, v in model.state_dict().items()}
    folded = poseresnet.fold_batchnorm(copy.deepcopy(model)).eval()
    for p in folded.parameters():
        p.requires_grad_(False)
    return state, folded


def calibrated(depth, seed=SEED):
    """-> (state_dict in the upstream key layout, folded fp32 module); the same objects for every call of a process (do not modify)."""
    if (depth, seed) not in _CACHE:
        _CACHE[(depth, seed)] = _build(depth, seed)
    return _CACHE[(depth, seed)]


def folded_copy(depth, seed=SEED):
    return copy.deepcopy(calibrated(depth, seed)[1])


def bf16_weights(model):
    """Every conv / transposed conv weight rounded to bf16 as the packing rounds it; biases fp32."""
    m = copy.deepcopy(model)
    with torch.no_grad():
        for c in m.modules():
            if isinstance(c, (nn.Conv2d, nn.ConvTranspose2d)):
                c.weight.copy_(c.weight.to(torch.bfloat16).float())
    return m


def stage_inputs(model, x):
    """The fp32 forward of the folded model on x (N, 3, H, W), tapped after every stage the executor can stop at:
    dict(stem, layer1 .. layer4, deconv0 .. deconv2, heatmaps)."""
    out = {}
    with torch.no_grad():
        x = model.stem(x); out['stem'] = x
        for k in range(1, 5):
            x = getattr(model, 'layer%d' % k)(x); out['layer%d' % k] = x
        dl = model.deconv_layers
        for k in range(3):
            x = dl[3 * k + 2](dl[3 * k + 1](dl[3 * k](x))); out['deconv%d' % k] = x
        out['heatmaps'] = model.final_layer(x)
    return out


def bf16_storage(model):
    """bf16 weights, and every value a bf16 executor stores rounded to bf16: each conv / transposed conv output, the max-pool and every
    Bottleneck output (fp32 arithmetic otherwise).  Its distance from the fp32 module is what bf16 alone costs a whole forward."""
    m = bf16_weights(model)
    rnd = lambda t: t.to(torch.bfloat16).float()

    def hook(mod, inp, out):
        return rnd(out)
    for c in m.modules():
        if isinstance(c, (nn.Conv2d, nn.ConvTranspose2d, nn.MaxPool2d, hrnet.Bottleneck)) and c is not m.final_layer:
            c.register_forward_hook(hook)
    return m
