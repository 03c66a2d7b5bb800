"""A test HRNet-W48 whose folded BatchNorm is not the identity (test infrastructure: nothing under the package imports this).

``hrnet.init_random`` sets every BN to gamma = 1 (0.3 on residual BNs), beta = 0, mean = 0, var = 1: after ``fold_batchnorm`` every
folded bias is 0 and every per-channel scale is uniform, so no test on it can see a bias that is packed, concatenated, sliced or summed
wrongly.  The network here draws gamma and beta per channel and then calibrates the running statistics on a seeded batch (one train-mode
forward with ``momentum=None``), which keeps the activations bounded through all eight HR modules while every folded conv gets its own
per-channel scale and a non-trivial bias.  CPU work, deterministic for a seed, built once per process."""
import copy

import torch
import torch.nn as nn

from pam import hrnet

SEED = 11
CALIB_SHAPE = (2, 3, 256, 192)        # the calibration batch: seeded N(0, 1) crops at the smaller pose resolution
GAMMA = (0.5, 1.5)                    # gamma ~ U[0.5, 1.5] on every BN ...
RESIDUAL_DAMP = 0.3                   # ... times this on the last BN of every residual branch (bn2 of BasicBlock, bn3 of Bottleneck), as init_random
BETA_STD = 0.3                        # beta ~ N(0, 0.3)

_CACHE = {}


def _build(seed):
    g = torch.Generator().manual_seed(seed)
    model = hrnet.init_random(hrnet.PoseHighResolutionNet(48, 17), seed=seed)         # He-normal convs; BN replaced below
    residual = set()
    for m in model.modules():
        if isinstance(m, hrnet.BasicBlock):
            residual.add(id(m.bn2))
        elif isinstance(m, hrnet.Bottleneck):
            residual.add(id(m.bn3))
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                gamma = GAMMA[0] + (GAMMA[1] - GAMMA[0]) * torch.rand(m.num_features, generator=g)
                if id(m) in residual:
                    gamma = gamma * RESIDUAL_DAMP
                m.weight.copy_(gamma)
                m.bias.copy_(BETA_STD * torch.randn(m.num_features, generator=g))
                m.momentum = None                     # cumulative average: after ONE forward the running stats are that batch's
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
    folded = hrnet.fold_batchnorm(copy.deepcopy(model)).eval()
    for p in folded.parameters():
        p.requires_grad_(False)
    return state, folded


def calibrated(seed=SEED):
    """-> (state_dict, folded): the unfolded network's state dict in the official key layout (what a checkpoint file holds) and the
    folded fp32 module (BN inside every conv's weight and bias), the same for every call of a process.  Callers must not modify them."""
    if seed not in _CACHE:
        _CACHE[seed] = _build(seed)
    return _CACHE[seed]


def folded_copy(seed=SEED):
    """A private copy of the folded fp32 module."""
    return copy.deepcopy(calibrated(seed)[1])


def bf16_weights(model):
    """The folded module with every conv weight rounded to bf16 (what the HIP packing stores) and the biases left in fp32: the
    reference the per-module tests compare the kernels with."""
    m = copy.deepcopy(model)
    with torch.no_grad():
        for c in m.modules():
            if isinstance(c, nn.Conv2d):
                c.weight.copy_(c.weight.to(torch.bfloat16).float())
    return m


def stage_inputs(model, x):
    """The fp32 forward of ``model`` (folded) on x, tapped at every piece the HIP executor issues on its own:
    dict(stem, layer1, t1 = [2 transition outputs], stage2 = [inputs of its module], stage3 = [...], stage4 = [...], t2, t3, features)
    where stageK[m] is the list of branch tensors module m of stage K reads."""
    F = torch.nn.functional
    out = {}
    with torch.no_grad():
        s = F.relu(model.conv2(F.relu(model.conv1(x))))
        out['stem'] = s
        x = model.layer1(s)
        out['layer1'] = x
        xs = [model.transition1[0](x), model.transition1[1](x)]
        out['t1'] = list(xs)
        out['stage2'] = [list(xs)]
        xs = model.stage2[0](xs)
        out['t2'] = model.transition2[2](xs[-1])
        xs = xs + [out['t2']]
        out['stage3'] = []
        for m in model.stage3:
            out['stage3'].append(list(xs))
            xs = m(xs)
        out['t3'] = model.transition3[3](xs[-1])
        xs = xs + [out['t3']]
        out['stage4'] = []
        for m in model.stage4:
            out['stage4'].append(list(xs))
            xs = m(xs)
        out['features'] = xs[0]
    return out


def bf16_storage(model):
    """The folded module with bf16 conv weights that also rounds to bf16 whatever a bf16 executor stores: the output of every conv, every
    residual block and every HR module (fp32 arithmetic otherwise).  Its distance from the fp32 module is what bf16 weights and bf16
    storage alone cost a whole forward."""
    m = bf16_weights(model)
    rnd = lambda t: t.to(torch.bfloat16).float()

    def hook(mod, inp, out):
        return [rnd(t) for t in out] if isinstance(out, list) else rnd(out)
    for c in m.modules():
        if isinstance(c, (nn.Conv2d, hrnet.BasicBlock, hrnet.Bottleneck, hrnet.HighResolutionModule)) and c is not m.final_layer:
            c.register_forward_hook(hook)
    return m
