"""hrnet_calibrated.py's calibrated-BN test network with the width as a parameter (HRNet-W32 and -W48; test infrastructure: nothing
under the package imports this).  Same recipe and constants: gamma ~ U[0.5, 1.5] (x 0.3 on residual BNs), beta ~ N(0, 0.3), running
statistics calibrated on one seeded 256 x 192 batch, BN folded.  The width-independent helpers (bf16_weights, stage_inputs,
bf16_storage) are hrnet_calibrated's own."""
import copy

import torch
import torch.nn as nn

from pam import hrnet
from hrnet_calibrated import SEED, CALIB_SHAPE, GAMMA, RESIDUAL_DAMP, BETA_STD, bf16_weights, stage_inputs, bf16_storage  # noqa: F401

_CACHE = {}


def _build(width, seed):
    g = torch.Generator().manual_seed(seed)
    model = hrnet.init_random(hrnet.PoseHighResolutionNet(width, 17), seed=seed)         # He-normal convs; BN replaced below
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


def calibrated(width, seed=SEED):
    """-> (state_dict, folded): the unfolded network's state dict in the official key layout (what a checkpoint file holds) and the
    folded fp32 module (BN inside every conv's weight and bias), the same for every call of a process.  Callers must not modify them."""
    if (width, seed) not in _CACHE:
        _CACHE[(width, seed)] = _build(width, seed)
    return _CACHE[(width, seed)]


def folded_copy(width, seed=SEED):
    """A private copy of the folded fp32 module."""
    return copy.deepcopy(calibrated(width, seed)[1])
