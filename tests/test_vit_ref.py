"""CPU: vitpose.ViTPose (as float64) against the float64 NumPy restatement of tests/vit_ref.py -- two statements of the published
network that share no code -- to 1e-10 relative, on a small network (D 128, 2 heads, 2 blocks) and on ViTPose-B with one crop; and each
fault the restatement can plant (position row 0 dropped, scale omitted, tanh GELU, post-norm, padding 0) is caught by that comparison."""
import numpy as np
import pytest
import torch

import vit_ref as R
from pam import vitpose

SMALL = dict(dim=128, depth=2, heads=2)


def randomised(variant, seed):
    """A seeded module with every parameter non-trivial: LayerNorm / BN scales and shifts, biases, running statistics."""
    m = vitpose.init_random(vitpose.ViTPose(variant, 17), seed).double().eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.LayerNorm, torch.nn.BatchNorm2d)):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g, dtype=torch.float64))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g, dtype=torch.float64))
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g, dtype=torch.float64))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g, dtype=torch.float64))
            if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d)) and mod.bias is not None:
                mod.bias.copy_(0.05 * torch.randn(mod.bias.shape, generator=g, dtype=torch.float64))
    return m


def both(variant, seed, n, fault=None):
    m = randomised(variant, seed)
    x = torch.randn((n, 3, 256, 192), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
    with torch.no_grad():
        got = m(x).numpy()
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    return got, R.forward(sd, x.numpy(), m.heads, fault=fault)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize('variant,n', [(SMALL, 2), ('B', 1)], ids=['d128', 'vitpose_b'])
def test_module_equals_the_restatement(variant, n):
    got, want = both(variant, 5, n)
    assert got.shape == want.shape == (n, 17, 64, 48)
    assert rel(got, want) <= 1e-10, rel(got, want)


@pytest.mark.parametrize('fault', R.FAULTS)
def test_the_comparison_catches_a_planted_fault(fault):
    got, bad = both(SMALL, 7, 1, fault=fault)
    assert rel(got, bad) > 1e-6, (fault, rel(got, bad))


def test_token_tensor_is_the_channels_last_map():
    """The (N, T, D) tokens behind last_norm ARE the NHWC tensor (N, 16, 12, D): token_map only permutes the view."""
    m = randomised(SMALL, 9)
    tok = torch.randn(2, 192, 128, dtype=torch.float64)
    fm = m.token_map(tok)
    assert tuple(fm.shape) == (2, 128, 16, 12)
    assert torch.equal(fm.permute(0, 2, 3, 1).reshape(2, 192, 128), tok)
