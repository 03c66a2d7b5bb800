"""CPU: the calibrated test network of hrnet_calibrated.py must stay a network whose folded biases and per-channel scales are non-trivial
and whose activations stay bounded -- the per-module GPU parity tests (test_gpu_hrnet_modules.py) see a packing fault only through them."""
import os

import torch
import torch.nn as nn

import hrnet_calibrated as HC
from pam import hrnet
from test_hrnet_checkpoint import OFFICIAL_KEYS


def test_every_folded_conv_has_a_real_bias_and_non_uniform_scales():
    state, folded = HC.calibrated()
    convs = [(name, m) for name, m in folded.named_modules() if isinstance(m, nn.Conv2d)]
    assert len(convs) == 293
    for name, m in convs:
        assert m.bias is not None and float(m.bias.abs().max()) > 0.05, name
    # per-channel scale of every (conv, BN) pair: gamma / sqrt(var + eps) must spread, not sit at one value
    for key, v in state.items():
        if key.endswith('.running_var'):
            s = state[key[:-len('running_var')] + 'weight'] / torch.sqrt(v + hrnet.BN_EPS)
            assert float(s.max() / s.min()) > 1.5, key
    # the same two facts on the network the product builds with random weights are what made the old whole-network checks blind
    plain = hrnet._folded_random_model(48, 17, 0)
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in plain.modules() if isinstance(m, nn.Conv2d) and m is not plain.final_layer)


def test_module_outputs_stay_bounded_on_a_fresh_input():
    folded = HC.calibrated()[1]
    x = torch.randn((1, 3, 256, 192), generator=torch.Generator().manual_seed(123))
    taps = HC.stage_inputs(folded, x)
    rms = lambda t: float(t.pow(2).mean().sqrt())
    outs = [taps['stem'], taps['layer1']] + taps['t1'] + [taps['t2'], taps['t3'], taps['features']]
    for stage in ('stage2', 'stage3', 'stage4'):
        for xs in taps[stage]:
            outs += xs
    assert len(outs) == 7 + 2 + 4 * 3 + 3 * 4
    for t in outs:
        assert 0.1 <= rms(t) <= 100.0, [round(rms(q), 3) for q in outs]


def test_calibrated_network_is_deterministic():
    a = HC._build(HC.SEED)[0]
    b = HC.calibrated()[0]
    assert a.keys() == b.keys()
    for k in a:
        assert torch.allclose(a[k].float(), b[k].float(), rtol=1e-5, atol=1e-6), k


def test_checkpoint_of_the_calibrated_network_loads_as_the_product_does(tmp_path):
    """The state dict carries the official key layout, and a file written from it (plain or wrapped as {'model': ...}) comes back through
    the product's checkpoint loader as exactly the folded module the tests compare with."""
    state, folded = HC.calibrated()
    for k in OFFICIAL_KEYS:
        assert k in state, k
    ref = folded.state_dict()
    for wrap in (False, True):
        path = os.path.join(str(tmp_path), 'pose_hrnet_w48_384x288%s.pth' % ('_w' if wrap else ''))
        torch.save({'model': state} if wrap else state, path)
        got = hrnet.load_folded_checkpoint(path, 48, 17).state_dict()
        assert got.keys() == ref.keys()
        for k in ref:
            assert torch.equal(got[k], ref[k]), k
