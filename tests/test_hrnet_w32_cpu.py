"""HRNet-W32 on the CPU: every convolution of the W32 network packs (32-channel outputs, the 224-channel merged up-convolution, the
fused 32-channel BasicBlock), the C = 32 block image holds every output channel exactly once per tap in the documented permutation and
swizzle, HRNetPose names the widths it supports, and a W32 checkpoint in the official key layout loads."""
import os

import pytest
import torch
import torch.nn as nn

from pam import hrnet
from pam.hrnet_hip import HipHRNet, HipHRNetW32, PackedBlock, PackedConv


def _convs(model):
    return [m for m in model.modules() if isinstance(m, nn.Conv2d) and m is not model.final_layer]


def test_every_w32_convolution_packs():
    m = hrnet._folded_random_model(32, 17, 0)
    convs = _convs(m)
    assert len(convs) == 292
    outs = set()
    for c in convs:
        op = PackedConv(c, 'cpu', pad_cin_to=8 if c.in_channels == 3 else None)
        outs.add(op.cout)
        if c.kernel_size == (3, 3) and c.stride == (1, 1) and c.in_channels == 32 and c.out_channels == 32:
            assert op._w_ohwi is not None                          # the rows-in-LDS form (k_conv3x3<32>) has a weight image
    assert 32 in outs
    blocks = [b for b in m.modules() if isinstance(b, hrnet.BasicBlock) and b.conv1.out_channels == 32]
    assert len(blocks) == 32                                       # 4 blocks of branch 0 in each of the eight HR modules
    for b in blocks:
        assert PackedBlock(b.conv1, b.conv2, 'cpu').wpack.numel() == 1024 + 2 * 9 * 32 * 64
    # the 224-channel merged up-convolution of the stage-4 modules' coarsest branch (32 + 64 + 128 output channels)
    up = [f[0] for f in (m.stage4[0].fuse_layers[i][3] for i in range(3))]
    assert PackedConv.merged(up, 'cpu').cout == 224


def test_w32_block_image_holds_every_channel_once_per_tap_in_the_documented_order():
    """wpack = [bias 1 KiB][conv1: 9 k-steps x 32 rows x 4 pieces x 8][conv2: same].  Row j * 16 + q = output channel 8 (q >> 2) + 4 j + (q & 3);
    physical piece p of row R holds input channels 8 (p ^ ((R >> 2) & 3)) .. + 7 of the k-step's tap."""
    g = torch.Generator().manual_seed(3)
    c1, c2 = nn.Conv2d(32, 32, 3, 1, 1), nn.Conv2d(32, 32, 3, 1, 1)
    with torch.no_grad():
        for c in (c1, c2):
            c.weight.copy_(torch.randn(c.weight.shape, generator=g).to(torch.bfloat16).float())
            c.bias.copy_(torch.randn(32, generator=g))
    pb = PackedBlock(c1, c2, 'cpu')
    assert pb.c == 32
    head = pb.wpack[:1024].view(torch.float32)
    assert torch.equal(head[:32], c1.bias) and torch.equal(head[32:64], c2.bias) and not head[64:].any()
    img = pb.wpack[1024:].view(torch.bfloat16).float().reshape(2, 9, 32, 4, 8)
    for k, conv in enumerate((c1, c2)):
        w = conv.weight.detach()                                   # [cout][cin][ky][kx]
        for t in range(9):
            seen = []
            for R in range(32):
                j, q = R // 16, R % 16
                ch = 8 * (q >> 2) + 4 * j + (q & 3)
                seen.append(ch)
                for p in range(4):
                    lp = p ^ ((R >> 2) & 3)
                    assert torch.equal(img[k, t, R, p], w[ch, 8 * lp:8 * lp + 8, t // 3, t % 3]), (k, t, R, p)
            assert sorted(seen) == list(range(32))


def test_hrnet_pose_rejects_unsupported_widths_before_anything_else():
    for c in (40, 64, 18):
        with pytest.raises(ValueError, match='width'):
            hrnet.HRNetPose(c, 17, None, resolution=(256, 192))


def test_w32_executor_configurations_and_rule():
    keys = {frozenset(v) for v in HipHRNet.CONFIGS.values()} | {frozenset(v) for v in HipHRNetW32.CONFIGS.values()}
    assert len(keys) == 1                                          # every configuration sets the same switches
    assert HipHRNetW32.config_name in HipHRNetW32.CONFIGS
    assert HipHRNetW32.CONFIGS['w32_fused']['block2'] & 1 and not HipHRNetW32.CONFIGS['w32_unfused']['block2'] & 1
    assert all(not v['fused_sums'] and not v['slab32'] for v in HipHRNetW32.CONFIGS.values())
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)                 # no GPU: only what config_for reads
    net.hip, net.autotune, net.tuned = HipHRNetW32.__new__(HipHRNetW32), True, {}
    net.width = 32
    assert {net.config_for(n) for n in (1, 4, 12, 20, 60)} == {HipHRNetW32.config_name}
    assert hrnet.HRNetPose.width == 48


def test_w32_checkpoint_in_the_official_key_layout_round_trips(tmp_path):
    src = hrnet.init_random(hrnet.PoseHighResolutionNet(32, 17), seed=5)
    with torch.no_grad():
        for m in src.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5); m.bias.uniform_(-0.1, 0.1)
    sd = src.state_dict()
    assert 'stage4.2.branches.0.0.conv1.weight' in sd and sd['final_layer.weight'].shape == (17, 32, 1, 1)
    for wrap in (False, True):
        path = os.path.join(str(tmp_path), 'pose_hrnet_w32_256x192_%d.pth' % wrap)
        torch.save({'model': sd} if wrap else sd, path)
        folded = hrnet.load_folded_checkpoint(path, 32, 17)
        ref = hrnet.fold_batchnorm(src.eval())
        x = torch.randn((1, 3, 128, 96), generator=torch.Generator().manual_seed(2))
        with torch.no_grad():
            assert torch.allclose(folded(x), ref(x), atol=1e-5, rtol=1e-5)
