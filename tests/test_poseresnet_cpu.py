"""PoseResNet on the CPU: the module matches the published Simple Baselines sizes and the upstream key layout, BN folding (transposed
convolutions included) keeps the eval forward, checkpoints load in every file form, HRNetPose names the depths and model names it
supports before it asks for a GPU, the deconvolution weight image holds every weight once in the documented order, a float64
emulation of k_deconv4x4s2's four parity GEMMs fed from that image equals F.conv_transpose2d, and the executor's shape-only forward
has the right shapes and counts the network's FLOPs exactly."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pam import hrnet, poseresnet
from pam.poseresnet import PoseResNet

PARAMS_M = {50: 34.00, 101: 52.99, 152: 68.64}
KEYS = {50: 338, 101: 644, 152: 950}
FLOPS = {(50, (256, 192)): 10826022912, (101, (256, 192)): 18098946048, (152, (256, 192)): 25371869184,
         (50, (384, 288)): 24358551552, (101, (384, 288)): 40722628608, (152, (384, 288)): 57086705664}


@pytest.mark.parametrize('depth', [50, 101, 152])
def test_parameter_and_key_counts_and_head_shapes(depth):
    m = PoseResNet(depth)
    assert abs(sum(p.numel() for p in m.parameters()) / 1e6 - PARAMS_M[depth]) <= 0.005
    sd = m.state_dict()
    assert len(sd) == KEYS[depth]
    shapes = {'deconv_layers.0.weight': (2048, 256, 4, 4), 'deconv_layers.1.weight': (256,), 'deconv_layers.1.running_var': (256,),
              'deconv_layers.3.weight': (256, 256, 4, 4), 'deconv_layers.4.bias': (256,), 'deconv_layers.6.weight': (256, 256, 4, 4),
              'deconv_layers.7.running_mean': (256,), 'final_layer.weight': (17, 256, 1, 1), 'final_layer.bias': (17,),
              'conv1.weight': (64, 3, 7, 7), 'layer1.0.downsample.0.weight': (256, 64, 1, 1), 'layer4.0.downsample.0.weight': (2048, 1024, 1, 1)}
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    assert not any(k.startswith('deconv_layers.%d.' % i) for k in sd for i in (2, 5, 8))
    assert isinstance(m.layer1[0], hrnet.Bottleneck) and m.layer2[0].conv2.stride == (2, 2) and m.layer2[0].conv1.stride == (1, 1)


def _calibrated_like(depth, seed=3):
    g = torch.Generator().manual_seed(seed)
    m = poseresnet.init_random(PoseResNet(depth), seed)
    with torch.no_grad():
        for bn in m.modules():
            if isinstance(bn, nn.BatchNorm2d):
                bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=g)); bn.bias.copy_(0.3 * torch.randn(bn.num_features, generator=g))
                bn.running_mean.copy_(0.2 * torch.randn(bn.num_features, generator=g)); bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
        m.final_layer.bias.copy_(0.1 * torch.randn(17, generator=g))
    return m.eval()


@pytest.mark.parametrize('res', [(256, 192), (384, 288)])
def test_folded_equals_unfolded_in_float64(res):
    m = _calibrated_like(50).double()
    folded = poseresnet.fold_batchnorm(copy.deepcopy(m))
    assert not any(isinstance(x, nn.BatchNorm2d) for x in folded.modules())
    assert all(c.bias is not None for c in folded.deconv_layers if isinstance(c, nn.ConvTranspose2d))
    x = torch.randn((1, 3) + res, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with torch.no_grad():
        a, b = m(x), folded(x)
    assert float((a - b).norm() / a.norm()) <= 1e-10


def test_hrnet_fold_is_untouched():
    """hrnet.fold_batchnorm on HRNet stays what it was: the PoseResNet fold is a function of its own, and on HRNet both agree bit for bit."""
    a = hrnet.fold_batchnorm(hrnet.init_random(hrnet.PoseHighResolutionNet(32), 1))
    b = poseresnet.fold_batchnorm(hrnet.init_random(hrnet.PoseHighResolutionNet(32), 1))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


@pytest.mark.parametrize('form', ['plain', 'wrapped', 'module', 'no_nbt'])
def test_checkpoint_round_trip_in_every_file_form(tmp_path, form):
    m = _calibrated_like(50, seed=7)
    sd = m.state_dict()
    if form == 'module':
        sd = {'module.' + k: v for k, v in sd.items()}
    elif form == 'no_nbt':
        sd = {k: v for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    obj = {'model': sd} if form == 'wrapped' else sd
    p = str(tmp_path / 'pose_resnet_50.pth')
    torch.save(obj, p)
    got = poseresnet.load_folded_checkpoint(p, 50)
    ref = poseresnet.fold_batchnorm(copy.deepcopy(m))
    for (k, v), (k2, v2) in zip(got.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k


def test_checkpoint_of_another_depth_raises(tmp_path):
    p = str(tmp_path / 'pose_resnet_101.pth')
    torch.save(PoseResNet(101).state_dict(), p)
    with pytest.raises(RuntimeError, match='PoseResNet-50'):
        poseresnet.load_folded_checkpoint(p, 50)
    p2 = str(tmp_path / 'pose_resnet_50.pth')
    torch.save(PoseResNet(50).state_dict(), p2)
    with pytest.raises(RuntimeError):
        poseresnet.load_folded_checkpoint(p2, 152)


def test_hrnet_pose_names_depths_and_model_names_before_asking_for_a_gpu():
    for name in poseresnet.MODEL_NAMES:
        for c in (18, 34, 48, 200):
            with pytest.raises(ValueError, match='depth'):
                hrnet.HRNetPose(c, 17, None, model_name=name, resolution=(256, 192))
    for name in ('HigherHRNet', 'pose_resnet', 'Resnet', None):
        with pytest.raises(ValueError, match='model_name'):
            hrnet.HRNetPose(50, 17, None, model_name=name, resolution=(256, 192))
    with pytest.raises(ValueError, match='width'):
        hrnet.HRNetPose(50, 17, None)                                  # the default model_name is HRNet: 50 is no HRNet width


def test_deconv_image_holds_every_weight_once_in_the_documented_order():
    cin, cout = 64, 128
    idx = poseresnet.deconv_image_index(cin, cout)
    assert idx.numel() == cin * cout * 16 and torch.equal(idx.reshape(-1).sort()[0], torch.arange(cin * cout * 16))
    w = torch.randn((cin, cout, 4, 4), generator=torch.Generator().manual_seed(2))
    img = poseresnet.deconv_image(w).reshape(4, cout // 64, cin // 32, 4, 4, 64, 8)       # [p][s][c][t][j][lane][8]
    for (p, s, c, t, j, lane) in [(0, 0, 0, 0, 0, 0), (3, 1, 1, 3, 3, 63), (1, 0, 1, 2, 1, 17), (2, 1, 0, 1, 2, 40)]:
        py, px, ty, tx = p >> 1, p & 1, t >> 1, t & 1
        ky, kx = poseresnet.DECONV_TAPS[py][ty][0], poseresnet.DECONV_TAPS[px][tx][0]
        co = 64 * s + 16 * ((lane & 15) >> 2) + 4 * j + (lane & 3)
        ci = 32 * c + 8 * (lane >> 4)
        assert torch.equal(img[p, s, c, t, j, lane], w[ci:ci + 8, co, ky, kx]), (p, s, c, t, j, lane)
    # every (ky, kx) belongs to exactly one (parity, tap)
    kk = sorted((poseresnet.DECONV_TAPS[py][ty][0], poseresnet.DECONV_TAPS[px][tx][0]) for py in range(2) for px in range(2)
                for ty in range(2) for tx in range(2))
    assert kk == [(a, b) for a in range(4) for b in range(4)]


@pytest.mark.parametrize('shape', [(2, 64, 64, 3, 5), (1, 32, 128, 4, 4), (3, 96, 64, 2, 7)])
def test_parity_gemm_emulation_equals_conv_transpose2d(shape):
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    wt = torch.randn((cin, cout, 4, 4), generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    x = torch.randn((n, cin, h, w), generator=g, dtype=torch.float64)
    got = poseresnet.deconv_emulate(x, poseresnet.deconv_image(wt), b, cin, cout)
    ref = F.conv_transpose2d(x, wt, b, 2, 1)
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-12


def test_stem_fragments_hold_every_tap_once():
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    fr = poseresnet.stem_fragments(conv)                               # [j][ky][s][lane][8]
    w = conv.weight.detach()
    for (j, ky, s, lane) in [(0, 0, 0, 0), (3, 6, 1, 47), (2, 3, 1, 63), (1, 5, 0, 20)]:
        co = 16 * ((lane & 15) >> 2) + 4 * j + (lane & 3)
        kx = 4 * s + (lane >> 4)
        exp = torch.zeros(8)
        if kx < 7:
            exp[:3] = w[co, :, ky, kx]
        assert torch.equal(fr[j, ky, s, lane], exp)


def _meta_engine(depth):
    from pam.hrnet_hip import HipPoseResNet
    eng = HipPoseResNet.__new__(HipPoseResNet)
    eng.lib, eng.device = None, torch.device('meta')
    m = poseresnet.fold_batchnorm(PoseResNet(depth).eval())
    m.final_layer = nn.Identity()
    HipPoseResNet._pack(eng, m, torch.device('meta'))
    return eng


@pytest.mark.parametrize('depth,res', sorted(FLOPS))
def test_meta_forward_shapes_and_counted_flops(depth, res):
    eng = _meta_engine(depth)
    h, w = res
    exp = dict(stem=(64, h // 4, w // 4), layer1=(256, h // 4, w // 4), layer2=(512, h // 8, w // 8), layer3=(1024, h // 16, w // 16),
               layer4=(2048, h // 32, w // 32), deconv0=(256, h // 16, w // 16), deconv1=(256, h // 8, w // 8), deconv2=(256, h // 4, w // 4))
    x = torch.empty((3, 8, h, w), dtype=torch.bfloat16, device='meta').contiguous(memory_format=torch.channels_last)
    for stop in eng.STAGES:
        for cfg in eng.CONFIGS:
            eng.apply_config(cfg)
            eng.stop_after = stop
            y = eng._features(x)
            assert tuple(y.shape) == (3,) + exp[stop], (stop, cfg)
    eng.stop_after = None
    for cfg in eng.CONFIGS:
        eng.apply_config(cfg)
        eng.count = dict(bytes=0, flops=0, launches=0)
        eng._features(x[:1])
        assert eng.count['flops'] == FLOPS[(depth, res)] == poseresnet.count_flops(depth, res), cfg


def test_executor_has_one_configuration_per_setting_and_no_flags():
    from pam.hrnet_hip import HipPoseResNet
    assert HipPoseResNet.config_name in HipPoseResNet.CONFIGS and len(HipPoseResNet.CONFIGS) == 2
    assert {v['fuse_layer1'] for v in HipPoseResNet.CONFIGS.values()} == {True, False}
    assert HipPoseResNet.flag_sync is False and HipPoseResNet.multi_stream is False
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)                     # no GPU: only what config_for and _flag_sync_ok read
    net.hip, net.autotune, net.tuned, net.width = HipPoseResNet.__new__(HipPoseResNet), True, {}, None
    assert [net.config_for(n) for n in (1, 5, 20, 60)] == ['resnet_fused'] * 4
    assert not net._flag_sync_ok()
