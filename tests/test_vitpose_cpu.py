"""ViTPose on the CPU: the state-dict round trip in the published key layout (a missing key is named, a class token ignored), what
HRNetPose refuses (-S, -H, 384 x 288), count_flops against the analytic sum, and PackedLinear's packing round trip."""
import copy

import pytest
import torch

from pam import hrnet, packing, vitpose


def test_state_dict_round_trip_in_the_published_key_layout(tmp_path):
    m = vitpose.init_random(vitpose.ViTPose('B'), 3)
    keys = set(m.state_dict())
    for k in ('backbone.patch_embed.proj.weight', 'backbone.patch_embed.proj.bias', 'backbone.pos_embed', 'backbone.blocks.0.norm1.weight',
              'backbone.blocks.11.attn.qkv.bias', 'backbone.blocks.5.attn.proj.weight', 'backbone.blocks.7.norm2.bias',
              'backbone.blocks.3.mlp.fc1.weight', 'backbone.blocks.3.mlp.fc2.bias', 'backbone.last_norm.weight',
              'keypoint_head.deconv_layers.0.weight', 'keypoint_head.deconv_layers.1.running_var', 'keypoint_head.deconv_layers.3.weight',
              'keypoint_head.deconv_layers.4.bias', 'keypoint_head.final_layer.weight', 'keypoint_head.final_layer.bias'):
        assert k in keys, k
    assert not any(k.startswith('backbone.blocks.12.') for k in keys) and 'backbone.cls_token' not in keys
    assert tuple(m.state_dict()['backbone.pos_embed'].shape) == (1, 193, 768)
    assert tuple(m.state_dict()['backbone.blocks.0.attn.qkv.weight'].shape) == (2304, 768)
    sd = dict(m.state_dict())
    sd['backbone.cls_token'] = torch.zeros(1, 1, 768)                      # present in the published files, never read
    path = str(tmp_path / 'vitpose-b.pth')
    torch.save({'state_dict': sd, 'meta': {}}, path)
    got = vitpose.load_folded_checkpoint(path, 'B')
    want = vitpose.fold_batchnorm(copy.deepcopy(m))
    a, b = got.state_dict(), want.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    top = str(tmp_path / 'top.pth')                                        # the weights at top level, DataParallel prefix
    torch.save({'module.' + k: v for k, v in sd.items()}, top)
    c = vitpose.load_folded_checkpoint(top, 768).state_dict()
    assert all(torch.equal(a[k], c[k]) for k in a)


def test_a_missing_or_unexpected_key_is_named():
    sd = dict(vitpose.ViTPose('B').state_dict())
    del sd['backbone.blocks.4.mlp.fc1.bias']
    with pytest.raises(RuntimeError, match=r'1 keys missing \(backbone\.blocks\.4\.mlp\.fc1\.bias\)'):
        vitpose.load_folded_checkpoint(sd, 'B')
    sd = dict(vitpose.ViTPose('B').state_dict())
    sd['backbone.blocks.12.norm1.weight'] = torch.zeros(768)
    with pytest.raises(RuntimeError, match=r'1 unexpected \(backbone\.blocks\.12\.norm1\.weight\)'):
        vitpose.load_folded_checkpoint(sd, 'B')
    with pytest.raises(RuntimeError, match='ViTPose-L'):                   # a -B file is not a -L file
        vitpose.load_folded_checkpoint(dict(vitpose.ViTPose('B').state_dict()), 'L')


@pytest.mark.parametrize('c,res', [('S', (256, 192)), ('H', (256, 192)), (384, (256, 192)), (1280, (256, 192)), ('B', (384, 288)),
                                   (1024, (384, 288))])
def test_hrnetpose_refuses_other_variants_and_resolutions(c, res):
    """-S (head dimension 32), -H (80) and 384 x 288 are refused with a ValueError that says what is supported, before a device is touched."""
    for name in vitpose.MODEL_NAMES:
        with pytest.raises(ValueError, match=r"ViTPose-B \(c = 'B' or 768\) and ViTPose-L \(c = 'L' or 1024\) at resolution \(256, 192\)"):
            hrnet.HRNetPose(c, 17, None, model_name=name, resolution=res)


def test_variants_by_letter_and_by_width():
    assert [vitpose.variant_of(c) for c in ('B', 'b', 768, 'L', 1024)] == ['B', 'B', 'B', 'L', 'L']
    for bad in ('S', 'H', 'huge', 48, 50, None, True, 768.5):
        with pytest.raises(ValueError):
            vitpose.variant_of(bad)
    with pytest.raises(ValueError, match='unknown model_name'):
        hrnet.HRNetPose('B', 17, None, model_name='ViT')


@pytest.mark.parametrize('v', ['B', 'L'])
def test_count_flops_against_the_analytic_sum(v):
    cfg = vitpose.VARIANTS[v]
    d, depth, t = cfg['dim'], cfg['depth'], 192
    mac = t * d * 3 * 256                                                  # patch embedding at 3 channels
    mac += depth * (t * d * 3 * d + t * d * d + 2 * t * d * 4 * d + 2 * t * t * d)      # qkv, proj, fc1 + fc2, Q K^T + P V
    mac += 32 * 24 * 256 * d * 4 + 64 * 48 * 256 * 256 * 4                 # the two deconvolutions, 4 live taps per output pixel
    got = vitpose.count_flops(v)
    assert abs(got / (2.0 * mac) - 1.0) <= 0.02, (got, 2 * mac)
    if v == 'B':
        assert 17.0 < got / 2e9 < 19.0                                     # "about 17 GMAC" with the head's deconvolutions


@pytest.mark.parametrize('n,k', [(64, 64), (2304, 768), (768, 3072), (768, 2048)])
def test_packed_linear_round_trip_and_layout(n, k):
    g = torch.Generator().manual_seed(n + k)
    w = torch.randn((n, k), generator=g)
    b = torch.randn(n, generator=g)
    op = packing.PackedLinear(w, b, 'cpu')
    assert op.w.dtype == torch.bfloat16 and op.w.numel() == n * k and (op.n, op.k) == (n, k)
    assert torch.equal(packing.linear_unimage(op.w, n, k), w.to(torch.bfloat16))
    assert torch.equal(op.bias, b) and op.bias.dtype == torch.float32
    assert torch.equal(packing.PackedLinear(w, None, 'cpu').bias, torch.zeros(n))
    # the layout include/pam.h states, element by element for a few lanes
    img = op.w.reshape(n // 64, k // 32, 4, 64, 8)
    wb = w.to(torch.bfloat16)
    for s, c, j, l in ((0, 0, 0, 0), (n // 64 - 1, k // 32 - 1, 3, 63), (0, 1, 2, 37), (n // 64 - 1, 0, 1, 22)):
        ch = 64 * s + 16 * ((l & 15) >> 2) + 4 * j + (l & 3)
        assert torch.equal(img[s, c, j, l], wb[ch, 32 * c + 8 * (l >> 4):32 * c + 8 * (l >> 4) + 8]), (s, c, j, l)


def test_patch_matrix_and_position_bias():
    m = vitpose.init_random(vitpose.ViTPose(dict(dim=128, depth=1, heads=2)), 4)
    with torch.no_grad():
        m.backbone.patch_embed.proj.bias.copy_(torch.arange(128.0))
    pm = vitpose.patch_matrix(m.backbone.patch_embed.proj).reshape(128, 16, 16, 8)
    assert torch.equal(pm[..., :3], m.backbone.patch_embed.proj.weight.detach().permute(0, 2, 3, 1)) and not pm[..., 3:].any()
    pb = vitpose.position_bias(m.backbone)
    pos = m.backbone.pos_embed.detach()[0]
    assert tuple(pb.shape) == (192, 128) and torch.equal(pb[5], pos[6] + pos[0] + torch.arange(128.0))
