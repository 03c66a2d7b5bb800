"""CPU: the YOLOv4 / YOLOv4-tiny definitions of pam.yolov4 -- cfg builders against the public files' layer, convolution and weight
counts (the weight-file sizes of yolov4.weights and yolov4-tiny.weights), the fp32 Darknet4 module, the HipDarknet4 plans (built on
torch.device('cpu'): plan only, nothing is launched), the refusals, and the references of tests/yolo4_ref.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import yolo4_ref as R
from oracle import yolo_ref as Y
from pam import yolov3, yolov4

CPU = torch.device('cpu')
#            layers, convolutions, floats, bytes of the public weights file
PUBLIC = {'yolov4-tiny': (38, 21, 6062814, 24251276), 'yolov4': (162, 110, 64429405, 257717640)}


def _floats(model):
    return sum(p.numel() for m in model.conv_modules()
               for p in ([m.bn.bias, m.bn.weight, m.bn.running_mean, m.bn.running_var] if hasattr(m, 'bn') else [m.conv.bias]) + [m.conv.weight])


@pytest.fixture(scope='module')
def models():
    return {a: yolov4.Darknet4(yolov4.ARCHS4[a]()).init_random(3).eval() for a in PUBLIC}


@pytest.mark.parametrize('arch', sorted(PUBLIC))
def test_cfg_builders_match_the_public_networks(models, arch):
    layers, convs, floats, nbytes = PUBLIC[arch]
    m = models[arch]
    assert (len(m.layers), len(m.conv_modules()), _floats(m)) == (layers, convs, floats) and 20 + 4 * floats == nbytes
    yl = m.yolo_layers()
    if arch == 'yolov4':
        assert [y['mask'] for y in yl] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]] and [y['scale_x_y'] for y in yl] == [1.2, 1.1, 1.05]
        assert yl[0]['anchors'] == [(12, 16), (19, 36), (40, 28), (36, 75), (76, 55), (72, 146), (142, 110), (192, 243), (459, 401)]
        acts = [b['activation'] for b in m.layers if b['type'] == 'convolutional']
        assert acts.count('mish') == 72 and acts.count('linear') == 3 and acts.count('leaky') == 35
        assert all(b['activation'] == 'mish' for b in m.layers[:105] if b['type'] == 'convolutional')
        assert [i for i, b in enumerate(m.layers) if b['type'] == 'yolo'] == [139, 150, 161]
        assert [m.chans[i] for i in (10, 23, 54, 85, 104, 113)] == [64, 128, 256, 512, 1024, 2048]
    else:
        assert [y['mask'] for y in yl] == [[3, 4, 5], [1, 2, 3]] and [y['scale_x_y'] for y in yl] == [1.05, 1.05]
        assert yl[0]['anchors'] == [(10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319)]
        assert [m.chans[i] for i in (3, 6, 8, 11, 16, 19, 24, 34)] == [32, 64, 128, 64, 256, 128, 512, 384]
        assert [i for i, b in enumerate(m.layers) if b['type'] == 'yolo'] == [30, 37]
    assert set(yolov4.ARCHS4) == {'yolov3', 'yolov3-tiny', 'yolov3-spp', 'yolov4', 'yolov4-tiny'} and set(yolov3.ARCHS) == set(yolov4.ARCHS4) - set(PUBLIC)


@pytest.mark.parametrize('arch', sorted(PUBLIC))
def test_weight_files_have_the_public_size_and_read_back_bit_for_bit(models, arch, tmp_path):
    path = str(tmp_path / 'w.weights')
    models[arch].save_darknet_weights(path)
    assert os.path.getsize(path) == PUBLIC[arch][3]
    other = yolov4.Darknet4(yolov4.ARCHS4[arch]()).init_random(4)
    other.load_darknet_weights(path)
    a, b = models[arch].state_dict(), other.state_dict()
    for k in a:
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
    with open(path, 'ab') as f:
        f.write(b'\0\0\0\0')
    with pytest.raises(ValueError, match='left over'):
        other.load_darknet_weights(path)


def test_fp32_forward_head_shapes_in_cfg_order(models):
    with torch.no_grad():
        t = models['yolov4-tiny'](torch.rand(2, 3, 64, 64))
        v = models['yolov4'](torch.rand(1, 3, 64, 96))                        # width 96, height 64: a 2 x 3 map at stride 32
    assert [tuple(h.shape) for h in t] == [(2, 255, 2, 2), (2, 255, 4, 4)]
    assert [tuple(h.shape) for h in v] == [(1, 255, 8, 12), (1, 255, 4, 6), (1, 255, 2, 3)]        # finest first
    assert all(bool(torch.isfinite(h).all()) for h in t + v)


def test_group_route_is_torch_chunk():
    cfg = '\n'.join(['[net]', 'width=16', 'height=16', 'channels=3', '[convolutional]', 'filters=24', 'size=3', 'stride=1', 'pad=1', 'activation=mish',
                     '[route]', 'layers=-1', 'groups=3', 'group_id=2', '[convolutional]', 'filters=8', 'size=1', 'stride=1', 'pad=1', 'activation=linear',
                     '[yolo]', 'mask=0', 'anchors=1,1', 'classes=1'])
    m = yolov4.Darknet4(cfg).init_random(0).eval()
    assert m.chans == [24, 8, 8, 8]
    x = torch.rand(2, 3, 16, 16)
    with torch.no_grad():
        y0 = m.mods[0](x)
        want = m.mods[2](torch.chunk(y0, 3, 1)[2])
        assert torch.equal(m(x)[0], want)
        assert torch.equal(y0, F.mish(m.mods[0].conv(x)))


@pytest.mark.parametrize('cfg', [yolov3.default_cfg, yolov3.tiny_cfg, yolov3.spp_cfg], ids=['yolov3', 'yolov3-tiny', 'yolov3-spp'])
def test_a_v3_cfg_gives_yolov3s_module_and_plan(cfg):
    text = cfg(96, 64)
    a, b = yolov3.Darknet(text).init_random(5).eval(), yolov4.Darknet4(text).eval()
    b.load_state_dict(a.state_dict())
    x = torch.rand(2, 3, 64, 96)
    with torch.no_grad():
        for p, q in zip(a(x), b(x)):
            assert torch.equal(p, q)
    pa, pb = yolov3.HipDarknet(a, CPU), yolov4.HipDarknet4(b, CPU)
    assert len(pa.plan) == len(pb.plan) and pa.real == pb.real and pa.padded == pb.padded and pb.head_scales == [1.0] * len(a.yolo_layers())
    for s, t in zip(pa.plan, pb.plan):
        if s[0] == 'conv':
            assert s[:2] + s[3:] == t[:2] + t[3:] and torch.equal(s[2].w, t[2].w) and torch.equal(s[2].bias, t[2].bias)
        else:
            assert s == t


def _plan(text):
    return yolov4.HipDarknet4(yolov4.Darknet4(text).init_random(0).eval(), CPU)


def _route_channels(hip, model):
    """Every route step: real = the concatenation of its slices, padded = yolov3's rounding of it, slices inside their sources."""
    for s in hip.plan:
        if s[0] != 'route':
            continue
        _, dst, parts, c_pad = s
        assert hip.real[dst] == sum(p[2] for p in parts) == model.chans[dst] and hip.padded[dst] == c_pad == yolov3._round_channels(hip.real[dst])
        for src, off, cnt, up in parts:
            assert off % 8 == 0 and cnt % 8 == 0 and off + cnt <= hip.real[src] <= hip.padded[src]


def test_tiny_plan(models):
    """The cfg has 11 [route] layers: 9 run as k_route steps (3 group routes, 6 routes over two layers), `route -4` (layer 31) is an alias
    and layers 33 + 34 (upsample, route -1, 23) stay yolov3's one `upcat` launch -- 10 launches that are not aliases."""
    hip = _plan(yolov4.yolov4_tiny_cfg())
    kinds = [s[0] for s in hip.plan]
    assert [kinds.count(k) for k in ('conv', 'route', 'upcat', 'alias', 'pool', 'head', 'spp', 'add')] == [21, 9, 1, 1, 3, 2, 0, 0]
    assert sum(b['type'] == 'route' for b in models['yolov4-tiny'].layers) == 11 == kinds.count('route') + kinds.count('upcat') + kinds.count('alias')
    assert hip.head_scales == [1.05, 1.05]
    routes = {s[1]: s[2] for s in hip.plan if s[0] == 'route'}
    assert routes[3] == [(2, 32, 32, False)] and routes[11] == [(10, 64, 64, False)] and routes[19] == [(18, 128, 128, False)]
    assert routes[6] == [(5, 0, 32, False), (4, 0, 32, False)] and (hip.real[4], hip.padded[4], hip.real[6], hip.padded[6]) == (32, 64, 64, 64)
    assert routes[8] == [(2, 0, 64, False), (7, 0, 64, False)] and (hip.real[3], hip.padded[3]) == (32, 64)
    assert ('upcat', 34, 32, 23) in hip.plan and ('alias', 31, 27) in hip.plan
    _route_channels(hip, models['yolov4-tiny'])
    assert not any(s[0] == 'conv' and s[4] == 'mish' for s in hip.plan)


def test_yolov4_plan(models):
    hip = _plan(yolov4.yolov4_cfg())
    kinds = [s[0] for s in hip.plan]
    assert [kinds.count(k) for k in ('conv', 'spp', 'head', 'route', 'alias', 'upcat', 'add', 'pool')] == [110, 1, 3, 9, 9, 0, 0, 0]
    assert sum(1 for s in hip.plan if s[0] == 'conv' and s[4] == 'mish') == 72
    assert sum(1 for s in hip.plan if s[0] == 'conv' and s[5] is not None) == 23 and all(s[4] == 'mish' for s in hip.plan if s[0] == 'conv' and s[5] is not None)
    assert [s[1] for s in hip.plan if s[0] == 'head'] == [139, 150, 161] and hip.head_scales == [1.2, 1.1, 1.05]
    assert ('spp', 113, 107, (5, 9, 13)) in hip.plan
    routes = {s[1]: s[2] for s in hip.plan if s[0] == 'route'}
    # the two [upsample] layers have no step of their own: the routes behind them read the half-size maps through the x2 flag
    assert routes[121] == [(120, 0, 256, False), (117, 0, 256, True)] and routes[131] == [(130, 0, 128, False), (127, 0, 128, True)]
    assert routes[142] == [(141, 0, 256, False), (126, 0, 256, False)] and routes[153] == [(152, 0, 512, False), (116, 0, 512, False)]
    assert not any(s[1] in (118, 128) for s in hip.plan)
    _route_channels(hip, models['yolov4'])
    assert hip.plan[0][0] == 'conv' and hip.plan[0][2]._stem is not None and hip.plan[0][4] == 'mish'


def test_yolov4_at_608_plans_or_names_its_limit():
    try:
        hip = _plan(yolov4.yolov4_cfg(608, 608))
    except NotImplementedError as e:
        assert 'layer' in str(e) or 'SPP' in str(e)
    else:
        assert len([s for s in hip.plan if s[0] == 'head']) == 3 and ('spp', 113, 107, (5, 9, 13)) in hip.plan       # a 19 x 19 map: inside k_spp's 32


def test_standalone_upsample_is_materialised_by_a_one_source_route():
    cfg = '\n'.join(['[net]', 'width=32', 'height=32', 'channels=3', '[convolutional]', 'batch_normalize=1', 'filters=64', 'size=3', 'stride=2', 'pad=1',
                     'activation=leaky', '[upsample]', 'stride=2', '[convolutional]', 'filters=18', 'size=1', 'stride=1', 'pad=1', 'activation=linear',
                     '[yolo]', 'mask=0,1,2', 'anchors=1,1,2,2,3,3', 'classes=1'])
    hip = _plan(cfg)
    assert hip.plan[1] == ('route', 1, [(0, 0, 64, True)], 64)
    with pytest.raises(NotImplementedError, match='upsample'):
        yolov3.HipDarknet(yolov3.Darknet(cfg).init_random(0).eval(), CPU)         # yolov3's refusal stands


HEAD = ['[net]', 'width=32', 'height=32', 'channels=3', '[convolutional]', 'batch_normalize=1', 'filters=64', 'size=3', 'stride=1', 'pad=1', 'activation=leaky']
YOLO = ['[convolutional]', 'filters=18', 'size=1', 'stride=1', 'pad=1', 'activation=linear', '[yolo]', 'mask=0,1,2', 'anchors=1,1,2,2,3,3', 'classes=1']


@pytest.mark.parametrize('extra,exc,word', [
    (YOLO + ['new_coords=1'], NotImplementedError, 'new_coords'),
    (YOLO + ['nms_kind=diounms'], NotImplementedError, 'nms_kind'),
    (YOLO + ['scale_x_y=0.9'], ValueError, 'scale_x_y'),
    (['[route]', 'layers=-1', 'groups=3', 'group_id=0'] + YOLO, ValueError, 'groups'),             # 64 channels in 3 groups
    (['[route]', 'layers=-1', 'groups=16', 'group_id=0'] + YOLO, NotImplementedError, 'multiples of 8'),   # groups of 4 channels
    (['[route]', 'layers=-1', 'groups=2', 'group_id=2'] + YOLO, ValueError, 'group_id'),
    (['[route]', 'layers=-1,-1,-1,-1,-1'] + YOLO, NotImplementedError, 'layers='),                  # 5 sources
    (['[convolutional]', 'filters=8', 'size=1', 'stride=1', 'pad=1', 'activation=swish'] + YOLO, NotImplementedError, 'swish'),
], ids=['new_coords', 'nms_kind', 'scale_x_y', 'groups-indivisible', 'groups-not-8', 'group_id', 'five-sources', 'activation'])
def test_refusals_name_the_key(extra, exc, word):
    with pytest.raises(exc, match=word):
        _plan('\n'.join(HEAD + extra))


def test_accepted_yolo_keys():
    hip = _plan('\n'.join(HEAD + YOLO + ['nms_kind=greedynms', 'scale_x_y=1.3', 'iou_loss=ciou', 'beta_nms=0.6', 'max_delta=5', 'jitter=.3', 'random=1']))
    assert hip.head_scales == [1.3]


def test_yolov3_module_keeps_its_refusals():
    with pytest.raises(NotImplementedError, match='mish'):
        yolov3.Darknet('\n'.join(HEAD[:-1] + ['activation=mish'] + YOLO))
    with pytest.raises(NotImplementedError, match='route over several layers'):
        yolov3.HipDarknet(yolov3.Darknet(yolov4.yolov4_tiny_cfg()).init_random(0).eval(), CPU)


# ---- yolo4_ref ---------------------------------------------------------------------------------------------------------------------------
def test_mish32_against_float64():
    """The definition of csrc/pam_conv.hpp in NumPy float32 on 4 million points of [-40, 40] plus +-100, +-88 and 1e4: finite everywhere,
    relative error below 1e-6 outside denormal results (measured 3.4e-7 with this exp; the bound leaves 3 x for another one)."""
    x = np.concatenate([np.linspace(-40, 40, 4000001), [100, -100, 88, -88, 1e4, 0.0, -0.6, np.nextafter(np.float32(-0.6), np.float32(0))]]).astype(np.float32)
    y = R.mish32(x)
    assert np.isfinite(y).all()
    want = R.mish64(x.astype(np.float64))
    ok = np.abs(want) > 1.2e-38
    err = np.abs(y[ok].astype(np.float64) - want[ok]) / np.abs(want[ok])
    print('MISH32 max rel err %.3g' % err.max())
    assert err.max() < 1e-6
    assert y[-8] == np.float32(100) and y[-4] == np.float32(1e4) and y[-3] == 0.0 and abs(y[-7]) < 1e-38
    t = torch.from_numpy(x[::37].copy())
    assert np.array_equal(R.mish_torch(t).numpy(), R.mish32(x[::37])) or np.abs(R.mish_torch(t).numpy() - R.mish32(x[::37])).max() < 1e-6


def test_layer_restatement_tells_planted_mistakes_apart():
    """The bound the GPU walk applies to a mish layer (test_gpu_darknet_layers.TOL: relative L2 error <= 0.0042 .. 0.0047) against three
    planted mistakes in the reference step: softplus without tanh, the activation after the shortcut, the activation before the bias."""
    g = torch.Generator().manual_seed(0)
    conv = nn.Conv2d(32, 64, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / 288) ** 0.5)
        conv.bias.copy_(0.3 * torch.randn(64, generator=g))
    x, skip = torch.randn(2, 32, 13, 13, generator=g), torch.randn(2, 64, 13, 13, generator=g)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    with torch.no_grad():
        good = R.layer(x, conv, 'mish', skip)
        assert torch.equal(good, F.mish(conv(x)) + skip)
        assert rel(R.layer(x, conv, 'mish', skip, acts=dict(R.ACTS, mish=R.mish_torch)), good) < 1e-6       # the kernel's form: far inside the bound
        assert rel(good.to(torch.bfloat16).float(), good) < 0.0042                                           # one bf16 rounding passes
        planted = {'softplus without tanh': R.layer(x, conv, 'mish', skip, acts=dict(R.ACTS, mish=lambda t: t * F.softplus(t))),
                   'activation after the shortcut': R.layer(x, conv, 'mish', skip, order='skip_then_act'),
                   'activation before the bias': R.layer(x, conv, 'mish', skip, bias_first=False),
                   'leaky for mish': R.layer(x, conv, 'leaky', skip)}
    for name, bad in planted.items():
        print('PLANTED %s: rel %.3g' % (name, rel(bad, good)))
        assert rel(bad, good) > 10 * 0.0047, name


DECODE_CASES = [
    # n, grids, nc, chan stride, cls, score_thresh, nms_thresh, max_det, logit sigma: the cases of test_gpu_yolo_tiny
    (3, (13, 26), 80, 256, 0, 0.6, 0.45, 64, 1.5), (2, (13, 26), 80, 255, 17, 0.5, 0.3, 8, 1.5), (1, (8, 16), 1, 24, 0, 0.2, 0.5, 100, 1.0),
    (2, (5, 9), 3, 32, 2, 0.999999, 0.45, 16, 1.0), (2, (13,), 80, 256, 0, 0.5, 0.45, 64, 1.5), (1, (52,), 80, 255, 3, 0.6, 0.45, 32, 1.5),
    (3, (13, 26, 52), 80, 256, 0, 0.6, 0.45, 64, 1.5)]


def decode_heads(cfg, seed=3):
    n, grids, nc, cs, cls, st, nt, max_det, sigma = cfg
    rng = np.random.default_rng(seed)
    heads = [Y.bf16_round((rng.standard_normal((n, g, g + 1, cs)) * sigma).astype(np.float32)) for g in grids]
    if grids == (8, 16):
        for h in heads:
            h[..., 4::(5 + nc)] += 4.0; h[..., 5::(5 + nc)] += 4.0
    return heads


def decode_anchors(nh):
    if nh == 2:
        return np.array(yolov3.TINY_ANCHORS, dtype=np.float32).reshape(2, 3, 2)[::-1].copy()
    return np.array(yolov3.ANCHORS, dtype=np.float32).reshape(3, 3, 2)[::-1][:nh].copy()


@pytest.mark.parametrize('cfg', DECODE_CASES)
def test_decode_with_scales_of_one_is_the_oracle(cfg):
    n, grids, nc, cs, cls, st, nt, max_det, sigma = cfg
    heads, anchors = decode_heads(cfg), decode_anchors(len(grids))
    moved = 0
    for i in range(n):
        a, ca = Y.detect([h[i] for h in heads], anchors, 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        b, cb = R.decode([h[i] for h in heads], anchors, [1.0] * len(grids), 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        assert ca == cb and a.tobytes() == b.tobytes()
        c, cc = R.decode([h[i] for h in heads], anchors, [1.2] * len(grids), 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        assert cc == ca                                      # scores do not depend on the scale
        if len(a) and len(c) == len(a):
            moved = max(moved, float(np.abs(c[:, :4] - a[:, :4]).max()))
    if st < 0.99:
        assert moved > 1.0                                   # scale 1.2 moves a centre by up to 0.1 cell: several frame pixels
