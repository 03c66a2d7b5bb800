"""CPU: the YOLOv3-tiny network definition (yolov3.tiny_cfg / parse_cfg / Darknet's [maxpool]), its Darknet .weights file, the
oracle's decode on two heads and the calibrated test network of darknet_tiny_calibrated.py.  No GPU."""
import os
from collections import Counter

import numpy as np
import pytest
import torch

import darknet_tiny_calibrated as TC
from oracle import yolo_ref as Y
from pam import yolov3

TINY_FLOATS = 8858734
TINY_BYTES = 20 + 4 * TINY_FLOATS          # 35 434 956: the size of the public yolov3-tiny.weights


def test_tiny_cfg_layer_table():
    net, layers = yolov3.parse_cfg(yolov3.tiny_cfg())
    assert len(layers) == 24
    assert Counter(b['type'] for b in layers) == {'convolutional': 13, 'maxpool': 6, 'yolo': 2, 'route': 2, 'upsample': 1}
    convs = [(b['filters'], b['size'], b['stride'], b['batch_normalize'], b['activation']) for b in layers if b['type'] == 'convolutional']
    assert convs == ([(f, 3, 1, 1, 'leaky') for f in (16, 32, 64, 128, 256, 512, 1024)] +
                     [(256, 1, 1, 1, 'leaky'), (512, 3, 1, 1, 'leaky'), (255, 1, 1, 0, 'linear'),
                      (128, 1, 1, 1, 'leaky'), (256, 3, 1, 1, 'leaky'), (255, 1, 1, 0, 'linear')])
    assert [(b['size'], b['stride']) for b in layers if b['type'] == 'maxpool'] == [(2, 2)] * 5 + [(2, 1)]
    assert [i for i, b in enumerate(layers) if b['type'] == 'maxpool'] == [1, 3, 5, 7, 9, 11]
    assert layers[16]['type'] == 'yolo' and layers[16]['mask'] == [3, 4, 5] and layers[23]['mask'] == [0, 1, 2]
    assert layers[16]['anchors'] == [(10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319)]
    assert layers[17]['layers'] == [-4] and layers[19]['type'] == 'upsample' and layers[20]['layers'] == [-1, 8]
    assert int(net['width']) == 416 and int(net['height']) == 416


def test_maxpool_cfg_defaults_and_padding():
    head = '[net]\nwidth=32\nheight=32\nchannels=3\n'
    head += '[convolutional]\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n'
    _, layers = yolov3.parse_cfg(head + '[maxpool]\n')
    assert layers[1]['size'] == 1 and layers[1]['stride'] == 1
    _, layers = yolov3.parse_cfg(head + '[maxpool]\nsize=3\nstride=2\npadding=2\n')
    assert (layers[1]['size'], layers[1]['stride']) == (3, 2)
    with pytest.raises(NotImplementedError):
        yolov3.parse_cfg(head + '[maxpool]\nsize=2\nstride=2\npadding=0\n')
    with pytest.raises(NotImplementedError, match='first layer'):          # a pool must have a layer to pool
        yolov3.parse_cfg('[net]\nwidth=32\nheight=32\nchannels=3\n[maxpool]\nsize=2\nstride=2\n')
    with pytest.raises(NotImplementedError):
        yolov3.parse_cfg(head + '[avgpool]\n')


@pytest.mark.parametrize('width,height', [(416, 416), (320, 320), (608, 608), (416, 256)])
def test_tiny_head_shapes(width, height):
    m = yolov3.Darknet(yolov3.tiny_cfg(width, height)).init_random(0).eval()
    with torch.no_grad():
        heads = m(torch.rand((1, 3, height, width), generator=torch.Generator().manual_seed(1)))
    assert [tuple(h.shape) for h in heads] == [(1, 255, height // 32, width // 32), (1, 255, height // 16, width // 16)]
    assert all(bool(torch.isfinite(h).all()) for h in heads)


def loop_maxpool(x, size, stride):
    """Darknet's forward_maxpool_layer restated: pad = size - 1, offsets -pad / 2, out = (in + pad - size) / stride + 1, taps outside
    the image skipped."""
    n, c, h, w = x.shape
    pad = size - 1
    off = -(pad // 2)
    ho, wo = (h + pad - size) // stride + 1, (w + pad - size) // stride + 1
    out = np.full((n, c, ho, wo), -np.inf, dtype=np.float32)
    for i in range(ho):
        for j in range(wo):
            for dy in range(size):
                for dx in range(size):
                    y, xx = off + i * stride + dy, off + j * stride + dx
                    if 0 <= y < h and 0 <= xx < w:
                        out[:, :, i, j] = np.maximum(out[:, :, i, j], x[:, :, y, xx])
    return out


@pytest.mark.parametrize('size', [2, 3])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('hw', [(13, 13), (31, 23), (26, 26), (8, 5)])
def test_darknet_maxpool_equals_the_loop_restatement(size, stride, hw):
    x = torch.randn((2, 3) + hw, generator=torch.Generator().manual_seed(size * 10 + stride))
    got = yolov3.darknet_maxpool(x, size, stride).numpy()
    want = loop_maxpool(x.numpy(), size, stride)
    assert got.shape == want.shape == (2, 3, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1)
    assert np.array_equal(got, want)
    if size == 2 and stride == 2 and hw == (31, 23):
        assert got.shape[2:] == (16, 12)
    # the same through the Darknet layer, behind a 1x1 convolution set to the identity
    cfg = ('[net]\nwidth=%d\nheight=%d\nchannels=3\n[convolutional]\nfilters=3\nsize=1\nstride=1\npad=1\nactivation=linear\n'
           '[maxpool]\nsize=%d\nstride=%d\n[yolo]\nmask=0,1,2\nanchors=1,1,2,2,3,3\nclasses=1\n' % (hw[1], hw[0], size, stride))
    m = yolov3.Darknet(cfg).eval()
    with torch.no_grad():
        m.mods[0].conv.weight.copy_(torch.eye(3).reshape(3, 3, 1, 1)); m.mods[0].conv.bias.zero_()
        assert np.array_equal(m(x)[0].numpy(), want)


def test_tiny_weights_file_size_and_round_trip(tmp_path):
    m = yolov3.Darknet(yolov3.tiny_cfg()).init_random(3)
    path = str(tmp_path / 'tiny.weights')
    m.save_darknet_weights(path)
    assert os.path.getsize(path) == TINY_BYTES == 35434956
    m2 = yolov3.Darknet(yolov3.tiny_cfg(320, 320))                 # the weights do not depend on the input size
    m2.load_darknet_weights(path)
    sd, sd2 = m.state_dict(), m2.state_dict()
    for k in sd:
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(sd[k], sd2[k]), k
    with pytest.raises(ValueError):
        yolov3.Darknet().load_darknet_weights(path)                # the tiny file into Darknet-53


def test_init_random_biases_the_two_heads():
    m = yolov3.Darknet(yolov3.tiny_cfg()).init_random(0)
    heads = [mm for mm, b in zip(m.mods, m.layers) if b['type'] == 'convolutional' and not b['batch_normalize']]
    assert len(heads) == 2
    for h in heads:
        assert float(h.conv.bias.detach()[4::85].mean()) < -1.5 and abs(float(h.conv.bias.detach()[0::85].mean())) < 0.5


def test_oracle_detect_takes_two_heads():
    rng = np.random.default_rng(5)
    anchors = np.array(yolov3.TINY_ANCHORS, dtype=np.float32).reshape(2, 3, 2)[::-1].copy()
    heads = [(rng.standard_normal((g, g + 1, 255)) * 1.5).astype(np.float32) for g in (13, 26)]
    boxes, nfound = Y.detect(heads, anchors, 416, 448, 80, 0, 0.5, 0.45, 1032, 776, 64)
    assert boxes.shape[1] == 5 and 0 < len(boxes) <= 64 and nfound >= len(boxes)
    assert (np.diff(boxes[:, 4]) <= 0).all()
    # the second head alone gives the candidates the pair has after the first head's
    b0, n0 = Y.detect(heads[:1], anchors[:1], 416, 448, 80, 0, 0.5, 0.45, 1032, 776, 64)
    b1, n1 = Y.detect(heads[1:], anchors[1:], 416, 448, 80, 0, 0.5, 0.45, 1032, 776, 64)
    assert n0 + n1 == nfound


def test_executor_refuses_an_unsupported_maxpool():
    """size = 5 parses (YOLOv3-SPP's pools) but the max-pool kernel takes 2 and 3 only: the executor says so when it is built."""
    cfg = ('[net]\nwidth=64\nheight=64\nchannels=3\n[convolutional]\nbatch_normalize=1\nfilters=32\nsize=3\nstride=1\npad=1\nactivation=leaky\n'
           '[maxpool]\nsize=5\nstride=1\n[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n'
           '[yolo]\nmask=0,1,2\nanchors=1,1,2,2,3,3\nclasses=1\n')
    m = yolov3.Darknet(cfg).init_random(0).eval()
    assert m.layers[1]['size'] == 5
    with torch.no_grad():
        assert tuple(m(torch.rand(1, 3, 64, 64))[0].shape) == (1, 18, 64, 64)
    with pytest.raises(NotImplementedError, match='maxpool'):
        yolov3.HipDarknet(m, torch.device('cpu'))


def test_tiny_plan_and_channel_padding():
    """The executor's plan for the standard tiny cfg (host logic: packs on the CPU): 13 conv steps, 6 pool steps, the route alias, one
    upsample + route, 2 heads; the 16-filter first layer is the stem kernel's 32-channel form with 16 zero filters."""
    m = yolov3.Darknet(yolov3.tiny_cfg()).init_random(0).eval()
    hip = yolov3.HipDarknet(m, torch.device('cpu'))
    assert Counter(s[0] for s in hip.plan) == {'conv': 13, 'pool': 6, 'alias': 1, 'upcat': 1, 'head': 2}
    assert [s[1:] for s in hip.plan if s[0] == 'pool'] == [(1, 0, 2, 2), (3, 2, 2, 2), (5, 4, 2, 2), (7, 6, 2, 2), (9, 8, 2, 2), (11, 10, 2, 1)]
    op0 = hip.plan[0][2]
    assert (op0.cin, op0.cout) == (8, 32) and op0._stem is not None
    assert hip.real[:3] == [16, 16, 32] and hip.padded[:3] == [32, 32, 64]
    assert hip.real[20] == hip.padded[20] == 384 and hip.real[15] == 255 and hip.padded[15] == 256
    # the zero filters of layer 0 and the zero input channels of layer 2
    assert float(op0.bias[16:].abs().max()) == 0.0 and float(op0.bias[:16].abs().min()) > 0.0
    assert float(hip.plan[2][2].w[:, :288].float().reshape(64, 9, 32)[:, :, 16:].abs().max()) == 0.0


def test_calibrated_tiny_is_deterministic_and_bounded():
    m = TC.calibrated()
    again = TC._build(TC.SEED)
    for (k, a), b in zip(m.state_dict().items(), again.state_dict().values()):
        assert torch.equal(a, b), k
    x = TC.images((2, 3, 416, 416), 99)
    trace = []
    heads = TC.storage_forward(m, x, trace=trace)
    assert len(trace) == 13 and [tuple(h.shape) for h in heads] == [(2, 255, 13, 13), (2, 255, 26, 26)]
    # every BN output has per-channel std gamma <= 1.5 and mean beta ~ N(0, 0.3) on the calibration batch, leaky-ReLU only shrinks:
    # rms <= sqrt(1.5^2 + (4 * 0.3)^2) = 1.9 there; twice that is allowed on other images of the same distribution
    for i, t in trace[:-1]:
        if m.layers[i]['batch_normalize']:
            assert bool(torch.isfinite(t).all()) and float(t.pow(2).mean().sqrt()) < 3.8, (i, float(t.pow(2).mean().sqrt()))
    ref = TC.storage_forward(m, x, bf16_weights=False, bf16_store=False)
    for h, r in zip(heads, ref):
        assert float((h - r).norm() / r.norm()) < 0.03
    per = TC.boxes_per_image(m, ref)
    print('tiny calibrated boxes (kept, candidates):', per)
    assert all(5 <= cand <= 200 and kept >= 1 for kept, cand in per), per
