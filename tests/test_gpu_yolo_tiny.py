"""GPU: YOLOv3-tiny on the HIP conv stack -- the max-pool kernel bit for bit against torch, the one-to-three-head decode + NMS entry
points against oracle/yolo_ref.py, every step of the tiny plan on its own against the fp32 torch op on the same bf16 input (the method
and the per-family bounds of test_gpu_darknet_layers.py, imported), the whole network against its bf16 floor, and the detector end to
end (cfg / weights files and ``arch='yolov3-tiny'``, graph replay, the ivclabpose facade built from the shipped config)."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_tiny_calibrated as TC
from oracle import yolo_ref as Y
import guarded_mem as G
from test_gpu_darknet_layers import HEAD_FLOOR_RATIO, Checker, Spy, family_of, input_x8, padded_bf16, rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- pam_maxpool_nhwc_bf16 ----------------------------------------------------------------------------------------------------------
POOL_CASES = [((5, 416, 416, 32), 2, 2), ((5, 208, 208, 32), 2, 2), ((2, 104, 104, 64), 2, 2), ((2, 52, 52, 128), 2, 2),
              ((10, 26, 26, 256), 2, 2), ((2, 13, 13, 512), 2, 1), ((1, 31, 23, 8), 2, 2), ((1, 7, 5, 16), 2, 1), ((2, 13, 13, 64), 3, 1)]


def _engine():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.ConvEngine()
    e.lib = _lib.load(); e.device = torch.device(DEV)
    return e


@pytest.mark.parametrize('shape,size,stride', POOL_CASES, ids=['%dx%dx%dx%d-%d-%d' % (s + (k, st)) for s, k, st in POOL_CASES])
def test_maxpool_bit_exact_vs_torch(shape, size, stride):
    """NHWC bf16, Darknet's window (pad = size - 1, start -pad / 2, taps outside the image ignored): the result is one of the inputs, so
    every bit equals torch.max_pool2d on the -inf-padded tensor; the last half of the channels is zero (padding) and stays zero."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(h * 1000 + c)
    real = c - c // 2 if c >= 16 else c
    x = torch.randn((n, real, h, w), generator=g)
    x = torch.cat([x, torch.zeros((n, c - real, h, w))], 1).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    e = _engine()
    e.arena = G.GuardArena(e.device, 2 * x.numel() + (1 << 20))  # the output between sentinel bands (tests/guarded_mem.py)
    y = e.maxpool(x, size, stride)
    lo, hi = (size - 1) // 2, (size - 1) - (size - 1) // 2
    want = F.max_pool2d(F.pad(x.float(), (lo, hi, lo, hi), value=float('-inf')), size, stride)
    torch.cuda.synchronize()
    assert e.arena.report() == ''                                # no write outside y, nothing of y left unwritten
    assert tuple(y.shape) == tuple(want.shape) == (n, c, (h - 1) // stride + 1, (w - 1) // stride + 1)
    if shape == (1, 31, 23, 8):
        assert tuple(y.shape[2:]) == (16, 12)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_bits(y.permute(0, 2, 3, 1)), _bits(want.to(torch.bfloat16).permute(0, 2, 3, 1)))
    if c > real:
        assert float(y[:, real:].float().abs().max()) == 0.0
        assert int(_bits(y[:, real:].permute(0, 2, 3, 1)).abs().max()) == 0          # +0, not -0


def test_maxpool_rejects_bad_arguments():
    from pam import _lib
    lib = _lib.load()
    x = torch.zeros((1, 8, 8, 16), dtype=torch.bfloat16, device=DEV)
    y = torch.full((1, 8, 8, 16), 3.0, dtype=torch.bfloat16, device=DEV)
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    assert lib.pam_maxpool_nhwc_bf16(None, px, py, 1, 8, 8, 12, 2, 2) == -1          # C % 8 != 0
    assert lib.pam_maxpool_nhwc_bf16(None, px, py, 1, 8, 8, 16, 4, 2) == -1          # size
    assert lib.pam_maxpool_nhwc_bf16(None, px, py, 1, 8, 8, 16, 2, 3) == -1          # stride
    assert lib.pam_maxpool_nhwc_bf16(None, None, py, 1, 8, 8, 16, 2, 2) == -1
    assert lib.pam_maxpool_nhwc_bf16(None, px, None, 1, 8, 8, 16, 2, 2) == -1
    assert lib.pam_maxpool_nhwc_bf16(None, px, py, 0, 8, 8, 16, 2, 2) == -1
    torch.cuda.synchronize()
    assert float((y.float() - 3.0).abs().max()) == 0.0                               # nothing was launched
    assert lib.pam_maxpool_nhwc_bf16(None, px, py, 1, 8, 8, 16, 2, 1) == 0
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0


# ---- decode + NMS over one to three heads ----------------------------------------------------------------------------------------------
def _run_heads(heads_np, anchors, net, nc, cls, st, nt, fw, fh, max_det, split, legacy=False):
    """The new entry points (legacy: the three-head ones) on bf16 copies of heads_np -> boxes, count, the bf16 heads as float32."""
    from pam import _lib
    lib = _lib.load()
    n, nh = heads_np[0].shape[0], len(heads_np)
    hd = [torch.from_numpy(h).to(torch.bfloat16).to(DEV).contiguous() for h in heads_np]
    hp = (C.c_void_p * nh)(*[C.c_void_p(h.data_ptr()) for h in hd])
    gh = (C.c_int32 * nh)(*[h.shape[1] for h in hd]); gw = (C.c_int32 * nh)(*[h.shape[2] for h in hd]); cs = (C.c_int32 * nh)(*[h.shape[3] for h in hd])
    an = np.ascontiguousarray(anchors.reshape(-1), dtype=np.float32)
    assert an.size == 6 * nh
    boxes = torch.full((n, max_det, 5), -1.0, dtype=torch.float32, device=DEV)
    count = torch.full((2 * n,), -1, dtype=torch.int32, device=DEV)
    tail = (hp, gh, gw, cs, an.ctypes.data_as(C.c_void_p), net[0], net[1], nc, cls, st, nt, fw, fh, max_det)
    out = (C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr()))
    if legacy:
        assert nh == 3
    if split:
        need = lib.pam_yolo_detect_workspace_bytes(n, gh, gw) if legacy else lib.pam_yolo_detect_heads_workspace_bytes(n, nh, gh, gw)
        assert need > 0
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        fn = (lambda *a: lib.pam_yolo_detect_ws(None, n, *a)) if legacy else (lambda *a: lib.pam_yolo_detect_heads_ws(None, n, nh, *a))
        scratch = (torch.empty_like(boxes), torch.empty_like(count))
        # the SAME workspace twice: the kernel must leave its tickets zero
        assert fn(*tail, C.c_void_p(scratch[0].data_ptr()), C.c_void_p(scratch[1].data_ptr()), C.c_void_p(ws.data_ptr()), need) == 0
        rc = fn(*tail, *out, C.c_void_p(ws.data_ptr()), need)
        assert fn(*tail, *out, C.c_void_p(ws.data_ptr()), need - 1) == -1
        assert fn(*tail, *out, None, need) == -1
        torch.cuda.synchronize()
        assert int(ws[:4 * n].view(torch.int32).abs().sum()) == 0
    else:
        rc = lib.pam_yolo_detect(None, n, *tail, *out) if legacy else lib.pam_yolo_detect_heads(None, n, nh, *tail, *out)
    assert rc == 0
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), count.cpu().numpy(), [h.float().cpu().numpy() for h in hd]


def _anchors(nh):
    from pam import yolov3
    if nh == 2:
        return np.array(yolov3.TINY_ANCHORS, dtype=np.float32).reshape(2, 3, 2)[::-1].copy()
    return np.array(yolov3.ANCHORS, dtype=np.float32).reshape(3, 3, 2)[::-1][:nh].copy()


@pytest.mark.parametrize('cfg', [
    # n, grids, nc, chan stride, cls, score_thresh, nms_thresh, max_det, logit sigma
    (3, (13, 26), 80, 256, 0, 0.6, 0.45, 64, 1.5),          # YOLOv3-tiny's two heads
    (2, (13, 26), 80, 255, 17, 0.5, 0.3, 8, 1.5),           # max_det cap reached
    (1, (8, 16), 1, 24, 0, 0.2, 0.5, 100, 1.0),             # > 1024 candidates are counted, 1024 enter
    (2, (5, 9), 3, 32, 2, 0.999999, 0.45, 16, 1.0),         # nothing passes
    (2, (13,), 80, 256, 0, 0.5, 0.45, 64, 1.5),             # one head
    (1, (52,), 80, 255, 3, 0.6, 0.45, 32, 1.5),             # one head, several scoring runs
    (3, (13, 26, 52), 80, 256, 0, 0.6, 0.45, 64, 1.5),      # three heads through the new entry points
], ids=['two', 'two-cap', 'two-overflow', 'two-none', 'one', 'one-52', 'three'])
@pytest.mark.parametrize('split', [False, True], ids=['one_wg', 'ws'])
def test_yolo_detect_heads_vs_oracle(cfg, split):
    n, grids, nc, cs, cls, st, nt, max_det, sigma = cfg
    rng = np.random.default_rng(3)
    anchors = _anchors(len(grids))
    heads = [(rng.standard_normal((n, g, g + 1, cs)) * sigma).astype(np.float32) for g in grids]      # non-square grids (13 x 14, 26 x 27)
    if grids == (8, 16):
        for h in heads:
            h[..., 4::(5 + nc)] += 4.0; h[..., 5::(5 + nc)] += 4.0
    boxes, count, hq = _run_heads(heads, anchors, (416, 448), nc, cls, st, nt, 1032, 776, max_det, split)
    for i in range(n):
        exp, nfound = Y.detect([h[i] for h in hq], anchors, 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        assert count[n + i] == nfound, (i, count[n + i], nfound)
        assert count[i] == len(exp), (i, count[i], len(exp))
        got = boxes[i, :count[i]]
        assert np.allclose(got, exp, rtol=2e-5, atol=1e-3), np.abs(got - exp).max()
        assert (boxes[i, count[i]:] == -1.0).all()                       # rows past the count are untouched
    if st > 0.99:
        assert (count[:n] == 0).all()
    else:
        assert count[:n].sum() > 0
    if grids == (8, 16):
        assert count[n] > 1024
    if len(grids) == 3:                                                      # the three-head entry points: the same bytes
        b3, c3, _ = _run_heads(heads, anchors, (416, 448), nc, cls, st, nt, 1032, 776, max_det, split, legacy=True)
        assert boxes.tobytes() == b3.tobytes() and count.tobytes() == c3.tobytes()


def test_yolo_detect_heads_rejects_bad_head_counts():
    from pam import _lib
    lib = _lib.load()
    h = torch.zeros((1, 4, 4, 24), dtype=torch.bfloat16, device=DEV)
    hp = (C.c_void_p * 3)(*[C.c_void_p(h.data_ptr())] * 3)
    g = (C.c_int32 * 3)(4, 4, 4); cs = (C.c_int32 * 3)(24, 24, 24)
    an = np.ones(18, dtype=np.float32)
    boxes = torch.zeros((1, 4, 5), dtype=torch.float32, device=DEV); count = torch.zeros(2, dtype=torch.int32, device=DEV)
    for nh in (0, 4, -1):
        assert lib.pam_yolo_detect_heads_workspace_bytes(1, nh, g, g) == -1
        assert lib.pam_yolo_detect_heads(None, 1, nh, hp, g, g, cs, an.ctypes.data_as(C.c_void_p), 64, 64, 3, 0, 0.5, 0.45, 64, 64, 4,
                                         C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr())) == -1
    assert lib.pam_yolo_detect_heads_workspace_bytes(1, 3, g, g) == lib.pam_yolo_detect_workspace_bytes(1, g, g) > 0
    assert 0 < lib.pam_yolo_detect_heads_workspace_bytes(1, 1, g, g) <= lib.pam_yolo_detect_heads_workspace_bytes(1, 3, g, g)


# ---- every step of the tiny plan on its own ---------------------------------------------------------------------------------------------
# (width, height, views)
CASES = [(416, 416, 1), (416, 416, 5), (416, 416, 10), (608, 608, 2), (320, 320, 3), (416, 256, 2)]
CASE_IDS = ['%dx%d-n%d' % c for c in CASES]


class Env(object):
    pass


@pytest.fixture(scope='module')
def env():
    """One executor per input size (packing is per network), TF32 off for the fp32 reference."""
    from pam import _lib, yolov3
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    e = Env()
    e.dev = torch.device(DEV)
    e.nets = {}

    def net(w, h):
        if (w, h) not in e.nets:
            model = TC.calibrated(width=w, height=h)
            hip = yolov3.HipDarknet(model, e.dev)
            hip.lib = Spy(_lib.load())
            convs = {i: c.to(e.dev) for i, c in TC.folded_convs(model).items()}
            e.nets[(w, h)] = (model, hip, convs)
        return e.nets[(w, h)]
    e.net = net
    try:
        yield e
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def walk(e, w, h, n, check):
    """Run the plan step by step on the reference's bf16 inputs (the walk of test_gpu_darknet_layers.py plus the pool step): a conv
    step against the fp32 torch op on the same input, bounded per family; pool and upsample + route steps bitwise; padded output
    channels exactly 0.  -> {(dst, family): launches}."""
    from pam import yolov3
    model, hip, convs = e.net(w, h)
    outs = {-1: input_x8(e, w, h, n, 2000 + 31 * n + w)}
    rec = {}
    for step in hip.plan:
        kind, dst = step[0], step[1]
        hip.lib.calls = []
        with torch.no_grad():
            y = hip.run_step(step, outs)
        torch.cuda.synchronize()
        if kind == 'conv':
            _, _, op, src, act, skip = step
            assert skip is None
            fam = family_of(hip, step, outs[src])
            c = convs[dst]
            with torch.no_grad():
                r = F.conv2d(outs[src][:, :c.in_channels].float(), c.weight, c.bias, c.stride, c.padding)
                r = F.leaky_relu(r, 0.1) if act == 'leaky' else r
            real = c.out_channels
            assert real == hip.real[dst] and y.shape[1] == hip.padded[dst]
            check(fam, 'layer %d' % dst, y[:, :real], r)
            if y.shape[1] > real:
                assert float(y[:, real:].float().abs().max()) == 0.0, ('padded channels of layer %d' % dst)
            outs[dst] = padded_bf16(r, y.shape[1])
            rec[(dst, fam)] = list(hip.lib.calls)
        elif kind == 'pool':
            x = outs[step[2]]
            want = yolov3.darknet_maxpool(x.float(), step[3], step[4]).to(torch.bfloat16)
            assert tuple(y.shape) == tuple(want.shape), (dst, tuple(y.shape), tuple(want.shape))
            assert torch.equal(_bits(y.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1))), 'max-pool of layer %d' % dst
            if y.shape[1] > hip.real[dst]:
                assert float(y[:, hip.real[dst]:].float().abs().max()) == 0.0, ('padded channels of layer %d' % dst)
            outs[dst] = y
            rec[(dst, 'pool')] = ['k_maxpool']
        elif kind == 'upcat':
            a, b = outs[step[2]], outs[step[3]]
            want = torch.cat([F.interpolate(a.float(), scale_factor=2, mode='nearest'), b.float()], 1)
            assert torch.equal(y.float(), want), 'upsample + route of layer %d' % dst
            outs[dst] = y
            rec[(dst, 'upcat')] = list(hip.lib.calls)
        else:                                          # alias, head: the same tensor
            assert kind in ('alias', 'head')
            outs[dst] = outs[step[2]]
    return rec


@pytest.mark.parametrize('w,h,n', CASES, ids=CASE_IDS)
def test_every_tiny_step_vs_fp32(env, w, h, n):
    """Every step of the tiny plan at this input size and view count against the fp32 op on the same bf16 input, within the per-family
    bounds of test_gpu_darknet_layers.TOL (all seven metrics): what differs is the bf16 rounding of one stored output, as there."""
    cid = CASE_IDS[CASES.index((w, h, n))]
    chk = Checker(cid)
    rec = walk(env, w, h, n, chk)
    print('FORMS ' + json.dumps(dict(case=cid, layers=['%d %s: %s' % (d, f, ', '.join(v)) for (d, f), v in sorted(rec.items())])))
    fams = [f for _, f in sorted(rec)]
    assert fams.count('stem') == 1 and fams.count('conv3x3') == 8 and fams.count('conv1x1') == 2 and fams.count('head1x1') == 2
    assert fams.count('pool') == 6 and fams.count('upcat') == 1
    assert rec[(0, 'stem')] == ['k_conv_stem s1 Cout=32']
    chk.done()


# ---- the whole network and the detector ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detector(env, tmp_path_factory):
    from pam import yolov3
    d = str(tmp_path_factory.mktemp('darknet_tiny'))
    cfg, weights = os.path.join(d, 'yolov3-tiny.cfg'), os.path.join(d, 'calibrated-tiny.weights')
    with open(cfg, 'w') as f:
        f.write(yolov3.tiny_cfg())
    TC.calibrated().save_darknet_weights(weights)
    assert os.path.getsize(weights) == 35434956
    det = yolov3.YOLOv3(cfg, weights, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64)
    assert det.weights == weights and det.anchors.shape == (2, 3, 2) and det.size == (416, 416)
    det.test_files = (cfg, weights)
    return det


@pytest.mark.parametrize('n', [2, 5])
def test_tiny_heads_within_the_bf16_floor(env, detector, n):
    """Both heads vs the fp32 network: within HEAD_FLOOR_RATIO (1.1, test_gpu_darknet_layers) of the error that bf16 weights and a bf16
    store after every convolution alone cost on the same images (darknet_tiny_calibrated.storage_forward)."""
    model = TC.calibrated()
    x8 = input_x8(env, 416, 416, n, 77 + n)
    with torch.no_grad():
        heads = detector.net.forward(x8)
        x = x8[:, :3].float()
        ref = TC.storage_forward(model, x, bf16_weights=False, bf16_store=False)
        floor = TC.storage_forward(model, x)
    torch.cuda.synchronize()
    assert len(heads) == 2 and [tuple(h.shape) for h in heads] == [(n, 256, 13, 13), (n, 256, 26, 26)]
    bad = []
    for k, (hd, r, fl) in enumerate(zip(heads, ref, floor)):
        assert float(hd[:, 255:].float().abs().max()) == 0.0
        err, ferr = rel(hd[:, :255].float() - r, r), rel(fl - r, r)
        print('HEAD ' + json.dumps(dict(n=n, head=k, rel=err, floor=ferr, ratio=err / ferr)))
        if not err <= HEAD_FLOOR_RATIO * ferr:
            bad.append('head %d: rel err %.4g > %.2f x the bf16 floor %.4g' % (k, err, HEAD_FLOOR_RATIO, ferr))
    assert not bad, bad


def _check_detector(det, eager, imgs, fw, fh):
    """Graph replay == eager bitwise, boxes == the oracle on the kernel's own heads, sorted by score, single image == element 0."""
    n = len(imgs)
    H, W = det.size
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    b1, c1 = [t.clone() for t in det.detect_dev(frames)]
    b2, c2 = [t.clone() for t in det.detect_dev(frames)]                      # replay
    b3, c3 = [t.clone() for t in eager.detect_dev(frames)]
    torch.cuda.synchronize()
    assert (n, fh, fw) in det._graphs and det._graphs[(n, fh, fw)][0] is not None and eager._graphs[(n, fh, fw)][0] is None
    assert torch.equal(b1, b2) and torch.equal(c1, c2)
    assert torch.equal(b1, b3) and torch.equal(c1, c3)
    x8 = torch.from_numpy(Y.resize_frames(np.stack(imgs), H, W)).to(DEV).permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        hq = [t.permute(0, 2, 3, 1).float().cpu().numpy() for t in det.net.forward(x8)]
    assert len(hq) == 2
    boxes, count = b1.cpu().numpy(), c1.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                       # a random net may exceed the pre-NMS capacity; the oracle caps alike
        res = det(imgs)
        single = det(imgs[0])
    total = 0
    for i in range(n):
        exp, cand = Y.detect([t[i] for t in hq], det.anchors, W, H, det.num_classes, 0, det.score_thresh, det.nms_thresh, fw, fh, det.max_det)
        assert count[n + i] == cand and count[i] == len(exp), (i, count[i], len(exp), count[n + i], cand)
        assert np.allclose(boxes[i, :count[i]], exp, rtol=2e-5, atol=1e-3), np.abs(boxes[i, :count[i]] - exp).max()
        assert res[i].dtype == np.float32 and res[i].shape == (len(exp), 5) and np.array_equal(res[i], boxes[i, :count[i]])
        assert (np.diff(res[i][:, 4]) <= 0).all()
        total += len(exp)
    assert np.array_equal(single, res[0])
    return total


def test_tiny_detector_from_files_replay_and_oracle(env, detector):
    from pam import yolov3
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (416, 416, 3), dtype=np.uint8) for _ in range(5)]
    eager = yolov3.YOLOv3(*detector.test_files, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64, use_graph=False)
    assert _check_detector(detector, eager, imgs, 416, 416) >= 5              # the calibrated network: boxes in every view
    # a cfg file decides the architecture whatever `arch` says
    assert yolov3.YOLOv3(detector.test_files[0], None, None, arch='yolov3').anchors.shape == (2, 3, 2)


def test_tiny_detector_by_arch_keyword():
    from pam import yolov3
    det = yolov3.YOLOv3(None, None, None, score_thresh=0.05, nms_thresh=0.45, use_cuda=True, max_det=32, seed=1, arch='yolov3-tiny')
    eager = yolov3.YOLOv3(None, None, None, score_thresh=0.05, nms_thresh=0.45, use_cuda=True, max_det=32, seed=1, arch='yolov3-tiny', use_graph=False)
    assert det.anchors.shape == (2, 3, 2) and len([s for s in det.net.plan if s[0] == 'pool']) == 6
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(2)]
    _check_detector(det, eager, imgs, 320, 240)
    # the seeded random tiny network against its fp32 form (13 bf16 layers)
    x8 = torch.from_numpy(Y.resize_frames(np.stack(imgs), 416, 416)).to(DEV).permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    model = yolov3.Darknet(yolov3.tiny_cfg()).init_random(1).eval().to(DEV)
    with torch.no_grad():
        ref = model(x8[:, :3].float())
        heads = det.net.forward(x8)
    torch.cuda.synchronize()
    for h, r in zip(heads, ref):
        assert rel(h[:, :255].float() - r, r) < 0.03
    with pytest.raises(ValueError):
        yolov3.YOLOv3(None, None, None, arch='yolov4')
    assert yolov3.YOLOv3(None, None, None, seed=1).anchors.shape == (3, 3, 2)      # the default stays Darknet-53


def _tiny_facade(weights):
    import pam
    from pam import ivclabpose as IV
    from pam.dataset import GetConfig
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_yolov3tiny.yaml'))
    pipe = cfg.PIPELINE_COMBINATION
    assert str(pipe['DETECT_MODEL']) == 'YOLOv3'
    d = dict(cfg.DETECT_MODELS[str(pipe['DETECT_MODEL']).upper()])
    assert d['ARCH'] == 'yolov3-tiny' and d['CFG'].endswith('yolov3-tiny.cfg') and d['WEIGHT'].endswith('yolov3-tiny.weights')
    assert not os.path.exists(d['CFG'])                                   # no cfg file here: ARCH decides
    d['WEIGHT'], d['SCORE_THRESH'], d['NMS_THRESH'] = weights, 0.5, 0.45  # the calibrated test weights: boxes in every view
    api = IV.ivclabpose(person_detector=d, pose_detector=None, person_matcher=None)
    assert api.bbox_detector.anchors.shape == (2, 3, 2) and api.bbox_detector.weights == weights
    return api


def test_tiny_persondetect_facade_format(detector):
    """ivclabpose built from configs/Shelf/model_configs_yolov3tiny.yaml: PersonDetect dicts in the format test_persondetect_facade_format checks."""
    api = _tiny_facade(detector.test_files[1])
    rng = np.random.default_rng(9)
    imgs = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)]
    out = api.PersonDetect(imgs, image_id=7)
    assert len(out) == 3 and sum(len(v) for v in out) > 0
    for persons, im in zip(out, imgs):
        for p in persons:
            assert p['image_id'] == 7 and p['category_id'] == 1 and p['data'] is im and p['feature'] == []
            x, y, w, h = p['bbox']
            assert x >= 0 and y >= 0 and x + w <= 320 + 1e-3 and y + h <= 240 + 1e-3
            assert isinstance(p['score'], float) and round(p['score'], 4) == p['score']


def test_tiny_detection_a_frame_ahead_gives_persondetects_boxes(detector):
    api = _tiny_facade(detector.test_files[1])
    rng = np.random.default_rng(11)
    sets = [[rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)] for _ in range(3)]
    want = [api.PersonDetect(imgs, image_id=k) for k, imgs in enumerate(sets)]
    t0 = api.PersonDetectAhead(sets[0], 0)
    got = []
    for k in range(3):
        nxt = api.PersonDetectAhead(sets[k + 1], k + 1) if k + 1 < 3 else None      # issued BEFORE frame k is collected
        got.append(api.PersonDetectResult(t0))
        t0 = nxt
    strip = lambda frames: [[(p['image_id'], p['bbox'], p['score']) for p in v] for v in frames]
    assert [strip(f) for f in got] == [strip(f) for f in want]
    assert sum(len(v) for f in want for v in f) > 0
