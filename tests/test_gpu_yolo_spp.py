"""GPU: YOLOv3-SPP on the HIP conv stack -- every step of the plan on its own against the fp32 torch op on the same bf16 input (the method
and the per-family bounds of test_gpu_darknet_layers.py, imported; the SPP step bitwise up to the sign of zeros and exactly one launch of
pam_spp_concat_nhwc_bf16), the three heads against the bf16-storage floor, and the detector end to end (cfg / weights files and
``arch='yolov3-spp'``, graph replay against eager and the oracle's boxes, the ivclabpose facade built from the shipped config)."""
import json
import os
import warnings
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_spp_calibrated as SC
import spp_ref as R
from oracle import yolo_ref as Y
from test_gpu_darknet_layers import HEAD_FLOOR_RATIO, TOL, Checker, Spy, family_of, input_x8, padded_bf16, rel  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPP_BYTES = 252209544

# (width, height, views)
CASES = [(416, 416, 2), (416, 416, 5), (608, 608, 1), (320, 320, 3), (416, 256, 2)]
CASE_IDS = ['%dx%d-n%d' % c for c in CASES]


class SppSpy(Spy):
    """test_gpu_darknet_layers.Spy that also records the SPP entry."""

    def __getattr__(self, name):
        if name != 'pam_spp_concat_nhwc_bf16':
            return Spy.__getattr__(self, name)
        fn = getattr(self._lib, name)

        def launch(*args):
            rc = fn(*args)
            self.calls.append('k_spp %d/%d/%d' % tuple(args[-3:]))
            return rc
        return launch


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
            model = SC.calibrated(width=w, height=h)
            hip = yolov3.HipDarknet(model, e.dev)
            hip.lib = SppSpy(_lib.load())
            convs = {i: c.to(e.dev) for i, c in SC.folded_convs(model).items()}
            e.nets[(w, h)] = (model, hip, convs)
        return e.nets[(w, h)]
    e.net = net
    try:
        yield e
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def walk(e, w, h, n, check):
    """test_gpu_darknet_layers.walk plus the SPP step: the plan step by step on the reference's bf16 inputs; a conv step against the fp32
    torch op on the same input, bounded per family; the SPP step against darknet_maxpool + cat on the same bf16 input, bitwise up to the sign
    of zeros; upsample + route steps bitwise; padded output channels exactly 0.  -> {(dst, family): launches}."""
    model, hip, convs = e.net(w, h)
    reads = lambda step: ([step[3]] + ([step[5]] if step[5] is not None else []) if step[0] == 'conv' else
                          [step[2]] if step[0] == 'spp' else list(step[2:]))
    last_use = {}
    for k, step in enumerate(hip.plan):
        for s in reads(step):
            last_use[s] = k
    outs = {-1: input_x8(e, w, h, n, 3000 + 31 * n + w)}
    rec = {}
    for k, step in enumerate(hip.plan):
        kind, dst = step[0], step[1]
        hip.lib.calls = []
        with torch.no_grad():
            y = hip.run_step(step, outs)
        torch.cuda.synchronize()
        if kind == 'conv':
            _, _, op, src, act, skip = step
            fam = family_of(hip, step, outs[src])
            c = convs[dst - 1 if skip is not None else dst]
            with torch.no_grad():
                r = F.conv2d(outs[src][:, :c.in_channels].float(), c.weight, c.bias, c.stride, c.padding)
                r = F.leaky_relu(r, 0.1) if act == 'leaky' else r
                if skip is not None:
                    r = r + outs[skip][:, :c.out_channels].float()
            real = c.out_channels
            assert real == hip.real[dst] and y.shape[1] == hip.padded[dst]
            check(fam, 'layer %d' % dst, y[:, :real], r)
            if y.shape[1] > real:
                assert float(y[:, real:].float().abs().max()) == 0.0, ('padded channels of layer %d' % dst)
            outs[dst] = padded_bf16(r, y.shape[1])
            rec[(dst, fam)] = list(hip.lib.calls)
            del r
        elif kind == 'spp':
            x = outs[step[2]]
            assert x.shape[1] == 512 and tuple(x.shape[2:]) == (h // 32, w // 32) and step[3] == (5, 9, 13)
            want = R.torch_spp(x.float(), step[3]).to(torch.bfloat16)
            assert tuple(y.shape) == tuple(want.shape) == (n, 2048, h // 32, w // 32) and y.is_contiguous(memory_format=torch.channels_last)
            ok = R.same_up_to_zero_sign(y.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1))
            assert bool(ok.all()), 'SPP block of layer %d: %d elements differ' % (dst, int((~ok).sum()))
            assert torch.equal(R.bits(y[:, 1536:].permute(0, 2, 3, 1)), R.bits(x.permute(0, 2, 3, 1)))
            assert hip.lib.calls == ['k_spp 5/9/13'], hip.lib.calls                    # ONE launch of the new entry, nothing else
            outs[dst] = y
            rec[(dst, 'spp')] = list(hip.lib.calls)
        elif kind == 'upcat':
            a, b = outs[step[2]], outs[step[3]]
            want = torch.cat([F.interpolate(a.float(), scale_factor=2, mode='nearest'), b.float()], 1)
            assert torch.equal(y.float(), want), 'upsample + route of layer %d' % dst
            outs[dst] = y
            rec[(dst, 'upcat')] = list(hip.lib.calls)
        else:                                          # alias, head: the same tensor
            assert kind in ('alias', 'head'), kind
            outs[dst] = outs[step[2]]
        del y
        for s in [s for s in outs if last_use.get(s, -1) <= k]:
            del outs[s]
    return rec


@pytest.mark.parametrize('w,h,n', CASES, ids=CASE_IDS)
def test_every_spp_network_step_vs_fp32(env, w, h, n):
    """Every step of the SPP plan at this input size and view count against the fp32 op on the same bf16 input, within the per-family
    bounds of test_gpu_darknet_layers.TOL (all seven metrics, unchanged: the new 2048 -> 512 layer is a conv1x1)."""
    cid = CASE_IDS[CASES.index((w, h, n))]
    chk = Checker(cid)
    rec = walk(env, w, h, n, chk)
    print('FORMS ' + json.dumps(dict(case=cid, layers=['%d %s: %s' % (d, f, ', '.join(v)) for (d, f), v in sorted(rec.items())])))
    fams = Counter(f for _, f in rec)
    assert fams['stem'] == 1 and fams['spp'] == 1 and fams['upcat'] == 2 and fams['head1x1'] == 3
    assert fams['conv3x3s2'] == 5 and fams['conv3x3+shortcut'] + fams['unfused3x3+add'] == 23
    assert fams['conv1x1'] == 23 + 9 + 2 + 1 and fams['conv3x3'] == 9            # Darknet-53's, plus layer 84
    assert (84, 'conv1x1') in rec and len(rec[(84, 'conv1x1')]) == 1 and rec[(83, 'spp')] == ['k_spp 5/9/13']
    assert set(f for _, f in rec) - {'spp', 'upcat'} <= set(TOL)
    chk.done()


# ---- the whole network and the detector ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detector(env, tmp_path_factory):
    from pam import yolov3
    d = str(tmp_path_factory.mktemp('darknet_spp'))
    cfg, weights = os.path.join(d, 'yolov3-spp.cfg'), os.path.join(d, 'calibrated-spp.weights')
    with open(cfg, 'w') as f:
        f.write(yolov3.spp_cfg())
    SC.calibrated().save_darknet_weights(weights)
    assert os.path.getsize(weights) == SPP_BYTES
    det = yolov3.YOLOv3(cfg, weights, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64)
    assert det.weights == weights and det.anchors.shape == (3, 3, 2) and det.size == (416, 416)
    assert [s[1:] for s in det.net.plan if s[0] == 'spp'] == [(83, 77, (5, 9, 13))]
    det.test_files = (cfg, weights)
    return det


@pytest.mark.parametrize('n', [2, 5])
def test_spp_heads_within_the_bf16_floor(env, detector, n):
    """All three heads vs the fp32 network: within HEAD_FLOOR_RATIO (1.1, test_gpu_darknet_layers) of the error that bf16 weights and a
    bf16 store after every layer alone cost on the same images (darknet_spp_calibrated.storage_forward)."""
    model = SC.calibrated()
    x8 = input_x8(env, 416, 416, n, 77 + n)
    with torch.no_grad():
        heads = detector.net.forward(x8)
        x = x8[:, :3].float()
        ref = SC.storage_forward(model, x, bf16_weights=False, bf16_store=False)
        floor = SC.storage_forward(model, x)
    torch.cuda.synchronize()
    assert [tuple(h.shape) for h in heads] == [(n, 256, 13, 13), (n, 256, 26, 26), (n, 256, 52, 52)]
    bad = []
    for k, (hd, r, fl) in enumerate(zip(heads, ref, floor)):
        assert float(hd[:, 255:].float().abs().max()) == 0.0
        err, ferr = rel(hd[:, :255].float() - r, r), rel(fl - r, r)
        print('HEAD ' + json.dumps(dict(n=n, head=k, rel=err, floor=ferr, ratio=err / ferr)))
        if not err <= HEAD_FLOOR_RATIO * ferr:
            bad.append('head %d: rel err %.4g > %.2f x the bf16 floor %.4g' % (k, err, HEAD_FLOOR_RATIO, ferr))
    assert not bad, bad


def _check_detector(det, eager, imgs, fw, fh):
    """Graph replay == eager bitwise, boxes == the oracle on the kernel's own (eager) heads, index-exact, sorted by score, single image ==
    element 0.  -> boxes per image."""
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
        hq = [t.permute(0, 2, 3, 1).float().cpu().numpy() for t in eager.net.forward(x8)]
    assert len(hq) == 3
    boxes, count = b1.cpu().numpy(), c1.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                       # a random net may exceed the pre-NMS capacity; the oracle caps alike
        res = det(imgs)
        single = det(imgs[0])
    per = []
    for i in range(n):
        exp, cand = Y.detect([t[i] for t in hq], det.anchors, W, H, det.num_classes, 0, det.score_thresh, det.nms_thresh, fw, fh, det.max_det)
        assert count[n + i] == cand and count[i] == len(exp), (i, count[i], len(exp), count[n + i], cand)
        assert np.allclose(boxes[i, :count[i]], exp, rtol=2e-5, atol=1e-3), np.abs(boxes[i, :count[i]] - exp).max()
        assert res[i].dtype == np.float32 and res[i].shape == (len(exp), 5) and np.array_equal(res[i], boxes[i, :count[i]])
        assert (np.diff(res[i][:, 4]) <= 0).all()
        per.append(len(exp))
    assert np.array_equal(single, res[0])
    return per


def test_spp_detector_from_files_replay_and_oracle(env, detector):
    from pam import yolov3
    imgs = SC.test_images()
    eager = yolov3.YOLOv3(*detector.test_files, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64, use_graph=False)
    per = _check_detector(detector, eager, imgs, 416, 416)
    print('BOXES ' + json.dumps(per))
    assert all(1 <= k <= 64 for k in per), per                                # the calibrated network: boxes in every view
    # a cfg file decides the architecture whatever `arch` says
    det = yolov3.YOLOv3(detector.test_files[0], None, None, arch='yolov3-tiny')
    assert det.anchors.shape == (3, 3, 2) and len([s for s in det.net.plan if s[0] == 'spp']) == 1


def test_spp_detector_by_arch_keyword():
    from pam import yolov3
    kw = dict(score_thresh=0.05, nms_thresh=0.45, use_cuda=True, max_det=32, seed=1, arch='yolov3-spp')
    det = yolov3.YOLOv3(None, None, None, **kw)
    eager = yolov3.YOLOv3(None, None, None, use_graph=False, **kw)
    assert det.anchors.shape == (3, 3, 2) and [s[1:] for s in det.net.plan if s[0] == 'spp'] == [(83, 77, (5, 9, 13))]
    assert det.weights == 'random(seed=1)' and len([s for s in det.net.plan if s[0] == 'conv']) == 76
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(2)]
    _check_detector(det, eager, imgs, 320, 240)
    with pytest.raises(ValueError):
        yolov3.YOLOv3(None, None, None, arch='yolov3-spp-tiny')


def _spp_facade(weights):
    import pam
    from pam import ivclabpose as IV
    from pam.dataset import GetConfig
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_yolov3spp.yaml'))
    pipe = cfg.PIPELINE_COMBINATION
    assert str(pipe['DETECT_MODEL']) == 'YOLOv3'
    d = dict(cfg.DETECT_MODELS[str(pipe['DETECT_MODEL']).upper()])
    assert d['ARCH'] == 'yolov3-spp' and d['CFG'].endswith('yolov3-spp.cfg') and d['WEIGHT'].endswith('yolov3-spp.weights')
    assert not os.path.exists(d['CFG'])                                   # no cfg file here: ARCH decides
    d['WEIGHT'], d['SCORE_THRESH'], d['NMS_THRESH'] = weights, 0.5, 0.45  # the calibrated test weights: boxes in every view
    api = IV.ivclabpose(person_detector=d, pose_detector=None, person_matcher=None)
    assert api.bbox_detector.anchors.shape == (3, 3, 2) and api.bbox_detector.weights == weights
    assert len([s for s in api.bbox_detector.net.plan if s[0] == 'spp']) == 1
    return api


def test_spp_persondetect_facade_format_and_a_frame_ahead(detector):
    """ivclabpose built from configs/Shelf/model_configs_yolov3spp.yaml: PersonDetect dicts in the format test_persondetect_facade_format
    checks, and PersonDetectAhead / PersonDetectResult (frame t + 1 issued before frame t is collected) return PersonDetect's boxes."""
    api = _spp_facade(detector.test_files[1])
    rng = np.random.default_rng(9)
    sets = [[rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)] for _ in range(3)]
    want = [api.PersonDetect(imgs, image_id=k) for k, imgs in enumerate(sets)]
    assert sum(len(v) for v in want[0]) > 0
    for persons, im in zip(want[0], sets[0]):
        for p in persons:
            assert p['image_id'] == 0 and p['category_id'] == 1 and p['data'] is im and p['feature'] == []
            x, y, w, h = p['bbox']
            assert x >= 0 and y >= 0 and x + w <= 320 + 1e-3 and y + h <= 240 + 1e-3
            assert isinstance(p['score'], float) and round(p['score'], 4) == p['score']
    t0 = api.PersonDetectAhead(sets[0], 0)
    got = []
    for k in range(3):
        nxt = api.PersonDetectAhead(sets[k + 1], k + 1) if k + 1 < 3 else None      # issued BEFORE frame k is collected
        got.append(api.PersonDetectResult(t0))
        t0 = nxt
    strip = lambda frames: [[(p['image_id'], p['bbox'], p['score']) for p in v] for v in frames]
    assert [strip(f) for f in got] == [strip(f) for f in want]
    assert sum(len(v) for f in want for v in f) > 0
