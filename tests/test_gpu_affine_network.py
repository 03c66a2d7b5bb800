"""GPU: box_transform='affine' through HRNetPose.predict and FramePipeline -- HRNet-W32 at 256 x 192 with seeded weights, 2 views x 2
persons on 131 x 97 frames.  predict() against the manual composition preprocess(eff=) -> features -> head_decode(eff), the keypoints
inside their effective boxes, the dump's raw boxes, pose_step against predict (also under flip_test + dark), the OKS-NMS on effective
areas on a doubled person whose fate the two area rules decide differently, and the default 'stretch' calling neither new entry."""
import functools

import numpy as np
import pytest
import torch

import affine_ref as A
import pose_nms_ref as P
from image_ref import noise_frames

pytestmark = pytest.mark.gpu

J = 17
FRAME = (131, 97)
RES = (256, 192)
MD = 2
# thin and flat boxes: the raw box covers a small share of its effective box, so keypoints outside it are certain among 68
BOXES = [[[30.0, 20.0, 9.0, 70.0], [50.5, 60.25, 40.0, 12.0]], [[10.0, 40.0, 60.0, 14.0], [70.25, 15.5, 8.0, 90.0]], []]
# the doubled person: a box at the aspect whose effective box (5.5, 6, 45, 60) samples the frame at multiples of 1/64, and the same
# box 2 pixels to the right, on a frame of period 2 along x: the two crops are the same bits, so the second person's keypoints are the
# first one's + 2 in x whatever the network computes.  OKS of such a pair (tests/pose_nms_ref.py, worked out on the CPU): 0.8794 with the
# raw areas 36 * 48, 0.9187 with the effective areas 45 * 60 -- at OKS_THRE 0.9 the raw rule keeps both, the official rule drops one.
TWIN = [[[10.0, 12.0, 36.0, 48.0], [12.0, 12.0, 36.0, 48.0]], [[10.0, 40.0, 60.0, 14.0]], []]


@functools.lru_cache(maxsize=None)
def rig():
    from test_gpu_pipeline import _rig
    seq, cams, cfg, conf, meta = _rig('S1')
    assert len(cams) == 3
    return cams, cfg, conf


def pipeline(**kw):
    from pam.pipeline import FramePipeline
    cams, cfg, conf = rig()
    return FramePipeline(cams, dict(cfg), conf, FRAME, max_dets=MD, autotune=False, width=32, resolution=RES, **kw)


@pytest.fixture(scope='module')
def affine_pipe():
    return pipeline(box_transform='affine')


@pytest.fixture(scope='module')
def frames():
    fr = noise_frames(3, FRAME[0], FRAME[1], 17)
    return [torch.from_numpy(f).cuda() for f in fr]


def pbl(frames, boxes):
    return [[dict(image_id=0, category_id=1, score=0.9, bbox=list(b), data=frames[v], feature=[]) for b in bs] for v, bs in enumerate(boxes)]


def tables(boxes, dev):
    vl = [v for v, bs in enumerate(boxes) for _ in bs]
    sl = [s for bs in boxes for s in range(len(bs))]
    bx = np.asarray([b for bs in boxes for b in bs], dtype=np.float32)
    t = lambda a, d: torch.tensor(a, dtype=d, device=dev)
    return t(vl, torch.int32), t(sl, torch.int32), torch.from_numpy(bx).to(dev), t([len(bs) for bs in boxes], torch.int32), vl, sl, bx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_predict_is_the_manual_composition_and_the_keypoints_come_back_through_the_effective_box(affine_pipe, frames):
    net = affine_pipe.net
    assert net.box_transform == 'affine' and net.box_scale == 1.25 and net.width == 32
    dev = net.device
    dump = net.predict(pbl(frames, BOXES))
    view_of, slot_of, bx, cnt, vl, sl, boxes = tables(BOXES, dev)
    n = len(vl)
    want_eff = A.box_cs64(boxes, RES[1], RES[0])
    assert np.array_equal(bits(dump.device_eff.cpu().numpy()), bits(want_eff))
    # the manual composition, into buffers of its own
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    x = net.input_buffer(4)
    eff = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    net.preprocess(ptrs, FRAME[0], FRAME[1], view_of, bx, x, eff=eff)
    f = net.features(x)
    det = torch.zeros_like(dump.device_det); kp = torch.zeros((n, J, 3), dtype=torch.float32, device=dev)
    net.head_decode(f, view_of, slot_of, eff, det, kp, n=n)
    torch.cuda.synchronize()
    assert torch.equal(eff, dump.device_eff)
    for v, s in zip(vl, sl):
        assert torch.equal(dump.device_det[v, s], det[v, s]), (v, s)
    listed = np.asarray([it['keypoints'] for v in dump for it in v], dtype=np.float32).reshape(n, J, 3)
    assert np.array_equal(listed, kp.cpu().numpy())
    # every keypoint inside its effective box, at least one outside its raw box; the dump's bbox is the caller's
    e = want_eff.astype(np.float64)
    xs, ys = listed[:, :, 0].astype(np.float64), listed[:, :, 1].astype(np.float64)
    assert np.all(xs >= e[:, None, 0]) and np.all(xs <= e[:, None, 0] + e[:, None, 2])
    assert np.all(ys >= e[:, None, 1]) and np.all(ys <= e[:, None, 1] + e[:, None, 3])
    b = boxes.astype(np.float64)
    outside = (xs < b[:, None, 0]) | (xs > b[:, None, 0] + b[:, None, 2]) | (ys < b[:, None, 1]) | (ys > b[:, None, 1] + b[:, None, 3])
    assert outside.any()
    assert [[it['bbox'] for it in v] for v in dump] == BOXES
    # a stretch decode of the same features lands elsewhere: the option reaches the decode
    det2 = torch.zeros_like(det)
    net.head_decode(f, view_of, slot_of, bx, det2, None, n=n)
    assert not torch.equal(det2, det)


def test_pose_step_writes_what_predict_writes(affine_pipe, frames):
    pipe, net = affine_pipe, affine_pipe.net
    dev = net.device
    assert pipe.eff_table is not None and pipe.eff_table[0].shape[0] >= 3 * MD
    dump = net.predict(pbl(frames, BOXES))
    view_of, slot_of, bx, cnt, vl, sl, boxes = tables(BOXES, dev)
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    pipe.det_local.zero_()
    with pipe.frame():
        pipe.pose_step(ptrs, view_of, slot_of, bx)
    torch.cuda.synchronize()
    for v, s in zip(vl, sl):
        assert torch.equal(pipe.det_local[v, s], dump.device_det[v, s]), (v, s)
    assert np.array_equal(bits(pipe.eff_table[0][:len(vl)].cpu().numpy()), bits(A.box_cs64(boxes, RES[1], RES[0])))
    assert torch.equal(bx.cpu(), torch.from_numpy(boxes))                # the caller's table is not written


def test_pose_step_writes_what_predict_writes_under_flip_test_and_dark(frames):
    pipe = pipeline(box_transform='affine', flip_test=True, dark=True)
    net = pipe.net
    assert net.flip_test and net.dark and net.box_transform == 'affine'
    dev = net.device
    dump = net.predict(pbl(frames, BOXES))
    view_of, slot_of, bx, cnt, vl, sl, boxes = tables(BOXES, dev)
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    pipe.det_local.zero_()
    with pipe.frame():
        pipe.pose_step(ptrs, view_of, slot_of, bx)
    torch.cuda.synchronize()
    x = net.input_buffer(4)
    xb = x.permute(0, 2, 3, 1).contiguous().view(torch.int16)
    assert torch.equal(xb[4:8], xb[:4].flip(2))                             # the mirrors of the affine crops
    for v, s in zip(vl, sl):
        assert torch.equal(pipe.det_local[v, s], dump.device_det[v, s]), (v, s)
    assert np.array_equal(bits(dump.device_eff.cpu().numpy()), bits(A.box_cs64(boxes, RES[1], RES[0])))
    assert torch.equal(pipe.eff_table[0][:len(vl)], dump.device_eff)


def twin_frames(dev):
    fr = noise_frames(3, FRAME[0], FRAME[1], 23).copy()
    fr[0] = fr[0][:, np.arange(FRAME[1]) % 2]                               # view 0: period 2 along x
    return [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in fr]


def test_oks_nms_takes_the_effective_areas(affine_pipe):
    net = affine_pipe.net
    dev = net.device
    fr = twin_frames(dev)
    view_of, slot_of, bx, cnt, vl, sl, boxes = tables(TWIN, dev)
    assert not net.pose_nms
    plain = net.predict(pbl(fr, TWIN))
    det = plain.device_det.cpu().numpy()
    # the design of the case holds on the device: the twin's keypoints are the first person's + 2 in x, same scores
    assert np.array_equal(det[0, 1, :, 0], det[0, 0, :, 0]) and np.array_equal(det[0, 1, :, 2], det[0, 0, :, 2])
    assert np.abs(det[0, 1, :, 1] - det[0, 0, :, 1] - 2.0).max() < 1e-4
    eff = A.box_cs64(boxes, RES[1], RES[0])
    S = det.shape[1]
    score = np.full((3, S), 0.9, dtype=np.float32)
    want = P.apply(det, [2, 1, 0], S, P.areas_from_rows(3, S, vl, sl, eff), score)
    raw = P.apply(det, [2, 1, 0], S, P.areas_from_rows(3, S, vl, sl, boxes), score)
    assert want['n_det_out'].tolist() == [1, 1, 0] and raw['n_det_out'].tolist() == [2, 1, 0]      # the two rules decide differently
    assert P.threshold_margin(want['oks'], 0.9) > 0.01 and P.threshold_margin(raw['oks'], 0.9) > 0.01
    net.pose_nms = True
    try:
        dump = net.predict(pbl(fr, TWIN))
        got_n = dump.device_n_det.cpu().numpy()
        assert got_n.tolist() == want['n_det_out'].tolist()
        assert np.array_equal(dump.device_det.cpu().numpy()[0, 0], want['det'][0, 0])
        assert [len(v) for v in dump] == [1, 1, 0] and dump[0][0]['bbox'] == TWIN[0][0]
        assert dump._kept() == [[0], [0], []]
    finally:
        net.pose_nms = False
    # the pipeline's filter behind pose_step, on the same network
    from pam.pipeline import FramePipeline
    cams, cfg, conf = rig()
    pipe = FramePipeline(cams, dict(cfg), conf, FRAME, max_dets=MD, net=net, pose_nms=True)
    ptrs = torch.tensor([f.data_ptr() for f in fr], dtype=torch.int64, device=dev)
    with pipe.frame():
        pipe.pose_step(ptrs, view_of, slot_of, bx, n_det=cnt)
    torch.cuda.synchronize()
    assert pipe.nms_n_det.cpu().tolist() == [1, 1, 0]
    assert pipe.nms_keep_from.cpu().numpy()[:, 0].tolist() == [0, 0, -1]


def test_stretch_is_the_default_and_calls_neither_new_entry(frames, monkeypatch):
    """An object built without the new arguments and one built with box_transform='stretch' give the same bits through predict() and
    pose_step, with both new bindings replaced by functions that raise."""
    stock = pipeline()
    named = pipeline(box_transform='stretch', box_scale=1.25)
    lib = stock.net.lib
    assert lib is named.net.lib

    def refuse(*a, **k):
        raise AssertionError('a new entry point was called under box_transform=stretch')
    monkeypatch.setattr(lib, 'pam_preprocess_crops_affine', refuse)
    monkeypatch.setattr(lib, 'pam_box_cs', refuse)
    with pytest.raises(AssertionError):
        lib.pam_box_cs()
    dev = stock.net.device
    view_of, slot_of, bx, cnt, vl, sl, boxes = tables(BOXES, dev)
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    outs = []
    for pipe in (stock, named):
        assert pipe.net.box_transform == 'stretch' and pipe.eff_table is None
        dump = pipe.net.predict(pbl(frames, BOXES))
        assert dump.device_eff is None
        pipe.det_local.zero_()
        with pipe.frame():
            pipe.pose_step(ptrs, view_of, slot_of, bx)
        torch.cuda.synchronize()
        for v, s in zip(vl, sl):
            assert torch.equal(pipe.det_local[v, s], dump.device_det[v, s])
        outs.append((dump.device_det.clone(), pipe.det_local.clone(), [[it['keypoints'] for it in v] for v in dump]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    # and the stretch decode maps through the raw box: keypoints never leave it
    k = np.asarray([kp for v in outs[0][2] for kp in v]).reshape(len(vl), J, 3)
    b = boxes.astype(np.float64)
    assert np.all(k[:, :, 0] >= b[:, None, 0]) and np.all(k[:, :, 0] <= b[:, None, 0] + b[:, None, 2])
    with pytest.raises(ValueError):
        from pam import hrnet
        hrnet.HRNetPose(32, 17, None, resolution=RES, box_transform='letterbox')
