"""GPU: the lens step behind the decode, through HRNetPose.predict and the façade.  The same box list with and without
``camera_parameter['distCoef']``: the tracker's device buffer of the on run is tests/lens_ref.py's inverse of the off run's buffer (within
1e-9 px), the host dicts and ``pts`` are the off run's bit for bit (raw-image pixels), the calls into the library are the off run's plus
one pam_undistort_keypoints -- behind pam_pose_nms when that is on -- and the off run makes the calls it made before the option existed.
HRNet-W32 at 256 x 192, random weights, 5 crops."""
import numpy as np
import pytest
import torch

import lens_ref as L
from pam import synth
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

H, W = 288, 360
ROWS = [[([20.0, 30.0, 80.0, 160.0], 0.9), ([200.0, 60.0, 100.0, 200.0], 0.7)], [([10.0, 20.0, 90.0, 180.0], 0.8)],
        [([120.0, 40.0, 90.0, 180.0], 0.9), ([220.0, 50.0, 110.0, 220.0], 0.6)]]


@pytest.fixture(scope='module')
def w32():
    from pam import hrnet
    net = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_dets=8, autotune=False)
    for n in (4, 6, 8):                                  # every forward these tests can replay is captured (and its form settled) up
        for _ in range(3):                               # front: the calls of a step are then the same from one run to the next
            net.features(net.input_buffer(n))
    torch.cuda.synchronize()
    return net


def _model(w32, dist):
    from pam.ivclabpose import ivclabpose
    seq = synth.make_sequence('S1', n_frames=1, seed=3)
    cfg = dict(synth.MATCHER_CFG['Shelf']); cfg.pop('CONF_THRESHOLD')
    cfg.update(EPI_THRESHOLD=1e6, INIT_THRESHOLD=1e6, JOINT_THRESHOLD=1e6)       # random weights decode no people: every pair is consistent
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), -1e6, max_dets=8)
    model.pose_model = w32
    model.tracker.set_input_guard(w32)
    calib = dict(seq['calib'])
    if dist is not None:
        calib['distCoef'] = dist
    cams = model.GetCameraParameters(calib, W, H)
    return model, cams


def _frame(model, t, nms):
    rng = np.random.default_rng(100 + t)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3)]
    pbl = [[dict(image_id=0, category_id=1, score=s, bbox=list(b), data=frames[v], feature=[]) for b, s in view] for v, view in enumerate(ROWS)]
    model.pose_model.pose_nms = nms
    with recorded_calls() as calls:
        dump = model.PersonPoseDetect(person_bbox_list=pbl, batch_size=20)
    n_det, det = dump.device_n_det.cpu().numpy().copy(), dump.device_det.cpu().numpy().copy()
    tup = model.PersonTrack_Project3DPose(t, pbl, dump, 'SVD')
    return dict(n_det=n_det, det=det, lists=[[dict(it) for it in v] for v in dump], poses=[p.copy() for p in dump.poses_host], tup=tup,
                calls=list(calls))


@pytest.mark.parametrize('nms', [False, True])
def test_predict_undistorts_the_trackers_buffer_only(w32, nms):
    dist = np.tile(np.asarray(L.SETS['vga']['dist']), (3, 1))
    dist[1] = 0.0                                                               # view 1 is a pin-hole: its rows stay bit-identical
    try:
        off_model, _ = _model(w32, None)
        assert w32.lens is None and w32.lens_info is None
        off = [_frame(off_model, t, nms) for t in range(2)]
        on_model, cams = _model(w32, dist)
        assert tuple(w32.lens.shape) == (3, 10) and cams[1].lens is None and cams[0].lens is not None
        on = [_frame(on_model, t, nms) for t in range(2)]
        info = w32.lens_info.tolist()
    finally:
        w32.pose_nms = False
        w32.set_lens(None)
    K5 = np.array([[400.0, 400.0, W / 2.0, H / 2.0, 0.0]] * 3)
    for a, b in zip(off, on):
        assert 'pam_undistort_keypoints' not in a['calls']
        assert [c for c in b['calls'] if c != 'pam_undistort_keypoints'] == a['calls'] and b['calls'].count('pam_undistort_keypoints') == 1
        if nms:
            assert b['calls'].index('pam_undistort_keypoints') > b['calls'].index('pam_pose_nms')
        assert b['calls'].index('pam_undistort_keypoints') > max(i for i, c in enumerate(b['calls']) if c.startswith('pam_head_decode'))
        assert np.array_equal(a['n_det'], b['n_det'])
        moved = 0.0
        for v in range(3):
            k = int(a['n_det'][v])
            want, ok = L.undistort_px(K5[v], dist[v], a['det'][v, :k, :, 1::-1])
            assert ok.all()
            assert np.abs(b['det'][v, :k, :, 1::-1] - want).max() <= L.TOL_PX
            assert np.array_equal(b['det'][v, :k, :, 2], a['det'][v, :k, :, 2]) and np.array_equal(b['det'][v, k:], a['det'][v, k:])
            if v == 1:
                assert np.array_equal(b['det'][v], a['det'][v])
            else:
                moved = max(moved, float(np.abs(b['det'][v, :k, :, :2] - a['det'][v, :k, :, :2]).max()))
        assert moved > 0.5
        # the host side is the raw image's: dicts, poses_host and the 9-tuple's pts
        assert a['lists'] == b['lists'] and all(np.array_equal(p, q) for p, q in zip(a['poses'], b['poses']))
        for cams_i, pts_i in zip(b['tup'][0], b['tup'][1]):
            for cid, row in zip(cams_i, pts_i):
                assert any(np.array_equal(row, r) for r in b['poses'][int(cid)])
    assert info[0] == 0 and info[1] == 17 * int(on[-1]['n_det'].sum())
