"""GPU: the ordered calls into libpam_hip.so that one frame makes, for every way through the optional stages' host code: the entry names
of the second of three frames against literals recorded on the commit before the stages' host code moved into shared homes
(DESIGN.md 10q).  Tracker only on the golden trace S1 with max_dets 8; the network scenarios: HRNet-W32 at 256 x 192 with random
weights, 2 views, 3 boxes."""
import numpy as np
import pytest
import torch

import golden_io as G
from pam import _lib, synth
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

MD, HW = 8, (288, 360)
BOXES = [[20.0, 30.0, 80.0, 160.0], [200.0, 60.0, 100.0, 200.0], [10.0, 20.0, 90.0, 180.0]]       # views 0, 0, 1
DIST = [-0.1, 0.02, 1e-3, -1e-3, 0.0]

FRAME, FRAME_OE = ['pam_frame_dev_views', 'pam_fetch'], ['pam_frame_dev_views', 'pam_one_euro', 'pam_fetch']
POSE = ['pam_preprocess_crops_ex', 'pam_head_decode_scratch_bytes', 'pam_head_decode']
EXPECTED = {
    'pipeline plain': FRAME,
    'pipeline one_euro': FRAME_OE,
    'pipeline overlap one_euro': FRAME_OE,
    'pipeline crops one_euro': ['pam_frame_dev', 'pam_one_euro', 'pam_fetch'],
    'track_boxes on the tracker stream': FRAME + ['pam_track_boxes'],
    'track_boxes on the current stream': FRAME + ['pam_track_boxes'],
    'tracking_dev': ['pam_frame_dev', 'pam_fetch', 'pam_sync'],
    'tracking_dev one_euro': ['pam_frame_dev', 'pam_one_euro', 'pam_fetch', 'pam_sync'],
    'predict_boxes': ['pam_frame_dev', 'pam_fetch', 'pam_sync', 'pam_track_boxes'],
    'pose_step plain': POSE + FRAME,
    'pose_step pose_nms': POSE + ['pam_pose_nms'] + FRAME,
    'pose_step lens': POSE + ['pam_undistort_keypoints'] + FRAME,
    'pose_step affine': ['pam_preprocess_crops_affine'] + POSE[1:] + FRAME,
    'pose_step_boxes pose_nms': ['pam_crop_table'] + POSE + ['pam_pose_nms'] + FRAME,
    'predict all three': ['pam_preprocess_crops_affine'] + POSE[1:] + ['pam_pose_nms', 'pam_undistort_keypoints'],
}


@pytest.fixture(scope='module')
def s1():
    from pam.ivclabpose import ivclabpose
    tr, c = G.load('trace_S1.npz'), G.cameras('S1')
    cfg = dict(synth.MATCHER_CFG[str(tr['meta.dataset'])]); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=MD, max_tracks=16)
    model.GetCameraParameters({'P': c['P'], 'K': c['K'], 'RT': c['RT']}, 0, 0, F=c['F'])
    frames = G.trace_frames(tr)[:3]
    assert all(any(len(v) for v in views) for views in frames)
    nd, dd = synth.pack_frames(frames, MD)
    return dict(model=model, cams=model.cameras, cfg=cfg, conf=conf, C=len(model.cameras), nd_host=nd,
                nd=[torch.tensor(nd[t], dtype=torch.int32, device='cuda:0') for t in range(3)],
                dd=[torch.tensor(dd[t], dtype=torch.float64, device='cuda:0') for t in range(3)])


@pytest.fixture(scope='module')
def w32():
    from pam import hrnet
    from pam.ivclabpose import Camera, fundamental_matrices
    net = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_dets=MD, autotune=False)
    for n in (3, 4):                                     # every forward the scenarios replay is captured (and its form settled) up front
        for _ in range(3):
            net.features(net.input_buffer(n))
    torch.cuda.synchronize()
    calib = synth.make_sequence('S1', n_frames=1, seed=3)['calib']
    P, K, RT = (calib[k][:2].astype(np.float32) for k in ('P', 'K', 'RT'))
    F = fundamental_matrices(K, RT)
    cfg = dict(synth.MATCHER_CFG['Shelf']); cfg.pop('CONF_THRESHOLD')
    cfg.update(EPI_THRESHOLD=1e6, INIT_THRESHOLD=1e6, JOINT_THRESHOLD=1e6)       # random weights decode no people: every pair is consistent
    dev = net.device
    frames = [torch.from_numpy(np.random.default_rng(7 + t).integers(0, 256, (2,) + HW + (3,), dtype=np.uint8)).to(dev) for t in range(3)]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    det_boxes = np.zeros((2, MD, 5), dtype=np.float32)                            # the same three boxes in the detector's layout
    for v, s, b in ((0, 0, BOXES[0]), (0, 1, BOXES[1]), (1, 0, BOXES[2])):
        det_boxes[v, s] = [b[0], b[1], b[0] + b[2], b[1] + b[3], 0.9]
    return dict(net=net, cams=[Camera(j, P[j], K[j], RT[j], F[j], w=HW[1], h=HW[0]) for j in range(2)], cfg=cfg, conf=-1e6,
                lens=_lib.lens_table(calib['K'][:2], np.tile(DIST, (2, 1))), frames=frames,
                ptrs=[torch.tensor([f[v].data_ptr() for v in range(2)], dtype=torch.int64, device=dev) for f in frames],
                view_of=i32([0, 0, 1]), slot_of=i32([0, 1, 0]), n_det=i32([2, 1]),
                xywh=torch.tensor(BOXES, dtype=torch.float32, device=dev), det_boxes=torch.from_numpy(det_boxes).to(dev),
                det_count=i32([2, 1, 2, 1]))


def second_of_three(frame):
    """frame(t) three times -> the entry names of the second."""
    got = []
    for t in range(3):
        with recorded_calls() as calls:
            frame(t)
        got.append(list(calls))
    torch.cuda.synchronize()
    return got[1]


def tracker_scenario(s1, name):
    from pam.distributed import CropGather
    from pam.pipeline import FramePipeline
    from pam.tracker import IterativeTracker
    mk = lambda **kw: FramePipeline(s1['cams'], s1['cfg'], s1['conf'], HW, max_dets=MD, max_tracks=16, hrnet=False, **kw)
    if name.startswith('pipeline crops'):
        p, C = mk(shard='crops', one_euro=True), s1['C']

        def frame(t):
            n = s1['nd_host'][t]
            sel = CropGather.select_index([v for v in range(C) for _ in range(n[v])], [s for v in range(C) for s in range(n[v])], C, MD, 1)[0]
            p.write_send(s1['dd'][t])
            p.track_step_crops(t, s1['nd'][t], torch.tensor(sel, dtype=torch.int64, device=p.device))
            p.results()
        return second_of_three(frame)
    if name.startswith('pipeline') or name.startswith('track_boxes'):
        p = mk(**{'pipeline plain': {}, 'pipeline one_euro': dict(one_euro=True),
                  'pipeline overlap one_euro': dict(overlap_tracker=True, one_euro=True),
                  'track_boxes on the tracker stream': dict(overlap_tracker=True), 'track_boxes on the current stream': {}}[name])

        def frame(t):
            p.write_local(s1['dd'][t])
            p.track_step(t, s1['nd'][t])
            if name.startswith('track_boxes'):
                p.track_boxes(t + 1)
            p.results()
        return second_of_three(frame)
    trk = IterativeTracker(s1['model'].tracker.args, max_dets=MD, max_tracks=16, one_euro=True if name.endswith('one_euro') else None)

    def frame(t):
        trk.tracking_dev(t, s1['cams'], s1['nd'][t], s1['dd'][t])
        if name == 'predict_boxes':
            trk.predict_boxes(t + 1, HW)
    return second_of_three(frame)


def network_scenario(w, name):
    from pam.pipeline import FramePipeline
    net = w['net']
    try:
        if name in ('pose_step affine', 'predict all three'):
            net.box_transform = 'affine'
        if name == 'predict all three':
            net.pose_nms = True
            net.set_lens(w['lens'])

            def frame(t):
                host = w['frames'][t].cpu().numpy()
                views = [0, 0, 1]
                pbl = [[dict(image_id=0, category_id=1, score=0.9, bbox=list(BOXES[i]), data=host[v], feature=[])
                        for i in range(3) if views[i] == v] for v in range(2)]
                net.predict(pbl, batch_size=20)
            return second_of_three(frame)
        p = FramePipeline(w['cams'], w['cfg'], w['conf'], HW, max_dets=MD, net=net, crop_cap=4, pose_nms=name.endswith('pose_nms'),
                          lens=w['lens'] if name == 'pose_step lens' else None)

        def frame(t):
            if name.startswith('pose_step_boxes'):
                p.pose_step_boxes(w['ptrs'][t], w['det_boxes'], w['det_count'])
                p.track_step(t, p.nms_n_det)
            else:
                p.pose_step(w['ptrs'][t], w['view_of'], w['slot_of'], w['xywh'], n_det=w['n_det'])
                p.track_step(t, p.nms_n_det if p.pose_nms else w['n_det'])
            p.results(strict=False)
        return second_of_three(frame)
    finally:
        net.box_transform, net.pose_nms = 'stretch', False
        net.set_lens(None)


TRACKER = [k for k in EXPECTED if not (k.startswith('pose_step') or k.startswith('predict all'))]
NETWORK = [k for k in EXPECTED if k not in TRACKER]


@pytest.mark.parametrize('name', TRACKER)
def test_tracker_only_frames_make_the_calls_of_before(s1, name):
    got = tracker_scenario(s1, name)
    print('%s: %r' % (name, got))
    assert got == EXPECTED[name]


@pytest.mark.parametrize('name', NETWORK)
def test_network_frames_make_the_calls_of_before(w32, name):
    got = network_scenario(w32, name)
    print('%s: %r' % (name, got))
    assert got == EXPECTED[name]
