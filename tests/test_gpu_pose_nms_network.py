"""GPU: the OKS-NMS behind the decode, through the Python layers.  HRNetPose.predict(pose_nms=True) and FramePipeline(pose_nms=True) on box
lists in which a box appears twice in two of the views (identical crops decode to bit-identical keypoints: OKS 1) against
tests/pose_nms_ref.apply on the option-off run, the tracker against the run on the de-duplicated list with the option off, and the option
off against the calls it made before.  HRNet-W32 at 256 x 192, random weights, 6 crops."""
import numpy as np
import pytest
import torch

import boxes_ref as B
import pose_nms_ref as R
from pam import synth
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

H, W = 288, 360
A, Bx, Cx, E = [20.0, 30.0, 80.0, 160.0], [200.0, 60.0, 100.0, 200.0], [10.0, 20.0, 90.0, 180.0], [220.0, 50.0, 110.0, 220.0]
# (view, box, score): a copy of A in FRONT of it with the lower score (slot 0 dies, the view's rows move down), a copy of C behind E with
# C's own score (equal scores: the lower slot stays)
DUP = [[(A, 0.8), (A, 0.9), (Bx, 0.7)], [], [(Cx, 0.9), (E, 0.6), (Cx, 0.9)]]
KEEP = [[1, 2], [], [0, 1]]
CLEAN = [[DUP[v][s] for s in KEEP[v]] for v in range(3)]


@pytest.fixture(scope='module')
def w32():
    from pam import hrnet
    net = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_dets=8, autotune=False)
    for n in (4, 6, 8):                                  # every forward these tests replay is captured (and its form settled) up front:
        for _ in range(3):                               # the calls of a step are then the same from one run to the next
            net.features(net.input_buffer(n))
    torch.cuda.synchronize()
    return net


def _rig():
    from pam.ivclabpose import Camera, fundamental_matrices
    meta = synth.SIZES['S1']
    seq = synth.make_sequence('S1', n_frames=2, seed=3)
    cfg = dict(synth.MATCHER_CFG['Shelf']); cfg.pop('CONF_THRESHOLD')
    # random weights decode no people: with the Shelf thresholds nothing these poses do would reach a hypothesis and the tracker
    # comparisons below would be between empty states.  Every joint counts (confidence threshold far below any score) and every pair
    # of poses from two views is consistent (thresholds far above any distance in a 360 x 288 frame), so the tracker does start tracks
    # on whatever rows it is given -- and a run that is given the copies too starts other ones.
    cfg.update(EPI_THRESHOLD=1e6, INIT_THRESHOLD=1e6, JOINT_THRESHOLD=1e6)
    conf = -1e6
    P32 = seq['calib']['P'].astype(np.float32); K32 = seq['calib']['K'].astype(np.float32); RT32 = seq['calib']['RT'].astype(np.float32)
    Fm = fundamental_matrices(K32, RT32)
    return seq, [Camera(j, P32[j], K32[j], RT32[j], Fm[j], w=W, h=H) for j in range(3)], cfg, conf


def frames_of(t):
    rng = np.random.default_rng(100 + t)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3)]


def person_list(rows, frames):
    return [[dict(image_id=0, category_id=1, score=s, bbox=list(b), data=frames[v], feature=[]) for b, s in view] for v, view in enumerate(rows)]


def reference(det_off, n_in, rows):
    """tests/pose_nms_ref.apply on the option-off buffer: areas and scores from the box list, as float32."""
    view_of = [v for v, view in enumerate(rows) for _ in view]
    slot_of = [s for view in rows for s in range(len(view))]
    xywh = np.array([b for view in rows for b, _ in view], dtype=np.float32).reshape(-1, 4)
    b = np.ones((3, 8), dtype=np.float32)
    for v, view in enumerate(rows):
        b[v, :len(view)] = [s for _, s in view]
    ref = R.apply(det_off, n_in, 8, R.areas_from_rows(3, 8, view_of, slot_of, xywh), b)
    assert R.threshold_margin(ref['oks'], 0.9) > 1e-9
    assert [list(k[:n]) for k, n in zip(ref['keep_from'], ref['n_det_out'])] == KEEP       # the planted copies, nothing else
    return ref


def same(a, b):
    if isinstance(a, (list, tuple)) or (isinstance(a, np.ndarray) and a.dtype == object):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def track_state(rec):
    return [rec['n_tracks'], rec['n_hyp']] + [(t['track_id'], t['state'], t['hits'], t['age'], t['emitted'], t['order'], t['matched_det'].tolist(), t['pose3d'].tobytes())
            for t in rec['tracks']]


def test_predict_filters_like_the_restatement_and_the_tracker_sees_the_clean_list(w32):
    from pam.ivclabpose import ivclabpose
    seq, _, cfg, conf = _rig()
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=8)
    model.pose_model = w32
    model.tracker.set_input_guard(w32)
    model.GetCameraParameters(seq['calib'], W, H)
    assert w32.pose_nms is False and (w32.oks_thre, w32.in_vis_thre) == (0.9, 0.2)
    runs = {}
    try:
        for form, rows, nms in (('off', DUP, False), ('on', DUP, True), ('clean', CLEAN, False)):
            w32.pose_nms = nms
            model.tracker.track_restart()
            out = []
            for t in range(2):
                pbl = person_list(rows, frames_of(t))
                with recorded_calls() as calls:
                    dump = model.PersonPoseDetect(person_bbox_list=pbl, batch_size=20)
                n_det, det = dump.device_n_det.cpu().numpy().copy(), dump.device_det.cpu().numpy().copy()
                tup = model.PersonTrack_Project3DPose(t, pbl, dump, 'SVD')
                out.append(dict(n_det=n_det, det=det, lists=[[dict(it) for it in v] for v in dump], poses=[p.copy() for p in dump.poses_host],
                                tup=tup, state=track_state(model.tracker.last), calls=list(calls), nms=dump._nms))
            runs[form] = out
            if form == 'off':                            # the option off uploads the tables it uploaded before and allocates nothing for the filter
                V, n = 3, 6
                assert 6 * n + V + (V & 1) + 2 * V in w32._meta_pinned and 6 * n + V + (V & 1) + 2 * V + V * 8 not in w32._meta_pinned
                assert all(r['nms'] is None for r in out)
                assert all(not ent[2] for ring in w32._kp_pinned.values() for ent in ring)
    finally:
        w32.pose_nms = False
    assert {46, 46 + 3 * 8, 34} <= set(w32._meta_pinned)                                       # off, on (+ the (V, S) score table), clean
    for t in range(2):
        off, on, clean = runs['off'][t], runs['on'][t], runs['clean'][t]
        assert 'pam_pose_nms' not in off['calls'] and [c for c in on['calls'] if c != 'pam_pose_nms'] == off['calls']
        assert on['calls'].count('pam_pose_nms') == 1 and on['calls'][-1] == 'pam_pose_nms'     # once, behind the last decode
        assert off['n_det'].tolist() == [3, 0, 3] and [len(v) for v in off['lists']] == [3, 0, 3]
        ref = reference(off['det'], off['n_det'], DUP)
        assert on['n_det'].tolist() == ref['n_det_out'].tolist() == [2, 0, 2]
        for v in range(3):
            k = int(ref['n_det_out'][v])
            assert on['det'][v, :k].tobytes() == ref['det'][v, :k].tobytes() and float(np.abs(on['det'][v, :k]).sum()) > 0 or k == 0
            assert not on['det'][v, k:int(off['n_det'][v])].any()
            assert len(on['lists'][v]) == k and on['poses'][v].tobytes() == off['poses'][v][KEEP[v]].tobytes()
            for slot, (it, src) in enumerate(zip(on['lists'][v], KEEP[v])):
                was = off['lists'][v][src]
                assert it['bbox'] == was['bbox'] == list(DUP[v][src][0]) and it['keypoints'] == was['keypoints']
                assert it['keypoints_score'] == was['keypoints_score'] and it['pose_score'] == ref['pose_score'][v, slot]
                assert 'pose_score' not in was
        # the tracker: the filtered run is the run on the list without the copies
        assert on['state'] == clean['state']
        assert same(list(on['tup'][:6]), list(clean['tup'][:6]))
        print('predict, frame %d: tracker [n_tracks, n_hyp] on %s, fed the copies %s' % (t, on['state'][:2], off['state'][:2]))
        for v in range(3):
            assert on['det'][v, :len(KEEP[v])].tobytes() == clean['det'][v, :len(KEEP[v])].tobytes()
    last = runs['on'][1]['state']
    assert last[0] > 0 and len(last) == 2 + last[0]                    # the comparison was between tracks, not between empty lists
    assert runs['off'][1]['state'] != last                            # ... and the copies, unfiltered, do reach the tracker


def test_predict_refuses_more_than_32_slots_per_view(w32):
    w32.pose_nms = True
    try:
        frames = frames_of(0)
        pbl = person_list([[(A, 0.9)] * 33, [], []], frames)
        with pytest.raises(ValueError, match='32'):
            w32.predict(pbl)
    finally:
        w32.pose_nms = False


def detector_list(rows):
    """rows -> a detector-layout list (3, 8, 5) (x1, y1, x2, y2, score) and its counts."""
    boxes = np.zeros((3, 8, 5), dtype=np.float32)
    for v, view in enumerate(rows):
        for s, (b, sc) in enumerate(view):
            boxes[v, s] = [b[0], b[1], b[0] + b[2], b[1] + b[3], sc]
    return boxes, [len(view) for view in rows] * 2


def test_frame_pipeline_filters_behind_the_decode_and_the_option_off_is_the_old_step(w32):
    from pam.pipeline import FramePipeline
    _, cams, cfg, conf = _rig()
    mk = lambda **kw: FramePipeline(cams, cfg, conf, (H, W), max_dets=8, net=w32, crop_cap=8, **kw)
    off, on, clean = mk(), mk(pose_nms=True), mk()
    assert w32.pose_nms is False and on.pose_nms and not off.pose_nms and off.nms_n_det is None     # a shared net keeps its own setting
    assert off._nms is None and off.nms_pose_score is None   # off: nothing allocated
    dev = off.device
    boxes, count = detector_list(DUP)
    cboxes, ccount = detector_list(CLEAN)
    table = B.crop_table(cboxes, ccount, W, H, max_dets=8, cap=4, n_views=3)
    for t in range(2):
        frames = torch.from_numpy(np.stack(frames_of(t))).to(dev)
        ptrs = torch.tensor([frames[v].data_ptr() for v in range(3)], dtype=torch.int64, device=dev)
        tb, tc = torch.from_numpy(boxes).to(dev), torch.tensor(count, dtype=torch.int32, device=dev)
        recs, calls, dets = {}, {}, {}
        for name, pipe in (('off', off), ('on', on)):
            pipe.det_local.zero_()
            with recorded_calls() as got:
                pipe.pose_step_boxes(ptrs, tb, tc)
                pipe.track_step(t, pipe.nms_n_det if pipe.pose_nms else pipe.table_n_det)
            recs[name], calls[name], dets[name] = pipe.results(), list(got), pipe.det_local.cpu().numpy().copy()
        # option off: the calls of the step as it was, no filter among them, and the decode's buffer and counts as the host table gives them
        assert 'pam_pose_nms' not in calls['off'] and 'pose_nms' not in recs['off']
        assert [c for c in calls['on'] if c != 'pam_pose_nms'] == calls['off'] and calls['on'].count('pam_pose_nms') == 1
        assert calls['on'].index('pam_pose_nms') == calls['on'].index('pam_head_decode') + 1
        assert off.table_n_det.cpu().tolist() == [3, 0, 3]
        full = B.crop_table(boxes, count, W, H, max_dets=8, cap=6, n_views=3)
        clean.det_local.zero_()
        clean.pose_step(ptrs, torch.from_numpy(full['view_of']).to(dev), torch.from_numpy(full['slot_of']).to(dev), torch.from_numpy(full['xywh']).to(dev))
        torch.cuda.synchronize()
        host = clean.det_local.cpu().numpy()
        for v in range(3):
            assert dets['off'][v, :count[v]].tobytes() == host[v, :count[v]].tobytes()
        # option on: the valid slots are the restatement's, the record says what was kept
        view_of = [v for v, view in enumerate(DUP) for _ in view]
        rows_xywh = [(list(full['xywh'][r]), DUP[v][s][1]) for r, (v, s) in enumerate(zip(full['view_of'], full['slot_of']))]
        by_view = [[rows_xywh[r] for r in range(len(view_of)) if view_of[r] == v] for v in range(3)]
        ref = reference(dets['off'], [3, 0, 3], by_view)
        assert on.nms_n_det.cpu().tolist() == [2, 0, 2] == recs['on']['pose_nms']['n_det']
        assert recs['on']['pose_nms']['keep_from'].tolist() == ref['keep_from'].tolist()
        assert np.array_equal(on.nms_pose_score.cpu().numpy(), ref['pose_score'])
        for v in range(3):
            k = int(ref['n_det_out'][v])
            assert dets['on'][v, :k].tobytes() == ref['det'][v, :k].tobytes() and not dets['on'][v, k:count[v]].any()
        # the tracker: the record of the run on the list without the copies, through the host table
        clean.det_local.zero_()
        clean.pose_step(ptrs, torch.from_numpy(table['view_of']).to(dev), torch.from_numpy(table['slot_of']).to(dev), torch.from_numpy(table['xywh']).to(dev))
        clean.track_step(t, torch.tensor(ccount[:3], dtype=torch.int32, device=dev))
        want = clean.results()
        assert recs['on']['n_tracks'] == want['n_tracks'] and track_state(recs['on']) == track_state(want)
        print('pipeline, frame %d: n_tracks %d, n_hyp %d; fed the copies n_tracks %d' % (t, want['n_tracks'], want['n_hyp'], recs['off']['n_tracks']))
    assert want['n_tracks'] > 0 and track_state(recs['off']) != track_state(want)   # tracks were compared, and the copies do change them


def test_pose_step_takes_the_counts_and_a_score_table_and_crop_sharding_is_refused(w32):
    from pam.pipeline import FramePipeline
    _, cams, cfg, conf = _rig()
    with pytest.raises(ValueError, match='views'):
        FramePipeline(cams, cfg, conf, (H, W), max_dets=8, hrnet=False, shard='crops', pose_nms=True)
    with pytest.raises(ValueError, match='32'):
        FramePipeline(cams, cfg, conf, (H, W), max_dets=33, hrnet=False, pose_nms=True)
    on = FramePipeline(cams, cfg, conf, (H, W), max_dets=8, net=w32, pose_nms=True)
    dev = on.device
    boxes, count = detector_list(DUP)
    full = B.crop_table(boxes, count, W, H, max_dets=8, cap=6, n_views=3)
    frames = torch.from_numpy(np.stack(frames_of(0))).to(dev)
    ptrs = torch.tensor([frames[v].data_ptr() for v in range(3)], dtype=torch.int64, device=dev)
    tabs = [torch.from_numpy(full[k]).to(dev) for k in ('view_of', 'slot_of', 'xywh')]
    with pytest.raises(ValueError, match='n_det'):
        on.pose_step(ptrs, *tabs)
    on.pose_step(ptrs, *tabs, n_det=torch.tensor(count[:3], dtype=torch.int32, device=dev), scores=torch.from_numpy(np.ascontiguousarray(boxes[:, :, 4])).to(dev))
    on.track_step(0, on.nms_n_det)
    rec = on.results()
    assert rec['pose_nms']['n_det'] == [2, 0, 2] and [list(k[:2]) for k in rec['pose_nms']['keep_from'][[0, 2]]] == [KEEP[0], KEEP[2]]
