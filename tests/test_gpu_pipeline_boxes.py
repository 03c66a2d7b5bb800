"""GPU: person boxes that never visit the host.  FramePipeline.pose_step_boxes (pam_crop_table in front of the crop, forward and decode
kernels) against pose_step on the same rows from the host; a tracker whose non-detector frames only see what FramePipeline.track_boxes
lets through against one that sees everything; the facade's PersonBoxesFromTracks against the reference rule."""
import numpy as np
import pytest
import torch

import boxes_ref as B
from pam import synth

pytestmark = pytest.mark.gpu


def _rig(size, n_frames):
    from pam.ivclabpose import Camera, fundamental_matrices
    meta = synth.SIZES[size]
    seq = synth.make_sequence(size, n_frames=n_frames, seed=3)
    cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]]); conf = cfg.pop('CONF_THRESHOLD')
    P32 = seq['calib']['P'].astype(np.float32); K32 = seq['calib']['K'].astype(np.float32); RT32 = seq['calib']['RT'].astype(np.float32)
    Fm = fundamental_matrices(K32, RT32)
    cams = [Camera(j, P32[j], K32[j], RT32[j], Fm[j], w=meta['w'], h=meta['h']) for j in range(meta['C'])]
    return seq, cams, cfg, conf, meta


@pytest.fixture(scope='module')
def w32():
    from pam import hrnet
    return hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_dets=8, autotune=False)


@pytest.mark.parametrize('cap', [6, 8])
def test_device_table_decodes_what_the_host_table_decodes(w32, cap):
    """S1 rig, seeded uint8 frames, HRNet-W32 at 256 x 192 with random weights; a hand-built detector-layout tensor with 2, 1 and 3 boxes.
    cap = 6 is the exact count, cap = 8 adds two rows that repeat the last one."""
    from pam.pipeline import FramePipeline
    seq, cams, cfg, conf, meta = _rig('S1', 2)
    h, w = meta['h'], meta['w']
    pipe = FramePipeline(cams, cfg, conf, (h, w), max_dets=8, net=w32, crop_cap=cap)
    dev = pipe.device
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)).to(dev)
    ptrs = torch.tensor([frames[v].data_ptr() for v in range(3)], dtype=torch.int64, device=dev)
    boxes = np.zeros((3, 8, 5), dtype=np.float32)
    boxes[0, :2] = [[20.5, 30.25, 120.0, 230.0, 0.9], [-6.0, 40.0, 95.5, 250.0, 0.8]]
    boxes[1, :1] = [[200.0, 60.0, 371.0, 270.0, 0.7]]
    boxes[2, :3] = [[10.0, -5.0, 70.0, 120.0, 0.9], [150.25, 40.5, 240.0, 300.0, 0.6], [90.0, 100.0, 180.0, 280.0, 0.5]]
    count = [2, 1, 3, 2, 1, 3]
    ref = B.crop_table(boxes, count, w, h, max_dets=8, cap=cap, n_views=3)
    assert ref['info'].tolist() == [6, 6, 0, 0]
    valid = [(v, s) for v in range(3) for s in range(count[v])]

    pipe.det_local.zero_()
    pipe.pose_step_boxes(ptrs, torch.from_numpy(boxes).to(dev), torch.tensor(count, dtype=torch.int32, device=dev))
    assert pipe.table_n_det.cpu().tolist() == [2, 1, 3]
    pipe.track_step(0, pipe.table_n_det)
    rec = pipe.results()
    assert rec['crop_table'] == dict(rows=6, wanted=6, status=0)
    got = pipe.det_local.clone()

    pipe.det_local.zero_()
    pipe.pose_step(ptrs, torch.from_numpy(ref['view_of']).to(dev), torch.from_numpy(ref['slot_of']).to(dev), torch.from_numpy(ref['xywh']).to(dev))
    torch.cuda.synchronize()
    want = pipe.det_local.clone()
    for v, s in valid:
        assert torch.equal(got[v, s], want[v, s]), (v, s)
        assert float(want[v, s].abs().sum()) > 0
    pipe.track_step(1, torch.tensor(count[:3], dtype=torch.int32, device=dev))
    assert 'crop_table' not in pipe.results()                   # the host path reports no table


def test_crop_sharding_refuses_the_device_table():
    from pam.pipeline import FramePipeline
    seq, cams, cfg, conf, meta = _rig('S1', 2)
    pipe = FramePipeline(cams, cfg, conf, (meta['h'], meta['w']), max_dets=8, hrnet=False, shard='crops')
    with pytest.raises(ValueError, match='views'):
        pipe.pose_step_boxes(None, None, None)


@pytest.mark.parametrize('overlap', [False, True])
def test_closed_loop_through_the_device_track_boxes(overlap):
    """S2, 60 frames, the detector every 5th frame: on the frames in between the tracker only sees the detections that the boxes of
    FramePipeline.track_boxes let through (tests/test_boxes_ref.py's gate).  Records equal those of the run that sees everything."""
    from pam.pipeline import FramePipeline, box_source
    seq, cams, cfg, conf, meta = _rig('S2', 60)
    C, md = meta['C'], 8
    n_det_all, det_all = synth.pack_frames(seq['frames'], md)
    ref = FramePipeline(cams, cfg, conf, (meta['h'], meta['w']), max_dets=md, hrnet=False)
    new = FramePipeline(cams, cfg, conf, (meta['h'], meta['w']), max_dets=md, hrnet=False, overlap_tracker=overlap, detect_every=5)
    dev = ref.device
    fed_all = 0
    for t in range(60):
        ref.track_step(t, torch.tensor(n_det_all[t], dtype=torch.int32, device=dev), torch.tensor(det_all[t], dtype=torch.float64, device=dev))
        a = ref.results()
        views = seq['frames'][t]
        if box_source(t, new.detect_every, True) == 'tracks':
            boxes, count, ids = new.track_boxes(t)               # no host wait in between: ordered behind frame t - 1's tracker on the device
            torch.cuda.current_stream().synchronize()
            boxes, count = boxes.cpu().numpy(), count.cpu().numpy()
            keep = [B.gate_detections(d, boxes[v, :count[v]]) for v, d in enumerate(views)]
            fed_all += all(k == list(range(len(d))) for k, d in zip(keep, views))
            views = [d[k] if len(k) else d[:0] for k, d in zip(keep, views)]
        nd, dd = synth.pack_frames([views], md)
        new.track_step(t, torch.tensor(nd[0], dtype=torch.int32, device=dev), torch.tensor(dd[0], dtype=torch.float64, device=dev))
        b = new.results()
        assert a['n_tracks'] == b['n_tracks'], t
        for ta, tb in zip(a['tracks'], b['tracks']):
            assert ta['track_id'] == tb['track_id'] and ta['emitted'] == tb['emitted'] and ta['hits'] == tb['hits'], t
            assert np.array_equal(ta['pose3d'], tb['pose3d']) and np.array_equal(ta['velocity'], tb['velocity']), t
    assert fed_all == 48                                         # every non-detector frame fed every detection
    new.reset()
    assert new._auto_no == 0 and not new.track_boxes(0)[1].cpu().numpy().any()


def test_facade_boxes_from_tracks_follow_the_rule():
    """Five facade frames on S1, then PersonBoxesFromTracks for the sixth: PersonDetect's dict format plus track_id, boxes = the
    reference rule on the tracker's record, through the host conversion."""
    from pam.ivclabpose import ivclabpose
    seq = synth.make_sequence('S1', n_frames=6, seed=3)
    cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf)
    h, w = seq['meta']['h'], seq['meta']['w']
    cams = model.GetCameraParameters(seq['calib'], w, h)
    imgs = [np.zeros((h, w, 3), dtype=np.uint8)] * 3
    assert model.PersonBoxesFromTracks(imgs, 0) == [[], [], []]
    for t in range(5):
        pbl, dr = synth.to_dump_results(seq['frames'][t])
        model.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
    got = model.PersonBoxesFromTracks(imgs, 5)
    ref = B.track_boxes(np.stack([c.P for c in cams]), model.tracker.last['tracks'], 5, w, h, max_det=model.tracker.max_tracks, **B.RULE)
    assert ref['margin'] > 1e-6 and [len(p) for p in got] == ref['count'][:3].tolist() and sum(len(p) for p in got) >= 6
    for v, persons in enumerate(got):
        for k, p in enumerate(persons):
            assert p['track_id'] == ref['ids'][v, k] and p['category_id'] == 1 and p['image_id'] == 5 and p['score'] == 1.0
            assert p['data'] is imgs[v] and p['feature'] == []
            want = B.xywh_row(ref['boxes'][v, k], w, h).astype(np.float64)
            assert np.all(np.abs(np.array(p['bbox']) - want) <= 2 * np.spacing(np.float32(max(w, h)))), (v, k, p['bbox'], want)
