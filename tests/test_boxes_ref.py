"""CPU: the box rules of tests/boxes_ref.py against what they stand for -- the track boxes must hold the people of the next frame
(and the rule without its pad must not), a tracker fed through them must not notice, the crop table must be the host path's boxes bit
for bit -- plus the schedule and the two new symbols' bindings."""
import ctypes
import os

import numpy as np
import pytest

import boxes_ref as B
from oracle import cpu_ref as O
from pam import _lib, pipeline, synth

_SEQ = {}


def sequence(size, n_frames):
    if (size, n_frames) not in _SEQ:
        _SEQ[(size, n_frames)] = synth.make_sequence(size, n_frames=n_frames, seed=3)
    return _SEQ[(size, n_frames)]


def oracle(seq, size):
    cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]])
    conf = cfg.pop('CONF_THRESHOLD')
    cams = O.make_cameras(seq['calib'])
    return O.Tracker(O.Params(cfg, conf), cams), np.stack([c.P for c in cams])


def yx(views):
    return [d[:, :, [1, 0, 2]] for d in views]


def containment(size, pad_px):
    """-> (pairs, failures): (emitted track, view) pairs whose person lies in the frame at t + 1, and how many of their boxes miss a joint."""
    seq = sequence(size, 60)
    w, h = seq['meta']['w'], seq['meta']['h']
    trk, P = oracle(seq, size)
    pairs = fails = 0
    for t in range(59):
        trk.step(t, yx(seq['frames'][t]))
        emitted = {tr.track_id for tr in trk.tracks if tr.tsu == 0 and tr.state == O.CONFIRMED}
        ref = B.track_boxes(P, B.oracle_tracks(trk), t + 1, w, h, max_det=16, **dict(B.RULE, pad_px=pad_px))
        gt = seq['gt3d'][t + 1]
        for tr in trk.tracks:
            if tr.track_id not in emitted:
                continue
            person = min(gt, key=lambda p: np.linalg.norm(gt[p].mean(0) - tr.hist[-1].mean(0)))
            assert np.linalg.norm(gt[person].mean(0) - tr.hist[-1].mean(0)) < 0.3
            for v in range(len(P)):
                x, y, h2 = B.project(P[v], gt[person])
                if not (np.all(h2 > 0) and x.min() >= 0 and y.min() >= 0 and x.max() <= w and y.max() <= h):
                    continue
                pairs += 1
                rows = [r for r in ref['boxes64'][v] if int(r[4]) == tr.track_id]
                ok = len(rows) == 1 and np.all((x >= rows[0][0]) & (x <= rows[0][2]) & (y >= rows[0][1]) & (y <= rows[0][3]))
                fails += not ok
    return pairs, fails


@pytest.mark.parametrize('size', ['S1', 'S2'])
def test_track_boxes_hold_every_joint_of_the_next_frame(size):
    pairs, fails = containment(size, B.RULE['pad_px'])
    print('%s: %d pairs, %d boxes miss a joint' % (size, pairs, fails))
    assert pairs > 400 and fails == 0


def test_the_rule_without_its_pad_is_rejected():
    """The wrong variant: grown boxes with no pad lose joints (what the 8 px are for)."""
    fails = sum(containment(size, 0.0)[1] for size in ('S1', 'S2'))
    assert fails >= 1


def run_full(seq, size, n_frames):
    trk, _ = oracle(seq, size)
    out = []
    for t in range(n_frames):
        trk.step(t, yx(seq['frames'][t]))
        c = trk.collect(t)
        out.append((list(map(int, c[5])), np.array(c[3])))
    return out


@pytest.mark.parametrize('every,n_frames', [(5, 60), (10, 60), (4, 130)])
def test_closed_loop_through_the_track_boxes_changes_nothing(every, n_frames):
    """S2: on non-detector frames the tracker only sees the detections the track boxes of that frame let through.  They let every one
    through, on every frame, so ids and poses are the full run's."""
    seq = sequence('S2', n_frames)
    w, h = seq['meta']['w'], seq['meta']['h']
    full = run_full(seq, 'S2', n_frames)
    trk, P = oracle(seq, 'S2')
    for t in range(n_frames):
        views = seq['frames'][t]
        if pipeline.box_source(t, every, True) == 'tracks':
            ref = B.track_boxes(P, B.oracle_tracks(trk), t, w, h, max_det=16, **B.RULE)
            fed = []
            for v, d in enumerate(views):
                keep = B.gate_detections(d, ref['boxes64'][v])
                assert keep == list(range(len(d))), (t, v, keep, len(d))
                fed.append(d[keep] if len(keep) else d[:0])
            views = fed
        trk.step(t, yx(views))
        c = trk.collect(t)
        assert list(map(int, c[5])) == full[t][0], t
        assert np.array_equal(np.array(c[3]), full[t][1]), t
    assert sum(len(f[0]) for f in full) > n_frames * 2


class _Frame(object):
    def __init__(self, h, w):
        self.shape = (h, w, 3)


def test_crop_table_is_the_host_path_bit_for_bit():
    """ivclabpose._person_dicts clamps and subtracts in Python floats, HRNetPose.predict packs np.float32: the reference of
    pam_crop_table must give the same bits, on boxes that cross every edge of the frame."""
    from pam.ivclabpose import ivclabpose
    rng = np.random.default_rng(11)
    V, D, w, h = 4, 12, 360, 288
    boxes = np.zeros((V, D, 5), dtype=np.float32)
    boxes[..., 0] = rng.uniform(-60, w - 20, (V, D)); boxes[..., 1] = rng.uniform(-60, h - 20, (V, D))
    boxes[..., 2] = boxes[..., 0] + rng.uniform(5, 200, (V, D)); boxes[..., 3] = boxes[..., 1] + rng.uniform(5, 200, (V, D))
    boxes[..., 4] = rng.uniform(0.3, 1, (V, D))
    boxes[0, 0, :4] = (-5.25, -0.0, w + 3.5, h + 0.125)                    # all four edges at once
    count = np.array([12, 0, 7, 3], dtype=np.int32)
    assert (boxes[..., 0] < 0).any() and (boxes[..., 1] < 0).any() and (boxes[..., 2] > w).any() and (boxes[..., 3] > h).any()
    results = [boxes[v, :count[v]] for v in range(V)]
    dicts = ivclabpose._person_dicts(None, [_Frame(h, w)] * V, 0, results)
    host = np.asarray([p['bbox'] for persons in dicts for p in persons], dtype=np.float32).reshape(-1, 4)
    ref = B.crop_table(boxes, count, w, h, max_dets=D, cap=int(count.sum()))
    assert ref['info'].tolist() == [22, 22, 0, 0] and ref['n_det'].tolist() == count.tolist()
    assert ref['xywh'].tobytes() == host.tobytes()
    assert ref['view_of'].tolist() == [v for v in range(V) for _ in range(count[v])]
    assert ref['slot_of'].tolist() == [s for v in range(V) for s in range(count[v])]


def test_crop_table_reference_cuts_and_pads():
    boxes = np.arange(3 * 8 * 5, dtype=np.float32).reshape(3, 8, 5)
    a = B.crop_table(boxes, [2, 0, 5], 1000, 1000, max_dets=4, cap=8)
    assert a['info'].tolist() == [6, 6, 1, 0] and a['n_det'].tolist() == [2, 0, 4]
    assert a['view_of'].tolist() == [0, 0, 2, 2, 2, 2, 2, 2] and a['slot_of'].tolist() == [0, 1, 0, 1, 2, 3, 3, 3]
    assert np.array_equal(a['xywh'][6], a['xywh'][5]) and np.array_equal(a['xywh'][7], a['xywh'][5])
    b = B.crop_table(boxes, [4, 4, 4], 1000, 1000, max_dets=4, cap=8)
    assert b['info'].tolist() == [8, 12, 2, 0] and b['n_det'].tolist() == [4, 4, 0]
    c = B.crop_table(boxes, [0, 0, 0], 360, 288, max_dets=4, cap=8)
    assert c['info'].tolist() == [0, 0, 0, 0] and c['view_of'].tolist() == [0] * 8 and c['xywh'][3].tolist() == [0, 0, 360, 288]


def test_box_source_schedule():
    assert [pipeline.box_source(t, 1, True) for t in range(4)] == ['detector'] * 4
    assert [pipeline.box_source(t, 4, True) for t in range(9)] == ['detector', 'tracks', 'tracks', 'tracks'] * 2 + ['detector']
    assert pipeline.box_source(3, 5, False) == 'tracks'
    with pytest.raises(ValueError):
        pipeline.box_source(5, 5, False)
    with pytest.raises(ValueError):
        pipeline.box_source(0, 0, True)


def test_both_symbols_are_bound_and_refuse_bad_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    I, P, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert _lib._SIGS['pam_track_boxes'] == (I, [P, P, I, I, I, I, F, F, F, I, I, P, P, P, P])
    assert _lib._SIGS['pam_crop_table'] == (I, [P, I, P, P, P, I, I, I, I, I, P, P, P, P, P])
    assert callable(_lib.Handle.track_boxes) and callable(_lib.crop_table)
    assert _lib.TRACK_BOX_RULE == dict(grow=1.25, pad_px=8.0, min_size_px=8.0, max_gap=3)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    tb, ct = lib.pam_track_boxes, lib.pam_crop_table
    tb.restype, tb.argtypes = _lib._SIGS['pam_track_boxes']
    ct.restype, ct.argtypes = _lib._SIGS['pam_crop_table']
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, P)
    assert tb(None, None, 0, 1, 360, 288, 1.25, 8.0, 8.0, 3, 8, p, p, None, p) == -1
    assert ct(None, 3, None, None, p, 8, 360, 288, 4, 8, p, p, p, p, p) == -1          # a NULL box list
    assert ct(None, 0, None, p, p, 8, 360, 288, 4, 8, p, p, p, p, p) == -1             # no views
    assert ct(None, 3, None, p, p, 8, 360, 288, 4, 0, p, p, p, p, p) == -1             # no rows
    assert list(buf) == [0] * 64


class _FakeModel(object):
    """The surface testmodel.frame_inputs drives, with the facade's own schedule methods."""
    person_detector = {'NAME': 'YOLOv3'}

    def __init__(self, every):
        from pam.ivclabpose import ivclabpose
        self.detect_every, self.frames_scheduled, self.calls = every, 0, []
        self.box_source = lambda ahead=0: ivclabpose.box_source(self, ahead)
        self.schedule_frame = lambda: ivclabpose.schedule_frame(self)

    def PersonDetect(self, imgs, fid):
        self.calls.append(('detect', fid)); return [[]]

    def PersonDetectResult(self, ticket):
        self.calls.append(('collect', ticket)); return [[]]

    def PersonDetectAhead(self, imgs, fid):
        self.calls.append(('ahead', fid)); return fid

    def PersonBoxesFromTracks(self, imgs, fid):
        self.calls.append(('tracks', fid)); return [[]]

    def PersonPoseDetect(self, imagelist=None, person_bbox_list=None, batch_size=20):
        return [[]]


@pytest.mark.parametrize('every', [1, 3])
def test_driver_detects_on_schedule_and_looks_ahead_only_for_detector_frames(every):
    """testmodel.frame_inputs: DETECT_EVERY absent (1) issues exactly today's calls; with 3 the detector runs on frames 0, 3, 6, the
    frames in between take PersonBoxesFromTracks, and PersonDetectAhead is issued only in front of a detector frame."""
    from pam import testmodel
    m, ahead = _FakeModel(every), None
    for t in range(7):
        _, _, _, _, ahead = testmodel.frame_inputs(m, {}, t, [None], ahead, (t + 1, [None]))
    if every == 1:
        want = [('detect', 0), ('ahead', 1)] + [c for t in range(1, 7) for c in (('collect', t), ('ahead', t + 1))]
    else:
        want = [('detect', 0), ('tracks', 1), ('tracks', 2), ('ahead', 3), ('collect', 3), ('tracks', 4), ('tracks', 5), ('ahead', 6),
                ('collect', 6)]
    assert m.calls == want


def test_shipped_config_sets_the_schedule_keys():
    import pam
    from pam.dataset import GetConfig
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_detect_every.yaml'))
    d = cfg.DETECT_MODELS['YOLOV3']
    assert (d['DETECT_EVERY'], d['TRACK_BOX_GROW'], d['TRACK_BOX_PAD']) == (5, 1.25, 8) and cfg.PIPELINE_COMBINATION['DETECT_MODEL'] == 'YOLOv3'
    base = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs.yaml'))
    assert 'DETECT_EVERY' not in base.DETECT_MODELS['YOLOV3']
