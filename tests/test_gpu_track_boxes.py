"""pam_track_boxes on the GPU against tests/boxes_ref.track_boxes, computed from the decoded record of the frame before (pose3d,
velocity, last_time): counts, track ids and order exact, coordinates within one float32 ulp (the double arithmetic of the two differs
by about 1e-13 px, so only a rounding tie can move the float32).  State is built by Handle.frame, on S4 by the three-launch k_frame."""
import numpy as np
import pytest
import torch

import boxes_ref as B
from pam import synth

pytestmark = pytest.mark.gpu

MAX_DET = 8


class Rig(object):
    def __init__(self, size, n_frames):
        from pam.ivclabpose import ivclabpose
        self.seq = synth.make_sequence(size, n_frames=n_frames, seed=3)
        cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]]); conf = cfg.pop('CONF_THRESHOLD')
        self.model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=8, max_tracks=16)
        m = self.seq['meta']
        self.w, self.h = m['w'], m['h']
        self.cams = self.model.GetCameraParameters(self.seq['calib'], self.w, self.h)
        self.P = np.stack([c.P for c in self.cams])
        self.trk, self.handle, self.C = self.model.tracker, self.model.tracker.handle, len(self.cams)
        self.dev = torch.device('cuda:0')

    def step(self, t):
        self.trk.tracking(t, self.cams, None, None, [d[:, :, [1, 0, 2]] for d in self.seq['frames'][t]])
        assert self.trk.last['status'] == 0
        return self.trk.last['tracks']

    def boxes(self, frame_id, w=None, h=None, max_det=MAX_DET, **rule):
        out = dict(boxes=torch.full((self.C, max_det, 5), -7.0, dtype=torch.float32, device=self.dev),
                   count=torch.full((2 * self.C,), -7, dtype=torch.int32, device=self.dev),
                   ids=torch.full((self.C, max_det), -7, dtype=torch.int32, device=self.dev),
                   info=torch.full((2,), -7, dtype=torch.int32, device=self.dev))
        self.handle.track_boxes(torch.cuda.current_stream().cuda_stream, frame_id, w or self.w, h or self.h, out['boxes'], out['count'],
                                out['ids'], out['info'], **rule)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def check(self, tracks, frame_id, w=None, h=None, max_det=MAX_DET):
        ref = B.track_boxes(self.P, tracks, frame_id, w or self.w, h or self.h, max_det, **B.RULE)
        assert ref['margin'] > 1e-6, 'a decision of the reference sits on its threshold: pick another seed'
        got = self.boxes(frame_id, w, h, max_det)
        assert got['count'].tolist() == ref['count'].tolist() and got['info'].tolist() == ref['info'].tolist()
        assert np.array_equal(got['ids'], ref['ids'])
        g, r = got['boxes'].astype(np.float64), ref['boxes'].astype(np.float64)
        assert np.all(np.abs(g - r) <= np.spacing(np.abs(ref['boxes'])).astype(np.float64)), np.abs(g - r).max()
        assert np.array_equal(got['boxes'][..., 4], ref['boxes'][..., 4])
        return got, ref


@pytest.mark.parametrize('size,n_frames,stops', [('S1', 12, (0, 3, 11)), ('S2', 12, (0, 3, 11)), ('S4', 6, (0, 3, 5))])
def test_boxes_of_the_next_frames_follow_the_record(size, n_frames, stops):
    rig = Rig(size, n_frames)
    assert rig.handle.plan()['launches'] == (3 if size == 'S4' else 1)
    boxed = 0
    for t in range(n_frames):
        tracks = rig.step(t)
        if t not in stops:
            continue
        assert len(tracks) >= rig.seq['meta']['P'] - 1
        for ahead in (1, 3):
            got, ref = rig.check(tracks, t + ahead)
            boxed += int(got['count'][:rig.C].sum())
            assert got['info'][1] == sum(1 for tr in tracks if t + ahead - tr['last_time'] <= 3)
        got, _ = rig.check(tracks, t + 4)
        if all(tr['last_time'] == t for tr in tracks):
            assert not got['count'].any() and got['info'].tolist() == [0, 0]
    assert boxed >= 2 * len(stops) * rig.C                      # the comparisons above were not about empty lists
    rig.handle.reset()
    got = rig.boxes(n_frames)
    assert not got['count'].any() and got['info'].tolist() == [0, 0] and np.all(got['ids'] == -1) and not got['boxes'].any()


def test_small_frame_clamps_and_drops_and_a_short_list_raises_the_status_bit():
    rig = Rig('S2', 12)
    for t in range(12):
        tracks = rig.step(t)
    assert len(tracks) == 4
    full, _ = rig.check(tracks, 12)
    assert full['count'][:5].tolist() == [4] * 5 and full['info'].tolist() == [0, 4]
    none, _ = rig.check(tracks, 12, w=200, h=150)               # the S2 rig looks at the middle of 1032 x 776: every box clamps to nothing
    assert not none['count'].any() and none['info'].tolist() == [0, 4]
    small, ref = rig.check(tracks, 12, w=500, h=400)
    n = small['count'][:5]
    assert 0 < n.sum() < 20                                      # some boxes are dropped, some stay ...
    kept = np.concatenate([small['boxes'][v, :n[v], :4] for v in range(5)])
    assert ((kept[:, 0] == 0) | (kept[:, 1] == 0) | (kept[:, 2] == 500) | (kept[:, 3] == 400)).any()      # ... and clamped ones among them
    short, _ = rig.check(tracks, 12, max_det=2)
    assert short['count'].tolist() == [2] * 5 + [4] * 5 and short['info'].tolist() == [1, 4]
    assert np.array_equal(short['ids'], full['ids'][:, :2])     # the first of the list stay
