"""pam_track_boxes with a lens table (pam_set_lens) on the GPU: the boxes lie round the tracks in the RAW image.  Compared with a float64
restatement that pushes tests/boxes_ref.py's joint projections through tests/lens_ref.py's forward model before boxing: counts and ids
exact, coordinates within one float32 ulp of the restatement's rounding (the two double computations differ by about 1e-13 px, so only a
rounding tie can move the float32).  Without a table -- before the first pam_set_lens and after pam_set_lens(NULL) -- the kernel gives
the same bits."""
import numpy as np
import pytest
import torch

import boxes_ref as B
import lens_ref as L
from pam import synth

pytestmark = pytest.mark.gpu

MAX_DET = 8
N_FRAMES = 6


def lens_boxes(P, K5, dist, tracks, frame_id, frame_w, frame_h, max_det, grow, pad_px, min_size_px, max_gap):
    """boxes_ref.track_boxes with every camera's joint projections moved to the raw image before the min / max (the rule of include/pam.h:
    centre = middle of the joints' min / max, half sizes = 0.5 * grow * (max - min) + pad_px, clamped to the frame, dropped below
    min_size_px, rounded once to float32).  -> dict(boxes, count, ids, info, margin)."""
    C = len(P)
    boxes = np.zeros((C, max_det, 5), dtype=np.float32)
    ids = np.full((C, max_det), -1, dtype=np.int32)
    count, info, margin = np.zeros(2 * C, dtype=np.int32), np.zeros(2, dtype=np.int32), np.inf
    grow, pad_px, min_size_px = float(np.float32(grow)), float(np.float32(pad_px)), float(np.float32(min_size_px))
    for tr in tracks:
        gap = int(frame_id) - int(tr['last_time'])
        if not 0 <= gap <= max_gap:
            continue
        info[1] += 1
        X = B.predict_pose(tr['pose3d'], tr['velocity'], gap)
        for v in range(C):
            x, y, h2 = B.project(P[v], X)
            margin = min(margin, float(np.abs(h2).min()))
            if not np.all(h2 > 0):
                continue
            raw = L.distort_px(K5[v], dist[v], np.stack([x, y], axis=1)) if np.any(dist[v]) else np.stack([x, y], axis=1)
            x, y = raw[:, 0], raw[:, 1]
            cx, cy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
            hx, hy = 0.5 * grow * (x.max() - x.min()) + pad_px, 0.5 * grow * (y.max() - y.min()) + pad_px
            x1, y1 = max(cx - hx, 0.0), max(cy - hy, 0.0)
            x2, y2 = min(cx + hx, float(frame_w)), min(cy + hy, float(frame_h))
            margin = min(margin, abs((x2 - x1) - min_size_px), abs((y2 - y1) - min_size_px))
            if x2 - x1 < min_size_px or y2 - y1 < min_size_px:
                continue
            n = int(count[C + v])
            if n < max_det:
                boxes[v, n] = (x1, y1, x2, y2, 1.0)
                ids[v, n] = tr['track_id']
            count[C + v] = n + 1
    count[:C] = np.minimum(count[C:], max_det)
    info[0] = 1 if np.any(count[C:] > max_det) else 0
    return dict(boxes=boxes, count=count, ids=ids, info=info, margin=margin)


class Rig(object):
    def __init__(self):
        from pam.ivclabpose import ivclabpose
        self.seq = synth.make_sequence('S1', n_frames=N_FRAMES, seed=3)
        cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
        self.model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=8, max_tracks=16)
        m = self.seq['meta']
        self.w, self.h = m['w'], m['h']
        self.cams = self.model.GetCameraParameters(self.seq['calib'], self.w, self.h)
        self.P = np.stack([c.P for c in self.cams])
        self.trk, self.handle, self.C = self.model.tracker, self.model.tracker.handle, len(self.cams)
        for t in range(N_FRAMES):
            self.trk.tracking(t, self.cams, None, None, [d[:, :, [1, 0, 2]] for d in self.seq['frames'][t]])
            assert self.trk.last['status'] == 0
        self.tracks = self.trk.last['tracks']

    def boxes(self, frame_id):
        dev = torch.device('cuda:0')
        out = dict(boxes=torch.full((self.C, MAX_DET, 5), -7.0, dtype=torch.float32, device=dev),
                   count=torch.full((2 * self.C,), -7, dtype=torch.int32, device=dev),
                   ids=torch.full((self.C, MAX_DET), -7, dtype=torch.int32, device=dev),
                   info=torch.full((2,), -7, dtype=torch.int32, device=dev))
        self.handle.track_boxes(torch.cuda.current_stream().cuda_stream, frame_id, self.w, self.h, out['boxes'], out['count'], out['ids'],
                                out['info'], **B.RULE)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k])
               for k in a)


def test_boxes_follow_the_lens_and_leave_with_it():
    from pam import _lib
    rig = Rig()
    assert len(rig.tracks) >= 2
    K = np.stack([np.asarray(c.K, dtype=np.float64) for c in rig.cams])
    K5 = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1]], axis=1)
    dist = np.tile(np.asarray(L.SETS['vga']['dist']), (rig.C, 1))
    dist[1] = 0.0                                                  # one camera of the rig is a pin-hole: its boxes are the ideal ones
    frames = (N_FRAMES, N_FRAMES + 2)
    never = {f: rig.boxes(f) for f in frames}                      # a handle that never had a table
    for f in frames:                                               # ... is the kernel tests/test_gpu_track_boxes.py knows
        ref = B.track_boxes(rig.P, rig.tracks, f, rig.w, rig.h, MAX_DET, **B.RULE)
        assert never[f]['count'].tolist() == ref['count'].tolist() and np.array_equal(never[f]['ids'], ref['ids'])
    rig.handle.set_lens(_lib.lens_table(K, dist))
    moved, boxed = 0.0, 0
    for f in frames:
        ref = lens_boxes(rig.P, K5, dist, rig.tracks, f, rig.w, rig.h, MAX_DET, **B.RULE)
        assert ref['margin'] > 1e-6, 'a decision of the restatement sits on its threshold: pick another seed'
        got = rig.boxes(f)
        assert got['count'].tolist() == ref['count'].tolist() and got['info'].tolist() == ref['info'].tolist()
        assert np.array_equal(got['ids'], ref['ids'])
        g, r = got['boxes'].astype(np.float64), ref['boxes'].astype(np.float64)
        assert np.all(np.abs(g - r) <= np.spacing(np.abs(ref['boxes'])).astype(np.float64)), np.abs(g - r).max()
        assert np.array_equal(got['boxes'][1].view(np.uint32), never[f]['boxes'][1].view(np.uint32))     # the pin-hole camera of the table
        boxed += int(got['count'][:rig.C].sum())
        if got['count'].tolist() == never[f]['count'].tolist():
            moved = max(moved, float(np.abs(got['boxes'] - never[f]['boxes']).max()))
    assert boxed >= 2 * rig.C and moved > 0.5                      # boxes were drawn, and not where the pin-hole model draws them
    rig.handle.set_lens(None)
    for f in frames:
        assert same_bits(rig.boxes(f), never[f])
    rig.handle.set_lens(_lib.lens_table(K, dist))
    rig.handle.set_lens(np.concatenate([K5, np.zeros((rig.C, 5))], axis=1))          # all-zero coefficients remove the table too
    for f in frames:
        assert same_bits(rig.boxes(f), never[f])


def test_set_lens_refuses_what_is_not_a_table():
    from pam import _lib
    rig = Rig()
    with pytest.raises(ValueError):
        rig.handle.set_lens(np.ones((rig.C + 1, 10)))
    bad = np.ones((rig.C, 10)); bad[0, 0] = 0.0
    with pytest.raises(ValueError):
        rig.handle.set_lens(bad)
    lib = _lib.load()
    nan = np.ones((rig.C, 10)); nan[1, 7] = np.nan
    assert lib.pam_set_lens(rig.handle.raw, nan.ctypes.data) != 0 and lib.pam_set_lens(rig.handle.raw, bad.ctypes.data) != 0
    assert lib.pam_set_lens(None, nan.ctypes.data) != 0
