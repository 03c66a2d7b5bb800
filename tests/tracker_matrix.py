"""Shared pieces of test_gpu_tracker_matrix.py: synthetic rigs of any size, the frame step through the drop-in facade checked
against the CPU oracle every frame, and record comparisons between handles.  A plain module (not a conftest.py)."""
import numpy as np

from oracle import cpu_ref as O
from pam import synth

# the stress pattern of the matrix: occlusions, empty views, a death and a birth at birth_death_frame (the leaver's track lives on
# for MAX_AGE frames beside the newcomer's, one track more than persons), and (churn) a person that
# vanishes from every view for longer than MAX_AGE every 20 frames, so that its track dies and a new one is born when it returns
STRESS = dict(occlusion_every=3, empty_view_every=7, birth_death_frame=14, churn_every=20, churn_len=12)


def add_rig(monkeypatch, C, P, dataset='Panoptic'):
    """Register a synthetic size of C views and P persons (HD images) for make_sequence; returns its name."""
    name = 'M%d_%d' % (C, P)
    monkeypatch.setitem(synth.SIZES, name, dict(C=C, P=P, w=1920, h=1080, f=1000.0))
    monkeypatch.setitem(synth.SIZE_TO_DATASET, name, dataset)
    return name


def matcher(size):
    cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]])
    conf = cfg.pop('CONF_THRESHOLD')
    return cfg, conf


def views_per_joint(jv):
    """Largest number of views any joint of one track was built from (joints_views[k] = joints kept in k + 1 views)."""
    return max((k + 1 for k, js in enumerate(jv) if len(js)), default=0)


class FacadeVsOracle(object):
    """The drop-in facade (k_frame) and the oracle fed the same frames; ``step`` asserts what
    test_facade_vs_oracle_on_fresh_stress_sequences asserts and records how far the case got."""

    def __init__(self, seq, max_dets, max_tracks):
        from pam.ivclabpose import ivclabpose
        size = seq['meta']['size']
        cfg, conf = matcher(size)
        self.dev = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=max_dets, max_tracks=max_tracks)
        cams = self.dev.GetCameraParameters(seq['calib'], seq['meta']['w'], seq['meta']['h'])
        self.ref = O.OracleIvclabpose(cfg, conf)
        self.ref.GetCameraParameters(seq['calib'], F=np.stack([c.F for c in cams]))
        self.handle = self.dev.tracker.handle
        self.max_det = self.max_tracks = self.max_views = self.n_out = 0

    def step(self, t, views):
        pbl, dr = synth.to_dump_results(views)
        a = self.dev.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        b = self.ref.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        assert self.dev.tracker.last['status'] == 0, (t, self.dev.tracker.last['status'])
        assert list(a[5]) == list(b[5]), (t, a[5], b[5])                                   # emitted track ids
        assert [list(map(int, c)) for c in a[0]] == [list(map(int, c)) for c in b[0]], t   # camera ids per track
        assert [list(map(int, c)) for c in a[2]] == [list(map(int, c)) for c in b[2]], t   # person (detection) ids per track
        assert a[4] == b[4], t                                                             # views per joint
        if len(a[5]):
            assert np.abs(np.asarray(a[3]) - np.asarray(b[3])).max() < 1e-6, t
        self.n_out += len(a[5])
        self.max_det = max(self.max_det, max(len(v) for v in views))
        self.max_tracks = max(self.max_tracks, self.dev.tracker.last['n_tracks'])
        self.max_views = max([self.max_views] + [views_per_joint(jv) for jv in a[4]])
        return a

    def record(self):
        """(out_i, out_d) of the facade's single-scene handle after the last step."""
        return self.handle.out_i[0], self.handle.out_d[0]


def handle_for(lib, size, cams, max_dets, max_tracks, n_scenes=1, max_hyps=0):
    """A bare handle on a rig of the given cameras (objects with P, F, RK_INV, position: the facade's or the oracle's)."""
    cfg, conf = matcher(size)
    h = lib.Handle(len(cams), lib.make_params(cfg, conf), max_dets=max_dets, max_tracks=max_tracks, max_hyps=max_hyps,
                   n_scenes=n_scenes)
    h.set_cameras(np.stack([c.P for c in cams]), np.stack([c.F for c in cams]), np.stack([c.RK_INV for c in cams]),
                  np.stack([c.position for c in cams]))
    return h


def run_dev(h, t, n_det, det):
    """One frame through pam_frame_dev (device counts are taken unchecked) -> the decoded record of scene 0."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    n_t = torch.tensor(np.asarray(n_det, dtype=np.int32), device='cuda')
    d_t = torch.tensor(np.asarray(det, dtype=np.float64), device='cuda')
    h.frame_dev(st, t, n_t.data_ptr(), d_t.data_ptr())
    h.fetch(st)
    h.sync(st)
    return h.decode(0)


def assert_same_record(layout, got, want, what, skip_status=False):
    """Records of two handles equal word for word, except the in-kernel clocks (and, on request, the status word)."""
    gi, gd = got
    wi, wd = want
    if skip_status:
        gi, wi = np.delete(gi, 1), np.delete(wi, 1)
    assert np.array_equal(gi, wi), what
    k = layout.dbl_hdr_words
    assert np.array_equal(gd[k:], wd[k:]), what
