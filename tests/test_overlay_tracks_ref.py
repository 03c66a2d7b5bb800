"""CPU: tests/overlay_tracks_ref.py, the restatement of pam_overlay_tracks (include/pam.h), against what it stands for -- on oracle
tracks of a synthetic S1 sequence its pin-hole rows are visualization.overlay_table(track_rows(...))'s, row for row -- and its edges:
joints behind the camera, NaN poses, coordinates beyond 2^18, the null rows behind the count.  Plus view3d_camera on the golden rigs
and the bindings of the two new symbols."""
import ctypes

import numpy as np
import pytest

import golden_io as G
import overlay_tracks_ref as T
from oracle import cpu_ref as O
from pam import _lib, synth
from pam import visualization as V

W, H = 360, 288
assert T.ROWS == _lib.OVERLAY_TRACK_ROWS           # the restatement and the library agree on the rows of a track in a view


class Cam(object):
    def __init__(self, P, position=None):
        self.P, self.position = np.asarray(P, dtype=np.float32), position

    def projectPoints(self, X):
        x = self.P.astype(np.float64) @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T
        return np.stack([x[1] / x[2], x[0] / x[2]], axis=1)           # rows (y, x)


class Track(object):
    def __init__(self, d):
        self.track_id, self.pose3d, self.emitted, self.pose3d_filtered = d['track_id'], d['pose3d'], d['emitted'], None


@pytest.fixture(scope='module')
def s1():
    """-> (cameras, [per compared frame the tracks in list order]) from the oracle tracker on 12 frames of S1."""
    seq = synth.make_sequence('S1', n_frames=12, seed=3)
    cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
    ocams = O.make_cameras(seq['calib'])
    trk = O.Tracker(O.Params(cfg, conf), ocams)
    out = []
    for t in range(12):
        trk.step(t, [d[:, :, [1, 0, 2]] for d in seq['frames'][t]])
        if t in (0, 3, 11):
            out.append([dict(track_id=tr.track_id, pose3d=np.array(tr.hist[-1], dtype=np.float64),
                             emitted=tr.tsu == 0 and tr.state == O.CONFIRMED) for tr in trk.tracks])
    return [Cam(c.P, c.position) for c in ocams], out


def views_of(cams, w=W, h=H):
    return [dict(P=c.P, w=w, h=h) for c in cams]


def test_pinhole_rows_are_overlay_tables_rows_of_the_reprojected_tracks(s1):
    cams, frames = s1
    cap = T.ROWS * 16
    drawn = 0
    for tracks in frames:
        for emitted_only in (True, False):
            ref = T.table(tracks, views_of(cams), cap, emitted_only=emitted_only)
            table, ranges = V.overlay_table(V.track_rows(cams, [Track(d) for d in tracks], emitted_only), [(W, H)] * len(cams))
            for v, (first, count) in enumerate(ranges):
                assert ref['count'][v] == count
                got, want = ref['prims'][v, :count].astype(np.int64), table[first:first + count].astype(np.int64)
                assert np.array_equal(got[:, 4:], want[:, 4:])                       # hw, colour, reserved: the same rows in the same order
                assert np.abs(got[:, :4] - want[:, :4]).max(initial=0) <= 1          # 1/8 pixel: h0 * (1 / h2) against h0 / h2
                assert np.array_equal(ref['prims'][v, count:], np.tile(np.array(T.NULL_ROW, dtype=np.int32), (cap - count, 1)))
                drawn += count
    assert len(frames[-1]) >= 2 and any(d['emitted'] for d in frames[-1]) and any(not d['emitted'] for d in frames[0])
    assert drawn > 10 * T.ROWS


def test_palette_and_style_are_the_host_drawings():
    assert T.palette() == V.track_palette() and len(T.palette()) == 25
    for size in ((360, 288), (1032, 776), (1920, 1080), (375, 400), (225, 300), (64, 48), (65535, 65535)):
        r, lw = V.overlay_style(*size)
        assert T.style(*size) == (8 * r, 4 * lw)
    assert T.style(375, 400) == (16, 8)                                             # 2.5 rounds to even


def one_track(pose, tid=3, emitted=True):
    return [dict(track_id=tid, pose3d=np.asarray(pose, dtype=np.float64), emitted=emitted)]


def test_joints_behind_the_camera_nan_rows_and_far_coordinates_drop_out_with_their_limbs():
    P = np.array([[100.0, 0, 32, 0], [0, 100.0, 24, 0], [0, 0, 1, 0]])
    rng = np.random.default_rng(1)
    X = np.concatenate([rng.uniform(-0.3, 0.3, (17, 2)), rng.uniform(2.0, 3.0, (17, 1))], axis=1)
    view = [dict(P=P, w=64, h=48)]
    full = T.table(one_track(X), view, 40)
    assert full['count'][0] == 36 and full['margin'] > 0
    rows = full['prims'][0]
    assert set(rows[:19, 4]) == {8} and set(rows[19:36, 4]) == {16} and np.all(rows[36:] == np.array(T.NULL_ROW))
    assert np.all(rows[:19, 5] == T.palette()[3]) and rows[19:36, 5].tolist() == T.palette()[8:]
    gone = (5, 7, 8, 17, 19 + 5)                                                    # the left shoulder: limbs 5-11, 5-6, 5-7, 0-5 and joint 5
    for bad in ((0.0, 0.0, -2.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 2.0), (0.0, np.inf, 2.0), (700.0, 0.0, 2.0), (0.0, -700.0, 2.0)):
        Y = X.copy(); Y[5] = bad
        got = T.table(one_track(Y), view, 40)
        assert got['count'][0] == 31, bad
        assert np.array_equal(got['prims'][0, :31], np.delete(rows[:36], gone, axis=0))
        assert np.all(got['prims'][0, 31:] == np.array(T.NULL_ROW))
    Y = X.copy(); Y[:] = np.nan
    none = T.table(one_track(Y), view, 40)
    assert none['count'][0] == 0 and np.all(none['prims'][0] == np.array(T.NULL_ROW)) and none['margin'] == float('inf')
    edge = T.table(one_track(np.tile([(32768.0 - 32) / 100.0, 0.0, 1.0], (17, 1))), view, 40)       # u = 32768 exactly: 2^18 eighths stays
    assert edge['count'][0] == 36 and edge['prims'][0, 0, 0] == 1 << 18
    assert T.table(one_track(X, emitted=False), view, 40)['count'][0] == 0
    assert T.table(one_track(X, emitted=False), view, 40, emitted_only=False)['count'][0] == 36
    assert T.table(one_track(X, tid=-3), view, 40)['prims'][0, 0, 5] == T.palette()[5]              # the non-negative remainder


def test_a_lens_row_moves_the_joints_and_a_zero_row_does_not():
    P = np.array([[100.0, 0, 32, 0], [0, 100.0, 24, 0], [0, 0, 1, 0]])
    rng = np.random.default_rng(2)
    X = np.concatenate([rng.uniform(-0.3, 0.3, (17, 2)), rng.uniform(2.0, 3.0, (17, 1))], axis=1)
    plain = T.table(one_track(X), [dict(P=P, w=64, h=48)], 36)
    zero = T.table(one_track(X), [dict(P=P, w=64, h=48, lens=[100.0, 100.0, 32.0, 24.0, 0, 0, 0, 0, 0, 0])], 36)
    bent = T.table(one_track(X), [dict(P=P, w=64, h=48, lens=[100.0, 100.0, 32.0, 24.0, 0, -0.5, 0, 0, 0, 0])], 36)
    assert np.array_equal(plain['prims'], zero['prims'])
    assert bent['count'][0] == 36 and not np.array_equal(plain['prims'][0, :, :4], bent['prims'][0, :, :4])
    assert np.array_equal(plain['prims'][0, :, 4:], bent['prims'][0, :, 4:])
    # a negative k1 alone pulls every joint towards the principal point, and rounding keeps the order
    c = np.array([8 * 32, 8 * 24])
    a, b = plain['prims'][0, 19:, :2].astype(np.int64) - c, bent['prims'][0, 19:, :2].astype(np.int64) - c
    assert np.all(np.abs(b) <= np.abs(a))


@pytest.mark.parametrize('size', ['S1', 'S2', 'S3'])
@pytest.mark.parametrize('canvas,angles', [((640, 480), dict()), ((300, 500), dict(azimuth=200.0, elevation=60.0, margin=0.02))])
def test_view3d_camera_holds_the_rig_and_every_golden_joint(size, canvas, angles):
    cam, tr = G.cameras(size), G.load('trace_%s.npz' % size)
    pos = np.asarray(cam['position'], dtype=np.float64)
    P = V.view3d_camera([Cam(p, q) for p, q in zip(cam['P32'], pos)], canvas, **angles)
    assert P.dtype == np.float32 and P.shape == (3, 4)
    pts = [np.asarray(tr[k]).transpose(0, 2, 1).reshape(-1, 3) for k in tr.files if k.endswith('.pts3d') and tr[k].size]
    assert sum(len(p) for p in pts) > 1000
    X = np.concatenate(pts + [pos])
    x = np.concatenate([X, np.ones((len(X), 1))], axis=1) @ P.astype(np.float64).T
    u, w = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
    assert x[:, 2].min() > 0 and u.min() >= 0 and u.max() <= canvas[0] - 1 and w.min() >= 0 and w.max() <= canvas[1] - 1
    assert max(u.max() - u.min(), w.max() - w.min()) > 0.4 * min(canvas)             # ... and the view is not a dot in the middle
    assert np.array_equal(V.view3d_camera(pos, canvas, **angles), P)                 # bare centres do as well as camera objects


def test_the_new_symbols_are_bound_and_refuse_a_null_handle():
    lib = _lib.load()
    assert _lib._SIGS['pam_overlay_draw_counted'][1][-1] == ctypes.c_void_p and len(_lib._SIGS['pam_overlay_tracks'][1]) == 13
    assert ctypes.sizeof(_lib.PamOverlayTrackView) == 16 and _lib.OVERLAY_TRACK_ROWS == T.ROWS == 19 + 17
    view = (_lib.PamOverlayTrackView * 1)()
    view[0].camera, view[0].width, view[0].height = 0, 64, 48
    pal = (ctypes.c_uint32 * 25)(*T.palette())
    assert lib.pam_overlay_tracks(None, None, 0, 1, view, None, 0, None, pal, 1, 36, ctypes.c_void_p(256), ctypes.c_void_p(256)) == -1
    dv = (_lib.PamOverlayView * 1)()
    dv[0].dev_bgr, dv[0].width, dv[0].height, dv[0].prim_first, dv[0].prim_count = 256, 16, 16, 0, 4
    assert lib.pam_overlay_draw_counted(None, 1, dv, ctypes.c_void_p(256), 4, None) == -1       # no counts: refused before any launch
