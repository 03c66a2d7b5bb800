"""pam_overlay_tracks / pam_overlay_draw_counted on a real MI355X against tests/overlay_tracks_ref.py (the restatement of include/pam.h)
with array_equal on rows and counts.  The state is built by the tracker as in test_gpu_track_boxes.py, on S4 by the three-launch frame
step; the poses the restatement is given come from the fetched record, so their bits are the kernel's.  Table and counts are carved from
a tests/guarded_mem.py arena: a row the kernel did not write, or a store outside the table, fails.  Then the edges of the rule, the
counted draw between sentinel bands against tests/overlay_ref.py's raster, and FramePipeline.overlay_step frame by frame, 3D canvas and
written JPEG files included."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guarded_mem as GM
import overlay_tracks_ref as T
from pam import _lib, synth
from pam import visualization as V
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

ROWS = T.ROWS
NEW_CALLS = ('pam_overlay_tracks', 'pam_overlay_draw_counted')
NULL = np.array(T.NULL_ROW, dtype=np.int32)


class Rig(object):
    def __init__(self, size, n_frames, max_tracks=16, seed=3, **seq):
        from pam.ivclabpose import ivclabpose
        self.seq = synth.make_sequence(size, n_frames=n_frames, seed=seed, **seq)
        cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]]); conf = cfg.pop('CONF_THRESHOLD')
        self.model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=8, max_tracks=max_tracks)
        m = self.seq['meta']
        self.w, self.h = m['w'], m['h']
        self.cams = self.model.GetCameraParameters(self.seq['calib'], self.w, self.h)
        self.P = np.stack([np.asarray(c.P, dtype=np.float32) for c in self.cams])
        self.trk, self.handle, self.C = self.model.tracker, self.model.tracker.handle, len(self.cams)
        self.max_tracks, self.dev = max_tracks, torch.device('cuda:0')

    def step(self, t):
        self.trk.tracking(t, self.cams, None, None, [d[:, :, [1, 0, 2]] for d in self.seq['frames'][t]])
        assert self.trk.last['status'] == 0
        return self.trk.last['tracks']

    def camera_views(self, w=None, h=None):
        return [dict(P=self.P[c], w=w or self.w, h=h or self.h, camera=c) for c in range(self.C)]

    def table(self, views, cap=None, extra=None, pose=None, emitted_only=True):
        """One pam_overlay_tracks launch into a fresh arena -> (prims (n_views, cap, 8), count (n_views,)) host arrays, after the arena
        has confirmed that every row was written and nothing beside them."""
        cap = ROWS * self.max_tracks if cap is None else cap
        n = len(views)
        arena = GM.GuardArena(self.dev, 2 * (4 * n * cap * 8 + 4 * n) + 16 * GM.GUARD + 8 * GM.ALIGN)
        arena.alloc(1, 1, 1, 2 * n * cap * 8); arena.alloc(1, 1, 1, 2 * n)
        prims = arena.payload(arena.allocs[0]).view(torch.int32).view(n, cap, 8)
        count = arena.payload(arena.allocs[1]).view(torch.int32)
        tv = (_lib.PamOverlayTrackView * n)()
        for k, v in enumerate(views):
            tv[k].camera, tv[k].extra, tv[k].width, tv[k].height = v.get('camera', -1), v.get('extra', 0), v['w'], v['h']
        ex = torch.from_numpy(np.ascontiguousarray(extra, dtype=np.float32)).to(self.dev) if extra is not None else None
        self.handle.overlay_tracks(torch.cuda.current_stream().cuda_stream, tv, T.palette(), prims, count, extra_P=ex, pose=pose,
                                   emitted_only=emitted_only)
        torch.cuda.synchronize()
        assert arena.report() == ''
        return prims.cpu().numpy(), count.cpu().numpy()

    def check(self, tracks, views, **kw):
        ref = T.table(tracks, views, kw.get('cap') or ROWS * self.max_tracks, emitted_only=kw.get('emitted_only', True))
        assert ref['margin'] > 1e-6, 'a coordinate of the restatement sits on a rounding boundary: pick another seed'
        prims, count = self.table(views, **kw)
        assert count.tolist() == ref['count'].tolist()
        assert np.array_equal(prims, ref['prims'])
        return ref


def extra_view(P, w, h, k=0):
    return dict(P=np.asarray(P, dtype=np.float32), w=w, h=h, camera=-1, extra=k)


@pytest.mark.parametrize('size,n_frames,stops', [('S1', 12, (0, 3, 11)), ('S2', 12, (0, 3, 11)), ('S4', 4, (3,))])
def test_table_of_the_record_equals_the_restatement(size, n_frames, stops):
    rig = Rig(size, n_frames)
    assert rig.handle.plan()['launches'] == (3 if size == 'S4' else 1)
    P3 = V.view3d_camera(rig.cams, (640, 480))
    views = rig.camera_views() + [extra_view(P3, 640, 480)]
    assert len(views) == (32 if size == 'S4' else rig.C + 1)
    rows = 0
    for t in range(n_frames):
        tracks = rig.step(t)
        if t not in stops:
            continue
        assert len(tracks) >= rig.seq['meta']['P'] - 1
        shown = rig.check(tracks, views, extra=P3[None], emitted_only=True)
        every = rig.check(tracks, views, extra=P3[None], emitted_only=False)
        n_emitted = sum(tr['emitted'] for tr in tracks)
        if t == 0:                                                           # the list holds Tentative tracks only: shown or not by the flag
            assert n_emitted == 0 and not shown['count'].any() and every['count'].all()
        assert shown['count'][-1] == ROWS * n_emitted and every['count'][-1] == ROWS * len(tracks)       # the 3D view holds everybody
        rows += int(shown['count'].sum())
    assert rows >= ROWS * len(views)                                          # the comparisons above were not about empty tables
    rig.handle.reset()
    prims, count = rig.table(views, extra=P3[None], emitted_only=False)
    assert not count.any() and np.all(prims == NULL)


@pytest.fixture(scope='module')
def s1():
    """An S1 rig after 12 frames: three Confirmed tracks."""
    rig = Rig('S1', 12)
    for t in range(12):
        tracks = rig.step(t)
    assert len(tracks) == 3 and all(tr['emitted'] for tr in tracks)
    return rig, tracks


def test_a_handle_with_one_track_slot():
    rig = Rig('S1', 4, max_tracks=1, shuffle=False)
    rig.seq['frames'] = [[v[:1] for v in views] for views in rig.seq['frames']]          # one slot: the first person alone
    for t in range(4):
        tracks = rig.step(t)
    assert len(tracks) == 1
    ref = rig.check(tracks, rig.camera_views(), cap=ROWS, emitted_only=False)
    assert ref['count'].tolist() == [ROWS] * 3                                # the table is full to its last row


def test_an_extra_view_inside_the_scene_and_one_that_leaves_the_coordinate_range(s1):
    rig, tracks = s1
    eye, f = np.array([0.0, 0.0, 1.0]), 300.0
    R = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])      # looks along +x from the middle of the people
    inside = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]]) @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)
    far = np.array([[3e5, 0, 320.0], [0, 3e5, 240.0], [0, 0, 1.0]]) @ np.concatenate([R, (-R @ (eye - [6.0, 0, 0]))[:, None]], axis=1)
    views = [extra_view(inside, 640, 480, 0), extra_view(far, 640, 480, 1), dict(rig.camera_views()[1])]
    ref = rig.check(tracks, views, extra=np.stack([inside, far]))
    assert 0 < ref['count'][0] < 3 * ROWS                                     # some joints lie behind the eye, some in front
    assert 0 < ref['count'][1] < 3 * ROWS                                     # some coordinates are beyond 2^18 eighths, some are not
    assert ref['count'][2] == 3 * ROWS


def test_explicit_poses_with_exact_products_and_a_nan_row(s1):
    rig, tracks = s1
    Pi = np.tile(np.array([[64.0, 0, 32, 0], [0, 64.0, 24, 0], [0, 0, 1, 0]], dtype=np.float32), (3, 1, 1))
    Pi[1, 0, 3] = 128.0
    cams = rig.cams
    rig.handle.set_cameras(Pi, np.stack([c.F for c in cams]), np.stack([c.RK_INV for c in cams]), np.stack([c.position for c in cams]))
    try:
        rng = np.random.default_rng(4)
        pose = np.zeros((1, 16, 17, 3))
        pose[0, :, :, :2] = rng.integers(-64, 65, (16, 17, 2)) / 64.0
        pose[0, :, :, 2] = 2.0 ** rng.integers(0, 3, (16, 17))                # h2 a power of two: 1.0 / h2 and both products are exact
        pose[0, 1] = np.nan
        pose[0, 2, 4] = (0.0, 0.0, -4.0)
        given = [dict(tr, pose3d=pose[0, i]) for i, tr in enumerate(tracks)]
        views = [dict(P=Pi[c], w=64, h=48, camera=c) for c in range(3)]
        ref = rig.check(given, views, pose=torch.from_numpy(pose).to(rig.dev))
        assert ref['margin'] >= 0.25                                          # every 8 v + 0.5 is a dyadic rational far from an integer
        assert ref['count'].tolist() == [ROWS + (ROWS - 2)] * 3               # the NaN track is gone, joint 4 and its limb 2-4 of the last one too
    finally:
        rig.handle.set_cameras(rig.P, np.stack([c.F for c in cams]), np.stack([c.RK_INV for c in cams]), np.stack([c.position for c in cams]))


def test_a_lens_table_moves_the_skeleton_onto_the_raw_image_except_for_the_camera_without_coefficients(s1):
    rig, tracks = s1
    K = np.asarray(rig.seq['calib']['K'], dtype=np.float64)
    lens = np.zeros((3, 10))
    lens[:, 0], lens[:, 1], lens[:, 2], lens[:, 3], lens[:, 4] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1]
    lens[0, 5:] = (-0.25, 0.08, 1e-3, -2e-3, 0.01)
    lens[2, 5:] = (0.1, 0.0, 0.0, 5e-4, 0.0)                                  # camera 1 keeps all-zero coefficients
    plain = rig.check(tracks, rig.camera_views())
    rig.handle.set_lens(lens)
    try:
        views = [dict(v, lens=lens[c]) for c, v in enumerate(rig.camera_views())]
        bent = rig.check(tracks, views + [extra_view(rig.P[0], rig.w, rig.h)], extra=rig.P[:1])
    finally:
        rig.handle.set_lens(None)
    assert not np.array_equal(bent['prims'][0], plain['prims'][0]) and not np.array_equal(bent['prims'][2], plain['prims'][2])
    assert np.array_equal(bent['prims'][1], plain['prims'][1])
    assert np.array_equal(bent['prims'][3], plain['prims'][0])                # camera 0's matrix as an extra view: no lens
    rig.check(tracks, rig.camera_views())                                      # and the table is gone again


def test_arguments_are_refused_before_any_device_call(s1):
    rig, _ = s1
    lib, h = rig.handle.lib, rig.handle.raw
    prims = torch.zeros((2, ROWS * 16, 8), dtype=torch.int32, device=rig.dev)
    count = torch.zeros(2, dtype=torch.int32, device=rig.dev)
    extra = torch.zeros((1, 3, 4), dtype=torch.float32, device=rig.dev)
    pal = (C.c_uint32 * 25)(*T.palette())

    def call(handle=h, scene=0, n=2, views=True, extra_ptr=extra.data_ptr(), n_extra=1, palette=pal, cap=ROWS * 16, table=prims.data_ptr(),
             cnt=count.data_ptr(), **view1):
        tv = (_lib.PamOverlayTrackView * 32)()
        for k in range(32):
            tv[k].camera, tv[k].extra, tv[k].width, tv[k].height = 0, 0, 64, 48
        for k, x in view1.items():
            setattr(tv[1], k, x)
        return lib.pam_overlay_tracks(handle, None, scene, n, tv if views else None, C.c_void_p(extra_ptr), n_extra, None, palette, 1, cap,
                                      C.c_void_p(table), C.c_void_p(cnt))

    assert call() == 0 and call(camera=-1) == 0 and call(camera=2, width=65535, height=1) == 0
    torch.cuda.synchronize()
    before = (prims.cpu().numpy(), count.cpu().numpy())
    assert before[1].tolist() == [3 * ROWS, 3 * ROWS]
    for kw in (dict(handle=None), dict(views=False), dict(palette=None), dict(table=None), dict(cnt=None), dict(n=0), dict(n=33),
               dict(camera=3), dict(camera=-2), dict(camera=-1, extra=1), dict(camera=-1, extra=-1), dict(camera=-1, n_extra=0),
               dict(camera=-1, extra_ptr=None), dict(n_extra=-1), dict(width=0), dict(width=65536), dict(height=0), dict(height=65536),
               dict(cap=ROWS * 16 - 1), dict(table=prims.data_ptr() + 8), dict(scene=1), dict(scene=-1)):
        assert call(**kw) == -1, kw
    bare = _lib.Handle(3, rig.handle.params, max_dets=8, max_tracks=16)
    try:
        assert call(handle=bare.raw) == -3                                     # PAM_E_STATE: no cameras
        assert call(handle=bare.raw, n=0) == -1
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert np.array_equal(prims.cpu().numpy(), before[0]) and np.array_equal(count.cpu().numpy(), before[1])      # a refused call writes nothing


class BandedFrame(object):
    """A BGR frame at an odd device address between two bands of `fill`."""

    def __init__(self, frame, fill, shift=1):
        band, n = 2 * GM.GUARD, frame.size
        self.raw = torch.full((band + shift + n + band,), fill, dtype=torch.uint8, device='cuda:0')
        self.lo, self.n, self.fill = band + shift, n, fill
        self.tensor = self.raw[self.lo:self.lo + n].view(frame.shape)
        self.tensor.copy_(torch.from_numpy(frame))

    def damaged(self):
        return int((self.raw[:self.lo] != self.fill).sum() + (self.raw[self.lo + self.n:] != self.fill).sum())


def test_counted_draw_paints_the_first_count_rows_and_clamps():
    lib = _lib.load()
    rng = np.random.default_rng(7)
    sizes = [(97, 61), (64, 48), (200, 150), (97, 61)]
    P = np.array([[100.0, 0, 48, 0], [0, 100.0, 30, 0], [0, 0, 1, 0]])
    people = [dict(track_id=k, emitted=True, pose3d=np.concatenate([rng.uniform(-0.6, 0.6, (17, 2)), rng.uniform(1.5, 2.5, (17, 1))], axis=1))
              for k in range(3)]
    cap = 4 * ROWS
    ref = T.table(people, [dict(P=P, w=w, h=h) for w, h in sizes], cap)
    assert ref['count'].tolist() == [3 * ROWS] * 4
    table = torch.from_numpy(ref['prims'].reshape(-1, 8)).cuda()
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    # view 0: its own count; view 1: none; view 2: a count beyond the host's range (2 tracks) clamps to it; view 3: a negative count
    dev_count = torch.tensor([3 * ROWS, 0, 1 << 30, -5], dtype=torch.int32, device='cuda:0')
    host_range = [cap, cap, 2 * ROWS, cap]
    effective = [3 * ROWS, 0, 2 * ROWS, 0]
    for fill in (0xE5, 0x1A):
        banded = [BandedFrame(f, fill, shift=1 + v) for v, f in enumerate(frames)]
        again = [BandedFrame(f, fill, shift=2 + v) for v, f in enumerate(frames)]
        dv, hv = (_lib.PamOverlayView * 4)(), (_lib.PamOverlayView * 4)()
        for v in range(4):
            for views, b, n in ((dv, banded[v], host_range[v]), (hv, again[v], effective[v])):
                views[v].dev_bgr, views[v].width, views[v].height = b.tensor.data_ptr(), sizes[v][0], sizes[v][1]
                views[v].prim_first, views[v].prim_count = v * cap, n
        assert lib.pam_overlay_draw_counted(None, 4, dv, table.data_ptr(), 4 * cap, dev_count.data_ptr()) == 0
        assert lib.pam_overlay_draw(None, 4, hv, table.data_ptr(), 4 * cap) == 0
        torch.cuda.synchronize()
        for v in range(4):
            want = T.paint(frames[v], ref['prims'][v], effective[v])
            got = banded[v].tensor.cpu().numpy()
            assert banded[v].damaged() == 0 and again[v].damaged() == 0, v
            assert np.array_equal(got, want), (v, int((got != want).any(axis=2).sum()))
            assert np.array_equal(again[v].tensor.cpu().numpy(), got)          # host counts through pam_overlay_draw: the same bytes
            assert np.array_equal(want, frames[v]) == (effective[v] == 0)
    assert lib.pam_overlay_draw_counted(None, 4, dv, table.data_ptr(), 4 * cap, None) == -1
    assert lib.pam_overlay_draw_counted(None, 0, dv, table.data_ptr(), 4 * cap, dev_count.data_ptr()) == -1
    torch.cuda.synchronize()


W1, H1, NF1 = 360, 288, 8


def pipeline_case(one_euro, overlap, tmp_path):
    import jpeg_enc_ref as E
    from pam.egress import FrameWriter
    from pam.pipeline import FramePipeline
    rig = Rig('S1', NF1)
    cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
    nd_all, dd_all = synth.pack_frames(rig.seq['frames'], 8)
    p = FramePipeline(rig.cams, cfg, conf, (H1, W1), max_dets=8, max_tracks=16, hrnet=False, one_euro=one_euro, overlap_tracker=overlap,
                      overlay=dict(view3d=dict(size=(320, 240), azimuth=20.0, elevation=30.0), emitted_only=True))
    background = p.view3d_background.cpu().numpy()
    assert (background != background[0, 0]).any()                              # a grid and camera discs, not a blank canvas
    P3 = p.overlay['view3d']['P']
    views = rig.camera_views() + [extra_view(P3, 320, 240)]
    rng = np.random.default_rng(9)
    clean = [rng.integers(0, 256, (H1, W1, 3), dtype=np.uint8) for _ in range(3)]
    writer = FrameWriter(0, workers=2, depth=2)
    store, wanted, drawn = str(tmp_path), {}, 0
    for t in range(NF1):
        nd = torch.tensor(nd_all[t], dtype=torch.int32, device=p.device); dd = torch.tensor(dd_all[t], dtype=torch.float64, device=p.device)
        frames = [torch.from_numpy(f).to(p.device) for f in clean]
        with recorded_calls() as calls:
            p.write_local(dd); p.track_step(t, nd, fetch=False)
            out = p.overlay_step(frames)
        assert [c for c in calls if c.startswith('pam_')] == ['pam_frame_dev_views'] + (['pam_one_euro'] if one_euro else []) + list(NEW_CALLS)
        assert len(out) == 4 and all(a is b for a, b in zip(out, frames)) and out[3] is p.view3d_canvas
        paths = [os.path.join(store, '%d_%d.jpg' % (t, c)) for c in range(3)] + [os.path.join(store, '%d_3d.jpg' % t)]
        writer.submit(t, out, paths)
        got = [f.cpu().numpy() for f in out]                                   # (the copies run on the consumer's stream, behind the draw)
        st = p.track_stream.cuda_stream if p.track_stream is not None else p.stream_ptr()
        p.handle.fetch(st, p.out_i.numpy(), p.out_d.numpy())                   # the record, fetched separately for the check
        rec = p.results()
        tracks = rec['tracks']
        if one_euro:
            filtered = p._oe.dev[0].cpu().numpy()[0]
            tracks = [dict(tr, pose3d=filtered[i]) for i, tr in enumerate(tracks)]
        ref = T.table(tracks, views, ROWS * 16)
        assert ref['margin'] > 1e-6
        for v in range(4):
            want = T.paint(clean[v] if v < 3 else background, ref['prims'][v], ref['count'][v])
            assert np.array_equal(got[v], want), (t, v)
            wanted[paths[v]] = E.encode_bgr(want)
        drawn += int(ref['count'].sum())
    writer.close()
    assert drawn > 4 * ROWS * 3
    for path, data in wanted.items():
        assert open(path, 'rb').read() == data, path
    return p, rec


def test_pipeline_overlay_step_draws_every_frame_from_the_device_state(tmp_path):
    pipeline_case(None, False, tmp_path)


def test_pipeline_overlay_step_draws_the_filtered_poses_behind_the_tracker_stream(tmp_path):
    p, rec = pipeline_case(True, True, tmp_path)
    assert p.track_stream is not None
    raw = T.table(rec['tracks'], [dict(P=np.asarray(p.cams[0].P, dtype=np.float32), w=W1, h=H1)], ROWS * 16)
    filt = T.table([dict(tr, pose3d=p._oe.dev[0].cpu().numpy()[0][i]) for i, tr in enumerate(rec['tracks'])],
                   [dict(P=np.asarray(p.cams[0].P, dtype=np.float32), w=W1, h=H1)], ROWS * 16)
    assert not np.array_equal(raw['prims'], filt['prims'])                     # the filter moved what was drawn


def test_without_the_option_nothing_new_is_called_or_allocated():
    from pam.pipeline import FramePipeline
    rig = Rig('S1', 3)
    cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
    nd_all, dd_all = synth.pack_frames(rig.seq['frames'], 8)
    with recorded_calls() as calls:
        p = FramePipeline(rig.cams, cfg, conf, (H1, W1), max_dets=8, max_tracks=16, hrnet=False)
        for t in range(3):
            nd = torch.tensor(nd_all[t], dtype=torch.int32, device=p.device); dd = torch.tensor(dd_all[t], dtype=torch.float64, device=p.device)
            p.write_local(dd); p.track_step(t, nd)
            p.results()
    assert not [c for c in calls if c in NEW_CALLS + ('pam_overlay_draw',)] and calls.count('pam_frame_dev_views') == 3
    assert p.overlay is None and not hasattr(p, 'view3d_canvas') and not hasattr(p.handle, '_overlay_tables')
    with pytest.raises(ValueError):
        p.overlay_step([])
    with pytest.raises(ValueError):
        FramePipeline(rig.cams, cfg, conf, (H1, W1), max_dets=8, max_tracks=16, hrnet=False, shard='crops', overlay=dict())
    with pytest.raises(ValueError):
        FramePipeline(rig.cams, cfg, conf, (H1, W1), max_dets=8, max_tracks=16, hrnet=False, overlay=dict(view_3d=None))


def test_draw_tracks_device_draws_what_draw_tracks_draws_on_the_device(s1):
    """visualization.draw_tracks_device from the state against draw_tracks(device=True) from the decoded record: the same pixels (no
    coordinate of this seed sits within an ulp of a rounding boundary: the margin is asserted)."""
    rig, tracks = s1
    rng = np.random.default_rng(11)
    clean = [rng.integers(0, 256, (rig.h, rig.w, 3), dtype=np.uint8) for _ in range(rig.C)]
    a = [torch.from_numpy(f).cuda() for f in clean]
    b = [torch.from_numpy(f).cuda() for f in clean]
    with recorded_calls() as calls:
        assert V.draw_tracks_device(rig.handle, a)[0] is a[0]
    assert [c for c in calls if c.startswith('pam_')] == list(NEW_CALLS)
    V.draw_tracks(b, rig.cams, rig.trk.tracks, device=True)
    torch.cuda.synchronize()
    ref = T.table(tracks, rig.camera_views(), ROWS * 16)
    assert ref['margin'] > 1e-6
    for v in range(rig.C):
        got = a[v].cpu().numpy()
        assert np.array_equal(got, T.paint(clean[v], ref['prims'][v], ref['count'][v])) and not np.array_equal(got, clean[v])
        assert np.array_equal(got, b[v].cpu().numpy())


def test_demo_loop_draws_the_tracks_and_the_3d_view_from_the_device_state(tmp_path, monkeypatch):
    """testmodel's loop with DATASET.OVERLAY_TRACKS and DATASET.VIEW3D: per drawn frame the per-camera files and <frame>_3d.jpg, each
    byte for byte the restatements' (the tracks of that frame's record, rastered and encoded on the host)."""
    import pickle
    from PIL import Image
    import jpeg_enc_ref as E
    import jpeg_ref as J
    import pam
    from pam import testmodel
    from pam.dataset import GetConfig, LoadFilenames, LoadImages
    n_frames = 5
    root = tmp_path / 'seq' / 'CampusSeq1'
    seq = synth.make_sequence('S1', n_frames=n_frames, seed=2)
    for c in range(3):
        os.makedirs(root / ('Camera%d' % c))
        for t in range(n_frames):
            Image.fromarray(J.content('smooth', W1, H1, 10 * c + t)).save(root / ('Camera%d' % c) / ('%04d.png' % t))
    with open(root / 'camera_parameter.pickle', 'wb') as f:
        pickle.dump(seq['calib'], f)
    pre = {}
    for t, views in enumerate(seq['frames']):
        _, dr = synth.to_dump_results(views)
        pre[t] = [[dict(bbox=d['bbox'], keypoints=d['keypoints'], keypoints_score=d['keypoints_score']) for d in v] for v in dr]
    with open(root / 'detections.pickle', 'wb') as f:
        pickle.dump(pre, f)
    cfg = GetConfig(os.path.join(pam.PKG_DIR, 'configs', 'CampusSeq1', 'model_configs.yaml'))
    cfg.DATASET.ROOT = str(root); cfg.DATASET.DATA_FORMAT = '*.png'; cfg.DATASET.TEST_RANGE = [0, n_frames]
    cfg.OUTPUT = str(tmp_path / 'out'); cfg.SAVE_IMAGE = True
    cfg.PIPELINE_COMBINATION.POSE_MODEL = 'Precomputed'
    view3d = dict(SIZE=[320, 240], AZIMUTH=20.0, ELEVATION=40.0)
    cfg.DATASET.DEVICE_OVERLAY, cfg.DATASET.OVERLAY_TRACKS, cfg.DATASET.VIEW3D, cfg.DATASET.WRITER_DEPTH = True, True, view3d, 2
    files = LoadFilenames(cfg.DATASET)
    built, seen = {}, []
    build = testmodel.build_model
    monkeypatch.setattr(testmodel, 'build_model', lambda c: built.setdefault('model', build(c)))

    def on_frame(fid, ts, res):
        if res is not None:
            seen.append((fid, [dict(track_id=tr['track_id'], pose3d=tr['pose3d'].copy(), emitted=tr['emitted'])
                               for tr in built['model'][0].tracker.last['tracks']]))
    with recorded_calls() as calls:
        testmodel.test_ivclabpose_PersonTrack_Project3DPose(cfg, files, on_frame=on_frame)
    torch.cuda.synchronize()
    store = os.path.join(cfg.OUTPUT, 'CampusSeq1', 'Images')
    saved = {n: open(os.path.join(store, n), 'rb').read() for n in sorted(os.listdir(store))}
    assert len(seen) > 2 and sorted(saved) == sorted(['%s_%d.jpg' % (fid, c) for fid, _ in seen for c in range(3)] + ['%s_3d.jpg' % fid for fid, _ in seen])
    assert calls.count('pam_overlay_tracks') == calls.count('pam_overlay_draw_counted') == len(seen) and calls.count('pam_overlay_draw') == 1
    cams = built['model'][0].cameras
    P3 = V.view3d_camera(cams, (320, 240), azimuth=20.0, elevation=40.0)
    background = V.view3d_background(cams, P3, (320, 240)).cpu().numpy()
    views = [dict(P=np.asarray(c.P, dtype=np.float32), w=W1, h=H1) for c in cams] + [dict(P=P3, w=320, h=240)]
    drawn = 0
    for fid, tracks in seen:
        frames, _ = LoadImages('CampusSeq1', files[fid])
        ref = T.table(tracks, views, ROWS * 32)
        assert ref['margin'] > 1e-6
        for v, name in enumerate(['%s_%d.jpg' % (fid, c) for c in range(3)] + ['%s_3d.jpg' % fid]):
            assert saved[name] == E.encode_bgr(T.paint(frames[v] if v < 3 else background, ref['prims'][v], ref['count'][v])), name
        drawn += int(ref['count'].sum())
    assert drawn > 4 * ROWS
    cfg.DATASET.DEVICE_OVERLAY = False
    with pytest.raises(ValueError):
        testmodel.test_ivclabpose_PersonTrack_Project3DPose(cfg, files)
