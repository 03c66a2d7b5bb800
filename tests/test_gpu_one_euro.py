"""GPU: the One-Euro filter on the tracks' 3D output (pam_op_one_euro, pam_set_one_euro, pam_one_euro; csrc/pam_one_euro.hip).

The step against the outputs of the reference's own class (tests/golden/one_euro.npz): every operation of the step is a correctly rounded
IEEE float64 + - * / or fabs and the library is built without contraction, so the expectation is equality of bits.  The life cycle on
the golden traces S1 and S3 (S3: births, deaths, slot reuse, skipped frames) against tests/one_euro_ref.Bank fed with the record's own
raw poses, in the same run as a tracker without the option whose 9-tuple must not differ in a bit."""
import ctypes

import numpy as np
import pytest
import torch

import golden_io as G
import one_euro_ref as R
from oracle import cpu_ref as O
from pam import _lib, synth
import tracker_matrix as M

pytestmark = pytest.mark.gpu

MD = 8            # detections per view (S3 has up to 7)


def same_bits(got, want, what):
    """The criterion of this file: equal bits.  The largest difference is printed first, so that a run that fails says by how much."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = float(np.abs(got - want).max()) if got.size else 0.0
    if d != 0.0:
        print('%s: largest difference %.3g' % (what, d))
    assert np.array_equal(got, want), '%s: largest difference %.3g' % (what, d)


@pytest.fixture(scope='module')
def seqs():
    return R.golden_sequences()


def _handle(size, max_tracks, n_scenes=1, max_dets=MD):
    c = G.cameras(size)
    tr = G.load('trace_%s.npz' % size)
    cfg = dict(synth.MATCHER_CFG[str(tr['meta.dataset'])]); conf = cfg.pop('CONF_THRESHOLD')
    cams = O.cameras_from_arrays(c['P32'], c['K32'], c['RT32'], c['F'], c['RK_INV'], c['position'])
    h = _lib.Handle(len(cams), _lib.make_params(cfg, conf), max_dets=max_dets, max_tracks=max_tracks, n_scenes=n_scenes)
    h.set_cameras(np.stack([x.P for x in cams]), np.stack([x.F for x in cams]), np.stack([x.RK_INV for x in cams]),
                  np.stack([x.position for x in cams]))
    return h, G.trace_frames(tr)


def test_op_against_every_golden_sequence(seqs):
    h, _ = _handle('S1', 4)
    try:
        assert {s['K'] for s in seqs} == {1, 51, 300} and any(s['n'] == 1 for s in seqs)          # one lane, a track, two workgroups; one sample
        worst = 0.0
        for i, s in enumerate(seqs):
            got = h.op_one_euro(s['t'], s['x'], s['cfg'])
            worst = max(worst, float(np.abs(got - s['out']).max()))
            assert got[0].tobytes() == s['x'][0].tobytes(), 'sequence %d: a first sample must come back as it went in' % i
        print('pam_op_one_euro against the reference class: largest difference %.3g over %d sequences' % (worst, len(seqs)))
        for i, s in enumerate(seqs):
            same_bits(h.op_one_euro(s['t'], s['x'], s['cfg']), s['out'], 'sequence %d (n %d, K %d)' % (i, s['n'], s['K']))
        assert h.op_one_euro(np.zeros(0), np.zeros((0, 3))).shape == (0, 3)
        cfg = _lib.one_euro_config(True)
        buf = np.zeros(4)
        for n, K in ((-1, 1), (1, 0), (1, 4097)):
            assert h.lib.pam_op_one_euro(h.raw, n, K, _lib._ptr(buf), _lib._ptr(buf), ctypes.byref(cfg), _lib._ptr(buf)) == -1
        bad = _lib.PamOneEuro(0.0, 0.8, 0.4, 0.4)
        assert h.lib.pam_op_one_euro(h.raw, 1, 1, _lib._ptr(buf), _lib._ptr(buf), ctypes.byref(bad), _lib._ptr(buf)) == -1
    finally:
        h.close()


def _facade(size, one_euro, max_tracks):
    from pam.ivclabpose import ivclabpose
    tr = G.load('trace_%s.npz' % size)
    c = G.cameras(size)
    cfg = dict(synth.MATCHER_CFG[str(tr['meta.dataset'])]); conf = cfg.pop('CONF_THRESHOLD')
    m = dict(cfg, NAME='Iterative')
    if one_euro:
        m['ONE_EURO'] = {}
    model = ivclabpose({'NAME': ''}, None, m, conf, max_dets=MD, max_tracks=max_tracks)
    model.GetCameraParameters({'P': c['P'], 'K': c['K'], 'RT': c['RT']}, 0, 0, F=c['F'])
    return model, G.trace_frames(tr)


def _check_rows(tracks, rows, t):
    for tr, (pose, fresh, samples) in zip(tracks, rows):
        assert tr.filter_fresh == fresh and tr.filter_samples == samples, (t, tr.track_id, tr.filter_fresh, fresh, tr.filter_samples, samples)
        same_bits(tr.pose3d_filtered.ravel(), pose, 'frame %d track %d' % (t, tr.track_id))


@pytest.mark.parametrize('size,max_tracks', [('S1', 8), ('S3', 8)])
def test_life_cycle_on_a_golden_trace(size, max_tracks):
    on, frames = _facade(size, True, max_tracks)
    off, _ = _facade(size, False, max_tracks)
    assert off.tracker.one_euro is None and off.pts3d_filtered is None
    bank, ids, held, moved, n_rows, tentative = R.Bank(), set(), 0, 0, 0, 0
    for t, views in enumerate(frames):
        if not any(len(v) for v in views):
            continue                                          # the drivers skip frames without any pose
        pbl, dr = synth.to_dump_results(views)
        a = on.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        b = off.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        # the filter does not feed back: the 9-tuple and the whole record are those of a tracker without it, bit for bit
        assert list(a[5]) == list(b[5]) and a[4] == b[4] and a[2] == b[2], t
        assert [list(map(int, c)) for c in a[0]] == [list(map(int, c)) for c in b[0]], t
        assert np.asarray(a[3]).tobytes() == np.asarray(b[3]).tobytes(), t
        assert np.array_equal(on.tracker.handle.out_i, off.tracker.handle.out_i), t
        k = on.tracker.handle.layout.dbl_hdr_words            # (the header words are in-kernel clocks)
        assert np.array_equal(on.tracker.handle.out_d[:, k:], off.tracker.handle.out_d[:, k:]), t
        assert all(x.pose3d_filtered is None and x.filter_fresh is None for x in off.tracker.tracks)
        trs = on.tracker.tracks                               # ALL listed tracks, tentative included
        rows = bank.frame(t, [(x.track_id, x.last_time, x.pose3d.ravel()) for x in trs])
        _check_rows(trs, rows, t)
        assert on.tracker.last['one_euro']['n_fresh'] == sum(x.filter_fresh for x in trs)
        ids |= {x.track_id for x in trs}
        held += sum(1 for x in trs if not x.filter_fresh and x.filter_samples > 0)
        moved += sum(1 for x in trs if x.filter_samples > 1 and not np.array_equal(x.pose3d_filtered, x.pose3d))
        n_rows += len(trs)
        tentative += sum(1 for x in trs if x.is_tentative())
        # the facade: the filtered poses of the emitted tracks, aligned with pts3d
        em = [x for x in trs if x.emitted]
        assert on.pts3d_filtered.shape == ((len(em), 3, 17) if em else (0,))
        for i, x in enumerate(em):
            assert int(a[5][i]) == x.track_id and np.array_equal(on.pts3d_filtered[i], x.pose3d_filtered.T)
    assert n_rows > 300 and moved > 200 and tentative > 0          # rows were compared, the filter moved them, tentative tracks among them
    assert held > 0, 'no track was held over a gap'
    if size == 'S3':
        # more tracks over the run than the handle has slots: that many filters at least started over in a slot another track had used
        reused = len(ids) - max_tracks
        print('S3: %d ids in %d slots, %d held rows, %d filtered rows' % (len(ids), max_tracks, held, moved))
        assert reused > 0, 'no filter restarted in a reused slot'


def test_idempotence_reset_and_switching_off():
    a, frames = _facade('S1', True, 8)
    b, _ = _facade('S1', True, 8)
    hb = b.tracker.handle
    pose2, meta2 = hb.one_euro_buffers()
    st = torch.cuda.current_stream().cuda_stream
    for t, views in enumerate(frames[:40]):
        if not any(len(v) for v in views):
            continue
        pbl, dr = synth.to_dump_results(views)
        a.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        b.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        for _ in range(2):                                    # the same frame again, twice: identical buffers ...
            hb.one_euro(st, t, pose2, meta2)
            hb.sync(st)
            assert torch.equal(pose2.cpu(), b.tracker._oe.host[0]) and torch.equal(meta2.cpu(), b.tracker._oe.host[1]), t
        for x, y in zip(a.tracker.tracks, b.tracker.tracks):  # ... and identical results on every later frame
            assert x.track_id == y.track_id and x.filter_samples == y.filter_samples and x.filter_fresh == y.filter_fresh
            assert x.pose3d_filtered.tobytes() == y.pose3d_filtered.tobytes(), t
    assert max(x.filter_samples for x in a.tracker.tracks) > 20
    # track_restart: pam_reset restarts every filter -- the first frame's output is the raw pose's bits
    a.tracker.track_restart()
    pbl, dr = synth.to_dump_results(frames[40])
    a.PersonTrack_Project3DPose(40, pbl, dr, 'SVD')
    assert len(a.tracker.tracks) > 0
    for x in a.tracker.tracks:
        assert x.filter_fresh and x.filter_samples == 1 and x.pose3d_filtered.tobytes() == x.pose3d.tobytes()
    # setting the configuration again restarts too; NULL switches off
    a.tracker.handle.set_one_euro(dict(beta=0.0))
    a.PersonTrack_Project3DPose(41, *synth.to_dump_results(frames[41]), 'SVD')
    assert all(x.filter_samples == 1 and x.pose3d_filtered.tobytes() == x.pose3d.tobytes() for x in a.tracker.tracks if x.filter_fresh)
    ha = a.tracker.handle
    pose, meta = ha.one_euro_buffers()
    assert ha.lib.pam_one_euro(ha.raw, ctypes.c_void_p(st), 42, None, ctypes.c_void_p(meta.data_ptr())) == -1
    assert ha.lib.pam_one_euro(ha.raw, ctypes.c_void_p(st), 42, ctypes.c_void_p(pose.data_ptr()), None) == -1
    ha.set_one_euro(None)
    assert ha.lib.pam_one_euro(ha.raw, ctypes.c_void_p(st), 42, ctypes.c_void_p(pose.data_ptr()), ctypes.c_void_p(meta.data_ptr())) == -3
    with pytest.raises(_lib.PamError):
        ha.one_euro(st, 42, pose, meta)
    for bad in (dict(freq=0), dict(mincutoff=-1.0), dict(dcutoff=0.0)):
        c = _lib.PamOneEuro(*[float(dict(_lib.ONE_EURO_3D, **bad)[k]) for k in ('freq', 'mincutoff', 'beta', 'dcutoff')])
        assert ha.lib.pam_set_one_euro(ha.raw, ctypes.byref(c)) == -1
    c = _lib.PamOneEuro(25.0, 0.8, float('inf'), 0.4)
    assert ha.lib.pam_set_one_euro(ha.raw, ctypes.byref(c)) == -1


def _drive(h, t, nd, dd, bufs, st):
    """One frame on device inputs (no overflow error on this path: the status word alone says so), the filter behind it."""
    n_t = torch.tensor(nd, dtype=torch.int32, device='cuda'); d_t = torch.tensor(dd, dtype=torch.float64, device='cuda')
    h.frame_dev(st, t, n_t.data_ptr(), d_t.data_ptr())
    h.one_euro(st, t, *bufs)
    h.fetch(st); h.sync(st)
    return bufs[0].cpu().numpy(), bufs[1].cpu().numpy()


def _check_scene(h, scene, t, pose, meta, bank):
    rec = h.decode(scene)
    f = _lib.Handle.decode_one_euro(pose, meta, scene)
    assert f['n_tracks'] == rec['n_tracks'] and f['ids'].tolist() == [x['track_id'] for x in rec['tracks']]
    rows = bank.frame(t, [(x['track_id'], x['last_time'], x['pose3d'].ravel()) for x in rec['tracks']])
    for k, (want, fresh, samples) in enumerate(rows):
        assert bool(f['fresh'][k]) == fresh and int(f['samples'][k]) == samples, (scene, t, k)
        same_bits(f['pose'][k].ravel(), want, 'scene %d frame %d row %d' % (scene, t, k))
    assert not pose[scene, rec['n_tracks']:].any() and f['n_fresh'] == int(f['fresh'].sum())
    assert meta[scene, 2 + 3 * rec['n_tracks']:].reshape(-1, 3).tolist() == [[-1, 0, 0]] * (h.max_tracks - rec['n_tracks'])
    return rec


def _small_rig(monkeypatch, persons, max_tracks, n_frames):
    """A 3-view synthetic rig with `persons` people (no capacity overflow at max_tracks >= persons) -> handle, packed frames."""
    size = M.add_rig(monkeypatch, 3, persons)
    seq = synth.make_sequence(size, n_frames=n_frames, seed=11)
    h = M.handle_for(_lib, size, O.make_cameras(seq['calib']), MD, max_tracks)
    return h, synth.pack_frames(seq['frames'], MD)


def test_one_track_slot(monkeypatch):
    h, (nd, dd) = _small_rig(monkeypatch, 1, 1, 30)
    try:
        h.set_one_euro(True)
        bufs, st, bank, seen = h.one_euro_buffers(), torch.cuda.current_stream().cuda_stream, R.Bank(), 0
        assert tuple(bufs[0].shape) == (1, 1, 17, 3) and tuple(bufs[1].shape) == (1, 5)
        for t in range(30):
            pose, meta = _drive(h, t, nd[t:t + 1], dd[t:t + 1], bufs, st)
            rec = _check_scene(h, 0, t, pose, meta, bank)
            assert rec['status'] == 0
            seen += rec['n_tracks']
        assert seen >= 20 and bank.groups and max(g.hdr.n for g in bank.groups.values()) >= 20
    finally:
        h.close()


def test_two_scenes_in_one_handle():
    h, frames = _handle('S3', 8, n_scenes=2)
    try:
        h.set_one_euro(True)
        nd, dd = synth.pack_frames(frames, MD)              # every frame is submitted, the trace's empty ones included
        nd2, dd2 = nd.copy(), dd.copy()
        nd2[:10] = 0                                          # scene 1: the same trace with its first 10 frames emptied
        bufs, st, banks = h.one_euro_buffers(), torch.cuda.current_stream().cuda_stream, [R.Bank(), R.Bank()]
        differ = 0
        for t in range(len(frames)):
            pose, meta = _drive(h, t, np.stack([nd[t], nd2[t]]), np.stack([dd[t], dd2[t]]), bufs, st)
            recs = [_check_scene(h, s, t, pose, meta, banks[s]) for s in (0, 1)]
            if t < 10:
                assert recs[1]['n_tracks'] == 0 and recs[0]['n_tracks'] > 0 and not pose[1].any()
            differ += recs[0]['n_tracks'] > 0 and recs[1]['n_tracks'] > 0 and not np.array_equal(pose[0], pose[1])
        assert differ > 20                                    # the scenes' filters hold different histories: nothing is shared
        assert all(len(b.groups) > h.max_tracks for b in banks)   # more ids than slots in both scenes: slots were reused
    finally:
        h.close()


def test_outputs_in_guarded_memory(monkeypatch):
    """dev_pose / dev_meta carved from the sentinel arena at 1 scene x 3 tracks, two of them alive: every element is written, the rows
    from n_tracks on are zero, the bands on both sides of both buffers stay intact."""
    import guarded_mem as GM
    h, (nd, dd) = _small_rig(monkeypatch, 2, 3, 8)
    try:
        h.set_one_euro(True)
        arena = GM.GuardArena(torch.device('cuda'), 1 << 20)
        st = torch.cuda.current_stream().cuda_stream
        bank, most = R.Bank(), 0
        for t in range(-1, 8):
            if t >= 0:
                n_t = torch.tensor(nd[t:t + 1], dtype=torch.int32, device='cuda'); d_t = torch.tensor(dd[t:t + 1], dtype=torch.float64, device='cuda')
                h.frame_dev(st, t, n_t.data_ptr(), d_t.data_ptr())
            pose = arena.alloc(1, 1, 1, 3 * 51 * 4)           # 3 tracks x 51 doubles and 2 + 3 * 3 int32 words, as 2-byte elements
            meta = arena.alloc(1, 1, 1, 11 * 2)
            assert h.lib.pam_one_euro(h.raw, ctypes.c_void_p(st), max(t, 0), ctypes.c_void_p(pose.data_ptr()), ctypes.c_void_p(meta.data_ptr())) == 0
            h.fetch(st); h.sync(st)
            assert arena.report() == '', arena.report()       # every element written, every band intact
            p = arena.payload(arena.allocs[-2]).view(torch.float64).cpu().numpy().reshape(1, 3, 17, 3)
            m = arena.payload(arena.allocs[-1]).view(torch.int32).cpu().numpy().reshape(1, 11)
            if t < 0:                                         # before the first frame: no track, every row zero
                assert m.tolist() == [[0, 0] + [-1, 0, 0] * 3] and not p.any()
            else:
                rec = _check_scene(h, 0, t, p, m, bank)       # (checks the zero rows from n_tracks on)
                assert rec['status'] == 0
                most = max(most, rec['n_tracks'])
        assert 0 < most < 3
    finally:
        h.close()
