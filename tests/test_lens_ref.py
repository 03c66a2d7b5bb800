"""The lens model on the CPU: tests/lens_ref.py (the restatement the GPU tests compare the kernel with) pinned by a 50-digit evaluation of
the forward model and by the round trip, Camera.undistort_points / distort_points / projectPoints against it, four planted faults that
must break the tolerance, and the precondition of the GPU trace tests.

Truth is by construction: ideal points -> closed-form forward model -> the inverse must return them, within lens_ref.TOL_PX = 1e-9 px on
every grid point of the four coefficient sets (the float64 floor measured when the model was specified is 1.1e-12 px from iteration 5
on; 8 steps are run)."""
import numpy as np
import pytest

import lens_ref as L
from oracle import cpu_ref as O
from pam import synth
from pam.ivclabpose import Camera


def _camera(name, dist='set'):
    s = L.SETS[name]
    fx, fy, cx, cy, skew = s['k']
    K = np.array([[fx, skew, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
    RT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    return Camera(0, K @ RT, K, RT, None, w=s['wh'][0], h=s['wh'][1], distCoef=s['dist'] if dist == 'set' else dist)


@pytest.mark.parametrize('name', L.ORDER)
def test_forward_model_against_50_digits(name):
    s = L.SETS[name]
    pts = L.grid(name, step=s['wh'][0] / 12.0)
    assert len(pts) >= 60
    n = L.to_norm(s['k'], pts)
    got = L.forward(s['dist'], n)
    worst = 0.0
    for (x, y), (gx, gy) in zip(n, got):
        tx, ty = L.forward_mp(s['dist'], x, y)
        bx, by = L.forward_bound(s['dist'], x, y)
        ex, ey = abs(float(gx - tx)), abs(float(gy - ty))
        worst = max(worst, ex / max(bx, 1e-300), ey / max(by, 1e-300))
        assert ex <= bx and ey <= by, (name, x, y, ex, bx, ey, by)
    print('%s: forward model within %.3f of its rounding bound on %d points' % (name, worst, len(pts)))


@pytest.mark.parametrize('name', L.ORDER)
def test_round_trip_on_the_grid(name):
    s = L.SETS[name]
    pts = L.grid(name)
    assert len(pts) > 2000
    raw = L.distort_px(s['k'], s['dist'], pts)
    back, ok = L.undistort_px(s['k'], s['dist'], raw)
    err = np.abs(back - pts).max()
    print('%s: %d points, largest move %.1f px, round trip %.3g px' % (name, len(pts), np.hypot(*(raw - pts).T).max(), err))
    assert ok.all() and err <= L.TOL_PX
    assert np.hypot(*(raw - pts).T).max() > 20.0                 # the grid reaches where the lens matters


@pytest.mark.parametrize('fault', L.FAULTS)
def test_planted_faults_break_the_tolerance(fault):
    for name in L.ORDER:
        s = L.SETS[name]
        pts = L.grid(name)
        raw = L.distort_px(s['k'], s['dist'], pts)
        back, _ = L.undistort_px(s['k'], s['dist'], raw, fault=fault)
        err = np.abs(back - pts).max()
        if fault == 'no_k3' and s['dist'][4] == 0.0:
            assert err <= L.TOL_PX                                # (the set has no k3 to drop)
            continue
        assert err > 1000 * L.TOL_PX, (fault, name, err)


@pytest.mark.parametrize('name', L.ORDER)
def test_camera_points_against_the_restatement(name):
    s = L.SETS[name]
    cam = _camera(name)
    pts = L.grid(name)
    raw = L.distort_px(s['k'], s['dist'], pts)
    got_raw = cam.distort_points(pts)
    assert got_raw.shape == pts.shape and np.abs(got_raw - raw).max() <= L.TOL_PX
    got = cam.undistort_points(raw)
    want, ok = L.undistort_px(s['k'], s['dist'], raw)
    assert ok.all() and np.abs(got - want).max() <= L.TOL_PX and np.abs(got - pts).max() <= L.TOL_PX
    # rows (x, y, w): the third column is not a coordinate
    rows = np.concatenate([raw, np.arange(len(raw), dtype=np.float64)[:, None]], axis=1)
    got3 = cam.undistort_points(rows)
    assert np.array_equal(got3[:, 2], rows[:, 2]) and np.array_equal(got3[:, :2], got)
    assert np.array_equal(rows[:, :2], raw)                       # the input is not written


def test_camera_points_the_model_cannot_invert_stay():
    s = L.SETS['barrel']
    cam = _camera('barrel')
    beyond = np.array([[s['k'][2] + 1.7 * s['k'][0], s['k'][3]], [np.nan, 5.0], [100.0, np.inf]])
    n0 = L.to_norm(s['k'], beyond[:1])
    assert L.det2(L.jacobian(s['dist'], n0))[0] <= 0              # the start of the iteration lies beyond the model's fold
    got = cam.undistort_points(beyond)
    assert np.array_equal(got, beyond, equal_nan=True)
    _, ok = L.undistort_px(s['k'], s['dist'], beyond)
    assert not ok.any()


def test_camera_without_coefficients_is_the_pinhole_of_before():
    pts = L.grid('vga')[::50]
    for cam in (_camera('vga', None), _camera('vga', (0, 0, 0, 0, 0))):
        assert cam.lens is None
        assert cam.undistort_points(pts) is pts and cam.distort_points(pts) is pts
        X = np.random.default_rng(0).uniform(-1, 1, (17, 3)) + [0, 0, 6]
        assert np.array_equal(cam.projectPoints(X), cam.projectPoints_undist(X))
        assert np.array_equal(cam.projectPoints(X), cam.projectPoints_parallel(X[None])[0])
    with pytest.raises(TypeError):
        Camera(0, None, None, None, None, distcoef=None)         # (the keyword is distCoef)


def test_project_points_lands_in_the_raw_image():
    s = L.SETS['hd']
    cam = _camera('hd')
    X = np.random.default_rng(1).uniform(-2.5, 2.5, (17, 3)) * [1, 0.6, 0] + [0, 0, 4]
    ideal = cam.projectPoints_undist(X)                           # (y, x)
    assert np.array_equal(ideal, cam.projectPoints_parallel(X[None])[0])
    raw = cam.projectPoints(X)
    want = L.distort_px(s['k'], s['dist'], ideal[:, ::-1])[:, ::-1]
    assert np.abs(raw - want).max() <= L.TOL_PX and np.abs(raw - ideal).max() > 5.0


def test_get_camera_parameters_reads_distcoef():
    from pam import _lib
    calib = synth.make_rig(3, 360, 288, 400.0)
    K = np.asarray(calib['K'], dtype=np.float64)
    dist = np.tile(np.asarray(L.TRACE_DIST), (3, 1)); dist[1] = 0.0
    table = _lib.lens_table(K, dist)
    assert table.shape == (3, 10) and np.array_equal(table[:, 5:], dist) and table[0, :5].tolist() == [400.0, 400.0, 180.0, 144.0, 0.0]
    assert _lib.lens_table(K, None) is None and _lib.lens_table(K, np.zeros((3, 5))) is None
    with pytest.raises(ValueError):
        _lib.lens_table(K, np.zeros((2, 5)))
    assert _lib.check_lens(table, 3) is not None and _lib.check_lens(table * np.r_[np.ones(5), np.zeros(5)], 3) is None
    with pytest.raises(ValueError):
        _lib.check_lens(table[:2], 3)


def _oracle_trace(calib, frames):
    """Every decision of the CPU oracle on a sequence: per frame (track ids, per-view det -> track, per track its views and their
    times, joints' view counts, state and life-cycle counters)."""
    trk = O.Tracker(O.Params(synth.MATCHER_CFG['CampusSeq1'], 0.4), O.make_cameras(calib))
    out, poses = [], []
    for t, views in enumerate(frames):
        trk.step(t, [d[:, :, [1, 0, 2]] for d in views])
        out.append(([tr.track_id for tr in trk.tracks], [a.tolist() for a in trk.assign],
                    [([(c, tr.p2d[c][0]) for c in tr.order], tr.nviews.tolist(), tr.V, tr.state, tr.hits, tr.age, tr.tsu) for tr in trk.tracks]))
        poses.append([tr.hist[-1].copy() for tr in trk.tracks])
    return out, poses


def test_the_trace_is_decided_alike_on_ideal_and_on_undistorted_rows():
    """The precondition of tests/test_gpu_lens_pipeline.py: on the chosen sequence the oracle, fed the NumPy-undistorted distorted poses,
    gives the ids, matched detections, view sets and life-cycle fields it gives on the ideal poses, on every frame (so that the device
    comparison there is exact); fed the distorted poses as they are it does not (so that the step is needed)."""
    T = L.trace()
    calib = T['seq']['calib']
    back = [L.undistort_views(T['K5'], T['dist'], views) for views in T['raw']]
    moved = max(np.abs(r[..., :2] - i[..., :2]).max() for rv, iv in zip(T['raw'], T['ideal']) for r, i in zip(rv, iv) if len(r))
    err = max(np.abs(b[..., :2] - i[..., :2]).max() for bv, iv in zip(back, T['ideal']) for b, i in zip(bv, iv) if len(b))
    print('trace: the lens moves a keypoint by up to %.1f px, the round trip leaves %.3g px' % (moved, err))
    assert err <= L.TOL_PX and moved > 10.0
    a, pa = _oracle_trace(calib, T['ideal'])
    b, pb = _oracle_trace(calib, back)
    assert a == b
    assert max(len(x[0]) for x in a) >= 3 and len({i for x in a for i in x[0]}) >= 4          # tracks live, die and are born
    d3 = max(np.abs(p - q).max() for fa, fb in zip(pa, pb) for p, q in zip(fa, fb))
    assert d3 <= 1e-9
    c, pc = _oracle_trace(calib, T['raw'])
    assert c != a or max(np.abs(p - q).max() for fa, fc in zip(pa, pc) for p, q in zip(fa, fc)) >= 1000 * max(d3, 1e-12)
