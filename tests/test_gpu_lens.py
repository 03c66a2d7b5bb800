"""pam_undistort_keypoints on the GPU, through ctypes, against tests/lens_ref.py: coordinates within 1e-9 px of the ideal points the
raw points were made from (and of the restatement's inverse), the score column, the rows beyond each view's count and every row of a
pin-hole camera bit-equal, the buffer between sentinel bands that stay intact, points the model cannot invert kept and counted.

Every case first checks on the CPU that the restatement's own verdict on every point is clear (a converged point has a residual 1000
times under the bound, a point that cannot be inverted shows a determinant below -1e-3 within the first three iterates or is not
finite), so that no verdict of the device hangs on its last bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guarded_mem as G
import lens_ref as L

pytestmark = pytest.mark.gpu

J = 17
SCORE0 = 0.123456789
CAMS = L.ORDER + ('pinhole',)


def cam_row(name):
    """The 10 doubles of a camera: one of the four sets, or the VGA-like K with all five coefficients 0.0."""
    if name == 'pinhole':
        return np.array(L.SETS['vga']['k'] + (0.0,) * 5)
    return L.lens_row(name)


def banded(shape, dev):
    """A float64 tensor of `shape` at a 256-byte-aligned address inside an int16 buffer that holds guarded_mem.SENTINEL everywhere, GUARD
    elements of band on each side, the band behind it starting at its last byte + 1 -> (tensor, front band, back band)."""
    n = int(np.prod(shape)) * 4                                   # int16 elements of the payload
    buf = torch.full((n + 2 * G.GUARD + G.ALIGN // 2,), G.as_i16(G.SENTINEL), dtype=torch.int16, device=dev)
    start = G.GUARD + ((-(buf.data_ptr() + 2 * G.GUARD)) % G.ALIGN) // 2
    buf = buf[:start + n + G.GUARD]
    t = buf[start:start + n].view(torch.float64).view(*shape)
    assert t.data_ptr() % G.ALIGN == 0
    return t, buf[:start], buf[start + n:]


@functools.lru_cache(maxsize=None)
def grid_of(name):
    return L.grid(name)


def raw_points(name, fill, n, seed):
    """n raw-image points (x, y) of camera `name` and the ideal points they were made from (None where the fill names raw points)."""
    s = L.SETS['vga' if name == 'pinhole' else name]
    w, h = s['wh']
    if fill == 'grid':
        pts = grid_of('vga' if name == 'pinhole' else name)
        ideal = pts[np.random.default_rng(seed).permutation(len(pts))[:n]]
        return (ideal.copy() if name == 'pinhole' else L.distort_px(s['k'], s['dist'], ideal)), ideal
    if fill == 'corners':
        base = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64)
    else:
        base = np.array([[s['k'][2], s['k'][3]]], dtype=np.float64)
    return base[np.arange(n) % len(base)], None


def clear_verdicts(name, raw):
    """The restatement's verdict on raw points (x, y) of a camera, asserted clear -> (want (.., 2), ok)."""
    if name == 'pinhole':
        return raw.copy(), np.ones(raw.shape[:-1], dtype=bool)
    s = L.SETS[name]
    want, ok = L.undistort_px(s['k'], s['dist'], raw)
    with np.errstate(all='ignore'):
        d = L.to_norm(s['k'], raw)
        n, low = d.copy(), np.full(raw.shape[:-1], np.inf)
        for it in range(L.ITERS):
            Jm = L.jacobian(s['dist'], n)
            dt = L.det2(Jm)
            if it < 3:
                low = np.fmin(low, dt)
            e = L.forward(s['dist'], n) - d
            n = n - np.stack([Jm[..., 1, 1] * e[..., 0] - Jm[..., 0, 1] * e[..., 1],
                              Jm[..., 0, 0] * e[..., 1] - Jm[..., 1, 0] * e[..., 0]], axis=-1) / dt[..., None]
        res = np.abs(L.forward(s['dist'], n) - d).max(axis=-1)
    fin = np.all(np.isfinite(raw), axis=-1)
    assert np.all(res[ok] <= L.RESID / 1000) and np.all(low[ok] > 1e-3)
    assert np.all((low[~ok & fin] < -1e-3))
    return want, ok


def launch(det, n_det, views, lens, info, n_views, max_dets, det_slots, stream=None):
    from pam import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    return _lib.load().pam_undistort_keypoints(C.c_void_p(st), n_views, max_dets, det_slots, p(det), p(n_det), p(views), p(lens), p(info))


def run_case(V, max_dets, extra, permute, counts, fill, cams=None, plant=None, seed=0):
    """One launch.  counts: 'full' | 'mixed' (0, full, above max_dets, negative, and in between).  plant: {(view, slot, joint): (x, y)}
    raw points put in after the fill.  -> dict of everything the assertions need."""
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(1000 * V + 10 * max_dets + seed)
    det_slots = max_dets + extra
    cams = cams or [CAMS[v % len(CAMS)] for v in range(V)]                      # camera g of the table
    views = rng.permutation(V).astype(np.int32) if permute else None            # view v is camera views[v]
    cam_of = [cams[int(views[v])] if permute else cams[v] for v in range(V)]
    if counts == 'full':
        n_raw = np.full(V, max_dets, dtype=np.int32)
    else:
        n_raw = np.array([(0, max_dets, max_dets + 3, -2, max(1, max_dets // 2), 1)[v % 6] for v in range(V)], dtype=np.int32)
    n_eff = np.clip(n_raw, 0, max_dets)
    host = np.empty((V, det_slots, J, 3))
    host.view(np.uint64)[:] = np.uint64(0x7FF8DEADBEEF0000) + np.arange(host.size, dtype=np.uint64).reshape(host.shape)      # distinct NaNs nobody computes
    want, ok = host.copy(), np.ones((V, det_slots, J), dtype=bool)
    ideal_err_mask, ideal = np.zeros((V, det_slots, J), dtype=bool), np.zeros((V, det_slots, J, 2))
    for v in range(V):
        raw, idl = raw_points(cam_of[v], fill, max_dets * J, seed + v)
        raw = raw.reshape(max_dets, J, 2)
        # every slot below max_dets gets a real row: a kernel that ignores a count would move it
        host[v, :max_dets, :, 0], host[v, :max_dets, :, 1] = raw[..., 1], raw[..., 0]
        host[v, :max_dets, :, 2] = SCORE0 + rng.uniform(0, 0.5, (max_dets, J))
        if idl is not None:
            ideal[v, :max_dets] = idl.reshape(max_dets, J, 2)
            ideal_err_mask[v, :n_eff[v]] = True
    for (v, s, j), (x, y) in (plant or {}).items():
        host[v, s, j, 0], host[v, s, j, 1] = y, x
        ideal_err_mask[v, s, j] = False
    want[:] = host
    for v in range(V):
        k = int(n_eff[v])
        if k == 0:
            continue
        raw = host[v, :k, :, 1::-1]                                             # (x, y)
        w, o = clear_verdicts(cam_of[v], raw)
        want[v, :k, :, 0], want[v, :k, :, 1] = w[..., 1], w[..., 0]
        ok[v, :k] = o
    det, front, back = banded((V, det_slots, J, 3), dev)
    det.copy_(torch.from_numpy(host))
    table = torch.from_numpy(np.stack([cam_row(c) for c in cams])).to(dev)
    t_n = torch.from_numpy(n_raw).to(dev)
    t_views = torch.from_numpy(views).to(dev) if permute else None
    info = torch.full((2,), -7, dtype=torch.int32, device=dev)
    rc = launch(det, t_n, t_views, table, info, V, max_dets, det_slots)
    torch.cuda.synchronize()
    assert rc == 0
    got = det.cpu().numpy()
    sent = G.as_i16(G.SENTINEL)
    assert bool((front == sent).all()) and bool((back == sent).all()), 'a sentinel band was written'
    return dict(got=got, host=host, want=want, ok=ok, info=info.cpu().numpy(), n_eff=n_eff, cam_of=cam_of, ideal=ideal,
                ideal_mask=ideal_err_mask, max_dets=max_dets)


def check(r):
    got, host, want, ok, n_eff = r['got'], r['host'], r['want'], r['ok'], r['n_eff']
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert np.array_equal(bits(got[..., 2]), bits(host[..., 2])), 'the score column was touched'
    for v in range(len(n_eff)):
        k = int(n_eff[v])
        assert np.array_equal(bits(got[v, k:]), bits(host[v, k:])), 'view %d: a row at or beyond the count was touched' % v
        if r['cam_of'][v] == 'pinhole':
            assert np.array_equal(bits(got[v]), bits(host[v])), 'view %d: a pin-hole camera\'s rows were touched' % v
    assert np.array_equal(bits(got[~ok]), bits(host[~ok])), 'a point the model cannot invert was moved'
    with np.errstate(invalid='ignore'):                          # (planted NaNs: masked out below)
        err = np.abs(got[..., :2] - want[..., :2])[ok & np.isfinite(want[..., 0])]
    worst = float(err.max()) if err.size else 0.0
    m = r['ideal_mask'] & ok
    ierr = np.abs(got[..., 1::-1][m] - r['ideal'][m])
    iworst = float(ierr.max()) if ierr.size else 0.0
    print('largest distance from the restatement %.3g px, from the ideal points %.3g px; %d kept of %d'
          % (worst, iworst, int((~ok).sum()), int(r['info'][1])))
    assert worst <= L.TOL_PX and iworst <= L.TOL_PX
    assert int(r['info'][0]) == int((~ok).sum()) and int(r['info'][1]) == int(n_eff.sum()) * J
    return worst


@pytest.mark.parametrize('fill', ['grid', 'corners', 'principal'])
@pytest.mark.parametrize('name', L.ORDER)
def test_one_view_one_slot(name, fill):
    for extra in (0, 1):
        r = run_case(1, 1, extra, False, 'full', fill, cams=[name])
        check(r)
        assert int(r['info'][1]) == J
        if fill == 'grid':
            assert np.abs(r['got'][0, 0, :, :2] - r['host'][0, 0, :, :2]).max() > 0.01          # the points did move


@pytest.mark.parametrize('V,max_dets', [(5, 8), (31, 16)])
@pytest.mark.parametrize('extra', [0, 1])
@pytest.mark.parametrize('permute', [False, True])
@pytest.mark.parametrize('counts', ['full', 'mixed'])
def test_rig_shapes(V, max_dets, extra, permute, counts):
    for fill in ('grid', 'corners', 'principal'):
        r = run_case(V, max_dets, extra, permute, counts, fill)
        check(r)
        assert set(r['cam_of']) == set(CAMS)                                      # the four sets and a pin-hole in one launch
        if fill == 'corners' and counts == 'full':
            assert int(r['info'][0]) > 0                                          # the wide barrel's frame corners lie beyond its fold


def test_planted_points_keep_their_rows_and_are_counted():
    s = L.SETS['barrel']
    fold = (s['k'][2] + 1.7 * s['k'][0], s['k'][3])                               # determinant <= 0 at the start of the iteration
    assert L.det2(L.jacobian(s['dist'], L.to_norm(s['k'], np.array([fold]))))[0] <= 0
    plant = {(2, 0, 0): fold, (2, 3, 16): fold, (0, 1, 5): (np.nan, 100.0), (0, 2, 6): (100.0, np.nan), (1, 0, 9): (np.inf, 50.0),
             (3, 7, 11): (-np.inf, np.nan), (4, 2, 2): (np.nan, np.nan)}         # view 2 is the wide barrel, view 4 the pin-hole
    r = run_case(5, 8, 1, False, 'full', 'grid', plant=plant)
    check(r)
    assert r['cam_of'][2] == 'barrel' and r['cam_of'][4] == 'pinhole'
    assert int(r['info'][0]) == 6 and int(r['info'][1]) == 5 * 8 * J               # (the pin-hole camera's NaN is copied, not counted)
    for (v, sl, j) in plant:
        assert np.array_equal(r['got'][v, sl, j].view(np.uint64), r['host'][v, sl, j].view(np.uint64))


def test_a_second_launch_starts_its_count_again():
    dev = torch.device('cuda:0')
    det = torch.zeros((1, 2, J, 3), dtype=torch.float64, device=dev)
    det[0, 0, 0, 0] = float('nan')
    n = torch.tensor([2], dtype=torch.int32, device=dev)
    table = torch.from_numpy(cam_row('hd')[None]).to(dev)
    info = torch.full((2,), 99, dtype=torch.int32, device=dev)
    for _ in range(2):
        assert launch(det, n, None, table, info, 1, 2, 2) == 0
        torch.cuda.synchronize()
        assert info.tolist() == [1, 2 * J]


def test_argument_errors_return_before_any_launch():
    from pam import _lib
    dev = torch.device('cuda:0')
    det, front, back = banded((2, 3, J, 3), dev)
    before = det.clone()
    n = torch.tensor([2, 2], dtype=torch.int32, device=dev)
    table = torch.from_numpy(np.stack([cam_row('hd'), cam_row('vga')])).to(dev)
    info = torch.full((2,), -7, dtype=torch.int32, device=dev)
    assert _lib.load().pam_undistort_keypoints(None, 1, 1, 0, None, None, None, None, None) != 0
    bad = [dict(det=None), dict(n_det=None), dict(lens=None), dict(info=None), dict(n_views=0), dict(n_views=-1), dict(max_dets=0),
           dict(max_dets=33), dict(max_dets=3, det_slots=2), dict(det_slots=1)]
    codes = []
    for b in bad:
        a = dict(det=det, n_det=n, views=None, lens=table, info=info, n_views=2, max_dets=2, det_slots=3)
        a.update(b)
        codes.append(launch(**a))
    torch.cuda.synchronize()
    assert len(set(codes)) == 1 and codes[0] != 0, codes
    # PAM_E_ARG is the code the library gives every argument error (pam_pose_nms with no buffers)
    assert codes[0] == _lib.load().pam_pose_nms(None, 0, 0, 0, None, None, 0, None, None, None, None, 0, 0, None, None, 0.0, 0.0, None, None, None)
    assert info.tolist() == [-7, -7] and torch.equal(det.view(torch.int64), before.view(torch.int64)), 'an argument error reached the device'


def test_the_wrapper_takes_the_tensors():
    from pam import _lib
    dev = torch.device('cuda:0')
    s = L.SETS['hd']
    ideal = L.grid('hd')[:2 * J].reshape(2, J, 2)
    raw = L.distort_px(s['k'], s['dist'], ideal)
    det = torch.zeros((1, 3, J, 3), dtype=torch.float64, device=dev)
    det[0, :2, :, 0], det[0, :2, :, 1] = torch.from_numpy(raw[..., 1]).to(dev), torch.from_numpy(raw[..., 0]).to(dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.undistort_keypoints(torch.cuda.current_stream().cuda_stream, det, torch.tensor([2], dtype=torch.int32, device=dev),
                             torch.from_numpy(L.lens_row('hd')[None]).to(dev), info, max_dets=2)
    torch.cuda.synchronize()
    got = det.cpu().numpy()
    assert np.abs(got[0, :2, :, 1::-1] - ideal).max() <= L.TOL_PX and info.tolist() == [0, 2 * J] and not got[0, 2].any()
    with pytest.raises(ValueError):
        _lib.undistort_keypoints(0, torch.zeros((1, 33, J, 3), dtype=torch.float64, device=dev), info, info, info)
