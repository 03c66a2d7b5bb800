"""The lens step in front of the tracker, on the GPU, without a network: the S1 trace of tests/lens_ref.py (3 cameras, 20 frames, the
VGA-like coefficients on the rig's K; tests/test_lens_ref.py checks on the CPU that the oracle decides it alike on ideal and on
undistorted rows).

Pass 1 tracks the ideal rows.  Pass 2 tracks the distorted rows -- the ideal ones pushed through the forward model in float64 NumPy --
behind the device-side step: ids, matched detections, view sets and life-cycle fields equal pass 1's on every frame, 3D joints within
1e-9 m (the inputs differ by about 1e-12 px; at metres of depth over a 400 px focal length that is about 1e-14 m before conditioning).
Pass 3 tracks the distorted rows with the step off and must not reproduce pass 1.  Once through FramePipeline (write_local ->
undistort_local -> track_step), once through the façade's host-list path."""
import numpy as np
import pytest
import torch

import lens_ref as L
from pam import synth

pytestmark = pytest.mark.gpu

MD = 8
TOL_M = 1e-9
FIELDS = ('track_id', 'state', 'hits', 'age', 'time_since_update', 'emitted', 'order', 'V', 'nhist', 'last_time')
ARRAYS = ('matched_det', 'time2d', 'nviews')


@pytest.fixture(scope='module')
def trace():
    T = L.trace()
    T['cfg'] = dict(synth.MATCHER_CFG['CampusSeq1'])
    T['conf'] = T['cfg'].pop('CONF_THRESHOLD')
    return T


def _cameras(T):
    from pam.ivclabpose import Camera, fundamental_matrices
    c, m = T['seq']['calib'], T['seq']['meta']
    P32, K32, RT32 = c['P'].astype(np.float32), c['K'].astype(np.float32), c['RT'].astype(np.float32)
    Fm = fundamental_matrices(K32, RT32)
    return [Camera(j, P32[j], K32[j], RT32[j], Fm[j], w=m['w'], h=m['h']) for j in range(m['C'])]


def _same_decisions(a, b):
    if a['n_tracks'] != b['n_tracks']:
        return False
    for ta, tb in zip(a['tracks'], b['tracks']):
        if any(ta[k] != tb[k] for k in FIELDS) or any(not np.array_equal(ta[k], tb[k]) for k in ARRAYS):
            return False
    return True


def _max3d(a, b):
    return max([float(np.abs(ta['pose3d'] - tb['pose3d']).max()) for ta, tb in zip(a['tracks'], b['tracks'])] or [0.0])


def _emitted(recs):
    return sum(1 for r in recs for t in r['tracks'] if t['emitted'])


def test_frame_pipeline_undistort_local(trace):
    from pam.pipeline import FramePipeline
    T, m = trace, trace['seq']['meta']
    cams = _cameras(T)
    nd_all, ideal = synth.pack_frames(T['ideal'], MD)
    _, raw = synth.pack_frames(T['raw'], MD)
    assert np.abs(raw[..., :2] - ideal[..., :2]).max() > 10.0
    mk = lambda lens: FramePipeline(cams, T['cfg'], T['conf'], (m['h'], m['w']), max_dets=MD, hrnet=False, net=None, lens=lens)
    p1, p2, p3 = mk(None), mk(T['lens']), mk(None)
    assert p1.lens is None and p3.lens_info is None and tuple(p2.lens.shape) == (m['C'], 10)
    dev = p1.device
    r1, r2, r3, pts = [], [], [], 0
    for t in range(m['n_frames']):
        nd = torch.tensor(nd_all[t], dtype=torch.int32, device=dev)
        p1.write_local(torch.tensor(ideal[t], dtype=torch.float64, device=dev)); p1.track_step(t, nd); r1.append(p1.results())
        p2.write_local(torch.tensor(raw[t], dtype=torch.float64, device=dev)); p2.undistort_local(nd); p2.track_step(t, nd)
        r2.append(p2.results())
        assert p2.lens_info.tolist() == [0, 17 * int(nd_all[t].sum())]
        got = p2.det_local[:, :MD].cpu().numpy()
        live = np.arange(MD)[None, :] < nd_all[t][:, None]
        assert np.abs(got[live][..., :2] - ideal[t][live][..., :2]).max() <= L.TOL_PX                  # the rows the tracker read
        assert np.array_equal(got[..., 2], raw[t][..., 2]) and np.array_equal(got[~live], raw[t][~live])
        pts += int(nd_all[t].sum())
        p3.write_local(torch.tensor(raw[t], dtype=torch.float64, device=dev)); p3.undistort_local(nd); p3.track_step(t, nd)
        r3.append(p3.results(strict=False))
    assert pts > 100 and _emitted(r1) >= 20
    d2 = 0.0
    for t, (a, b) in enumerate(zip(r1, r2)):
        assert _same_decisions(a, b), 'frame %d' % t
        d2 = max(d2, _max3d(a, b))
    d3 = max(_max3d(a, c) for a, c in zip(r1, r3))                 # (track by track in list order, as far as both lists go)
    print('3D joints: %.3g m from the ideal run with the step, %.3g m without; emitted tracks %d / %d / %d; decisions without the step %s'
          % (d2, d3, _emitted(r1), _emitted(r2), _emitted(r3), 'equal' if all(_same_decisions(a, c) for a, c in zip(r1, r3)) else 'differ'))
    assert d2 <= TOL_M
    assert _emitted(r3) < _emitted(r1) or d3 >= 1000 * max(d2, 1e-12)


def test_pipeline_arguments():
    from pam.pipeline import FramePipeline
    T = L.trace()
    cfg = dict(synth.MATCHER_CFG['CampusSeq1']); conf = cfg.pop('CONF_THRESHOLD')
    m = T['seq']['meta']
    with pytest.raises(ValueError):
        FramePipeline(_cameras(T), cfg, conf, (m['h'], m['w']), max_dets=MD, hrnet=False, lens=T['lens'], shard='crops')
    with pytest.raises(ValueError):
        FramePipeline(_cameras(T), cfg, conf, (m['h'], m['w']), max_dets=MD, hrnet=False, lens=T['lens'][:2])
    zero = FramePipeline(_cameras(T), cfg, conf, (m['h'], m['w']), max_dets=MD, hrnet=False, lens=T['lens'] * np.r_[np.ones(5), np.zeros(5)])
    assert zero.lens is None


def _facade(T, dist):
    from pam.ivclabpose import ivclabpose
    m = T['seq']['meta']
    model = ivclabpose({'NAME': ''}, None, dict(T['cfg'], NAME='Iterative'), T['conf'], max_dets=MD, max_tracks=16)
    calib = dict(T['seq']['calib'])
    if dist is not None:
        calib['distCoef'] = dist
    cams = model.GetCameraParameters(calib, m['w'], m['h'])
    return model, cams


def _run_facade(model, frames):
    out = []
    for t, views in enumerate(frames):
        pbl, dr = synth.to_dump_results(views)                     # plain lists: the host-list path
        out.append(model.PersonTrack_Project3DPose(t, pbl, dr, 'SVD'))
    return out


def _same_tuple(a, b):
    return ([list(map(int, c)) for c in a[0]] == [list(map(int, c)) for c in b[0]] and list(a[5]) == list(b[5]) and a[4] == b[4]
            and a[2] == b[2])


def test_facade_host_list_path(trace):
    T = trace
    ideal_model, cams0 = _facade(T, None)
    lens_model, cams = _facade(T, T['dist'])
    off_model, _ = _facade(T, None)
    assert all(c.lens is None and c.distCoef is None for c in cams0) and ideal_model.lens is None
    assert all(np.array_equal(c.lens, row) for c, row in zip(cams, T['lens'])) and np.array_equal(lens_model.lens, T['lens'])
    a, b, c = _run_facade(ideal_model, T['ideal']), _run_facade(lens_model, T['raw']), _run_facade(off_model, T['raw'])
    d2, n_pts = 0.0, 0
    for t, (x, y) in enumerate(zip(a, b)):
        assert _same_tuple(x, y), 'frame %d' % t
        if len(x[5]):
            d2 = max(d2, float(np.abs(np.asarray(x[3]) - np.asarray(y[3])).max()))
        # pts: the RAW rows of the frame, (y, x, score), bit for bit -- what an overlay draws on
        raw_rows = [v[:, :, [1, 0, 2]] for v in T['raw'][t]]
        for cams_i, pts_i in zip(y[0], y[1]):
            for cid, row in zip(cams_i, pts_i):
                assert any(np.array_equal(row, r) for r in raw_rows[int(cid)]), 'frame %d: pts is not a raw row' % t
                n_pts += 1
    assert n_pts > 50 and sum(len(x[5]) for x in a) >= 20
    d3 = 0.0                                                       # (person by person, for the ids both runs emitted in a frame)
    for x, z in zip(a, c):
        for i, pid in enumerate(x[5]):
            for k in np.flatnonzero(np.asarray(z[5]) == pid):
                d3 = max(d3, float(np.abs(np.asarray(x[3][i]) - np.asarray(z[3][k])).max()))
    print('façade: 3D joints %.3g m from the ideal run with distCoef, %.3g m without; emitted %d / %d / %d'
          % (d2, d3, sum(len(x[5]) for x in a), sum(len(y[5]) for y in b), sum(len(z[5]) for z in c)))
    assert d2 <= TOL_M
    assert sum(len(z[5]) for z in c) < sum(len(x[5]) for x in a) or d3 >= 1000 * max(d2, 1e-12)
    # the tracker's boxes follow: the handle has the table, a rig without distCoef has none (pam_set_lens through set_cameras)
    h, w = T['seq']['meta']['h'], T['seq']['meta']['w']
    n = T['seq']['meta']['n_frames']
    with_lens = lens_model.tracker.predict_boxes(n, (h, w))
    without = ideal_model.tracker.predict_boxes(n, (h, w))
    assert sum(len(v) for v in with_lens) > 0 and sum(len(v) for v in without) > 0
    assert max(float(np.abs(p[:, :4] - q[:, :4]).max()) for p, q in zip(with_lens, without) if len(p) and len(p) == len(q)) > 0.5
