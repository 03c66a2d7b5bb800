"""k_frame in every launch form it has, at the ends of pam_create's capacity range, against the CPU oracle.

launch_frame picks one of these forms per handle (pam_frame_plan reports which one):
  A  256 threads, hot scratch + integer state in LDS             (<= 8 views, small capacities)
  B  256 threads, hot scratch + integer state in global memory   (<= 8 views, hot data above 128 KB)
  C  3 launches (1024 / 256 x 256 / 1024), LDS                   (> 8 views, one scene, small capacities)
  D  3 launches, global                                           (> 8 views, one scene, large capacities)
  E  one 1024-thread launch for n_scenes > 1, LDS
  F  one 1024-thread launch for n_scenes > 1, global
Each case asserts the plan it is named after, so a case cannot silently test another form."""
import numpy as np
import pytest

import tracker_matrix as M
from oracle import cpu_ref as O
from pam import synth

pytestmark = pytest.mark.gpu

PLANS = M.PLANS


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib


# form, views, persons, max_dets, max_tracks, frames.  Persons = max_dets wherever it fits, so that some view carries max_dets
# detections; B is the top of the capacity range (32 detections per view, LSAP at N = 64, more than 32 tracks over the sequence);
# the 32-view rigs set bit 31 of the per-joint view masks; 12 views is a rig between the 8- and 31-view ones.
SINGLE = [
    ('A', 5, 8, 8, 16, 80),
    ('B', 5, 32, 32, 64, 60),
    ('C', 12, 16, 16, 32, 60),
    ('C', 31, 8, 8, 16, 60),
    ('C', 32, 8, 8, 16, 60),
    ('D', 31, 16, 16, 32, 60),
    ('D', 32, 16, 16, 32, 60),
]


@pytest.mark.parametrize('form,C,P,max_dets,max_tracks,n_frames', SINGLE,
                         ids=['%s-c%d-p%d-d%d-t%d' % c[:5] for c in SINGLE])
def test_single_scene_form_vs_oracle(monkeypatch, form, C, P, max_dets, max_tracks, n_frames):
    """Stress sequences through the facade with explicit capacities: ids, camera and detection ids, views per joint identical to the
    oracle's, 3D <= 1e-6 m, status 0, every frame; the case reaches the per-view detection count and track count it is meant to."""
    size = M.add_rig(monkeypatch, C, P)
    seq = synth.make_sequence(size, n_frames=n_frames, seed=100 + C + max_dets, **M.STRESS)
    run = M.FacadeVsOracle(seq, max_dets, max_tracks)
    assert run.handle.plan() == PLANS[form]
    for t, views in enumerate(seq['frames']):
        run.step(t, views)
    assert run.max_det == max_dets                       # some view is full
    assert run.max_tracks >= P                           # every person had a track at some point ...
    if form == 'B':
        assert run.max_tracks > 32                       # ... and more tracks than the next smaller capacity holds
    if C == 32:
        assert run.max_views == 32                       # a joint built from all 32 views: bit 31 of the view masks
    else:
        assert run.max_views >= min(C, 8)
    assert run.n_out > n_frames * P // 2


# One sequence gross enough that k_frame's DLT certainly leaves the inverse iteration for the Jacobi fall-back: 12 views (form C, tracks of
# more than 8 views fold their rows four ways), 40 px of keypoint noise, every second pose with an outlier joint.  Chosen on the CPU from the
# systems the oracle solves (O.dlt_solve wrapped), each against mpmath's 50-digit SVD: seed 6 has 8 278 solved joints, 77 of them with
# s4 / s3 > 0.3 -- eight steps shrink the iteration's error by no more than 0.3^14 ~ 5e-8, so the device took Jacobi for them (tests/
# test_gpu_dlt_paths.py pins that rule on the operator; the kept view sets are asserted identical here) -- and LAPACK's worst error against
# the truth is 3.9e-9 m over all of them, so the 1e-6 m bar of `step` is a fair one.
FALLBACK = dict(C=12, P=4, max_dets=8, max_tracks=32, n_frames=60, seed=6, noise_px=40.0, outlier_p=0.5)


def test_gross_noise_drives_the_frame_step_into_the_jacobi_fall_back(monkeypatch):
    f = FALLBACK
    size = M.add_rig(monkeypatch, f['C'], f['P'])
    seq = synth.make_sequence(size, n_frames=f['n_frames'], seed=f['seed'], noise_px=f['noise_px'], outlier_p=f['outlier_p'], **M.STRESS)
    rho, solve = [], O.dlt_solve

    def spy(A, mask, nviews, next_pose=None):
        for j in np.nonzero(np.asarray(nviews) >= 2)[0]:
            s = np.linalg.svd(A[j][np.asarray(mask[j]) == 1], compute_uv=False)
            rho.append(s[3] / s[2])
        return solve(A, mask, nviews, next_pose)
    monkeypatch.setattr(O, 'dlt_solve', spy)
    run = M.FacadeVsOracle(seq, f['max_dets'], f['max_tracks'])
    assert run.handle.plan() == PLANS['C']
    for t, views in enumerate(seq['frames']):
        run.step(t, views)
    rho = np.array(rho)
    assert len(rho) > 5000 and (rho > 0.3).sum() >= 50, (len(rho), (rho > 0.3).sum())
    assert run.max_views > 8 and run.n_out > f['n_frames'] * f['P'] // 2


BATCHED = [('E', 31, 8, 8, 16), ('F', 31, 16, 16, 32), ('E', 32, 8, 8, 16), ('F', 32, 16, 16, 32)]


@pytest.mark.parametrize('form,C,P,max_dets,max_tracks', BATCHED, ids=['%s-c%d-p%d-d%d-t%d' % c for c in BATCHED])
def test_batched_wide_rig_matches_single_scenes_and_oracle(lib, monkeypatch, form, C, P, max_dets, max_tracks):
    """Three scenes in one launch on a wide rig: each scene's record equals, frame by frame, what a single-scene handle of the same
    capacities gives (clock header words excluded); scene 0's single-scene handle is the facade's, checked against the oracle."""
    S, n_frames = 3, 60
    size = M.add_rig(monkeypatch, C, P)
    seqs = [synth.make_sequence(size, n_frames=n_frames, seed=200 + 10 * C + s, **M.STRESS) for s in range(S)]
    run = M.FacadeVsOracle(seqs[0], max_dets, max_tracks)
    cams = run.dev.cameras
    hb = M.handle_for(lib, size, cams, max_dets, max_tracks, n_scenes=S)
    assert hb.plan() == PLANS[form]
    singles = [M.handle_for(lib, size, cams, max_dets, max_tracks) for _ in range(1, S)]
    assert all(h.plan() == PLANS['C' if form == 'E' else 'D'] for h in singles)
    packed = [synth.pack_frames(q['frames'], max_dets) for q in seqs]
    for t in range(n_frames):
        nd = np.stack([p[0][t] for p in packed])
        dd = np.stack([p[1][t] for p in packed])
        oi, od = hb.frame(t, nd, dd)
        run.step(t, seqs[0]['frames'][t])
        M.assert_same_record(hb.layout, (oi[0], od[0]), run.record(), (t, 0))
        for s in range(1, S):
            si, sd = singles[s - 1].frame(t, nd[s:s + 1], dd[s:s + 1])
            M.assert_same_record(hb.layout, (oi[s], od[s]), (si[0], sd[0]), (t, s))
        assert all(oi[s][1] == 0 for s in range(S)), t
    assert run.max_det == max_dets and run.n_out > n_frames * P // 2
    for h in singles:
        h.close()
    hb.close()


HYP = [('A', 5, 16, 8, 16), ('D', 31, 32, 16, 32)]


@pytest.mark.parametrize('form,C,P,max_dets,max_tracks', HYP, ids=['%s-c%d-p%d-d%d-t%d' % c for c in HYP])
def test_hypothesis_overflow_is_reported(lib, monkeypatch, form, C, P, max_dets, max_tracks):
    """A birth frame in which every view sees max_dets of P = 2 max_dets persons, a different subset per view, on a handle with as few
    hypothesis slots as it takes (max_hyps = max_dets): the frame raises ST_HYP_OVERFLOW, and the sticky bits keep it afterwards."""
    size = M.add_rig(monkeypatch, C, P)
    seq = synth.make_sequence(size, n_frames=1, seed=7, outlier_p=0.0, occlusion_every=0, empty_view_every=0, shuffle=False)
    frame = [v[[(3 * c + k) % P for k in range(max_dets)]] for c, v in enumerate(seq['frames'][0])]
    h = M.handle_for(lib, size, O.make_cameras(seq['calib']), max_dets, max_tracks, max_hyps=max_dets)
    assert h.plan() == PLANS[form]
    nd, dd = synth.pack_frames([frame], max_dets)
    rec = M.run_dev(h, 0, nd[0], dd[0])
    assert rec['status'] & lib.ST_HYP_OVERFLOW, rec['status']
    assert rec['status_sticky'] & lib.ST_HYP_OVERFLOW
    assert rec['n_hyp'] <= max_dets
    rec = M.run_dev(h, 1, np.zeros_like(nd[0]), dd[0])           # nothing to spawn: clean frame, sticky bit stays
    assert not rec['status'] & lib.ST_HYP_OVERFLOW
    assert rec['status_sticky'] & lib.ST_HYP_OVERFLOW
    h.close()


CLAMP = [('A', 5, 8, 8, 16, 40), ('D', 31, 16, 16, 32, 40)]


@pytest.mark.parametrize('form,C,P,max_dets,max_tracks,n_frames', CLAMP, ids=['%s-c%d-p%d-d%d-t%d' % c[:5] for c in CLAMP])
def test_device_counts_out_of_range_are_clamped(lib, monkeypatch, form, C, P, max_dets, max_tracks, n_frames):
    """pam_frame_dev takes device-side detection counts unchecked.  A count above max_dets must act as max_dets, a negative one as
    no detections, and the frame must raise ST_NDET_CLAMPED: the record equals, word for word, that of the facade fed the input so
    truncated, and the facade's equals the oracle's."""
    size = M.add_rig(monkeypatch, C, P)
    seq = synth.make_sequence(size, n_frames=n_frames, seed=300 + C, **M.STRESS)
    run = M.FacadeVsOracle(seq, max_dets, max_tracks)
    h = M.handle_for(lib, size, run.dev.cameras, max_dets, max_tracks)
    assert h.plan() == run.handle.plan() == PLANS[form]
    nd, dd = synth.pack_frames(seq['frames'], max_dets)
    n_high = n_low = 0
    for t in range(n_frames):
        views = list(seq['frames'][t])
        counts = nd[t].copy()
        full = [v for v in range(C) if counts[v] == max_dets]
        if t % 5 == 2 and full:                              # a full view claims more rows than the buffer has
            counts[full[0]] = max_dets + 1 + (t % 3) * 1000
            n_high += 1
        elif t % 5 == 4 and counts[t % C] > 0:               # a negative count: the view is read as empty
            counts[t % C] = -1 - t
            views[t % C] = views[t % C][:0]
            n_low += 1
        run.step(t, views)
        rec = M.run_dev(h, t, counts, dd[t])
        bad = bool((counts < 0).any() or (counts > max_dets).any())
        assert rec['status'] == (lib.ST_NDET_CLAMPED if bad else 0), (t, counts)
        M.assert_same_record(h.layout, (h.out_i[0], h.out_d[0]), run.record(), t, skip_status=True)
    assert rec['status_sticky'] & lib.ST_NDET_CLAMPED
    assert n_high >= 4 and n_low >= 4
    h.close()
