"""Shared pieces of test_gpu_tracker_matrix.py and of the scenario tests (test_tracker_scenarios_ref.py, test_gpu_tracker_scenarios.py):
synthetic rigs of any size, the frame step through the drop-in facade checked against the CPU oracle every frame, record comparisons
between handles, the score / gross-noise scenarios and the spies that witness them on the oracle.  A plain module (not a conftest.py)."""
import warnings

import numpy as np

from oracle import cpu_ref as O
from oracle.cpu_ref import J
from pam import synth

# what Handle.plan() reports for each launch form (the forms: test_gpu_tracker_matrix.py)
PLANS = {'A': dict(block=256, launches=1, hot_in_lds=1), 'B': dict(block=256, launches=1, hot_in_lds=0),
         'C': dict(block=1024, launches=3, hot_in_lds=1), 'D': dict(block=1024, launches=3, hot_in_lds=0),
         'E': dict(block=1024, launches=1, hot_in_lds=1), 'F': dict(block=1024, launches=1, hot_in_lds=0)}

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

    def __init__(self, seq, max_dets, max_tracks, F=None):
        """F: fundamental matrices to hand to the facade (and through it to the oracle) in place of its own float32 set-up."""
        from pam.ivclabpose import ivclabpose
        size = seq['meta']['size']
        cfg, conf = matcher(size)
        self.dev = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=max_dets, max_tracks=max_tracks)
        cams = self.dev.GetCameraParameters(seq['calib'], seq['meta']['w'], seq['meta']['h'], **({} if F is None else {'F': F}))
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


# ---- score and gross-noise scenarios (test_tracker_scenarios_ref.py on the CPU, test_gpu_tracker_scenarios.py on the device) ----------
GROSS = dict(noise_px=40.0, outlier_p=0.5)
SCENARIO_FRAMES = 40


# a score mix with more confident detections than synth.SCORE_MIX: under gross noise on a 5-view rig the default mix leaves too few
# tracks alive for the update path's branches
MILD_MIX = dict(high=0.60, low=0.12, mixed=0.08, negative=0.06, half=0.07, two_fifths=0.07)


def rounded_F(calib):
    """The fundamental matrices of ivclabpose.py:166-177 formed in float64 from the float32 K and RT and rounded to float32 once.  The
    reference (and the facade, and O.fundamental_matrices) form them in float32 products, which round differently from one CPU's BLAS
    kernels to the next (golden_io.camera_variants); under gross noise a last-bit change of F flips decisions and sends the tracker
    another way.  The scenarios fix F to these values, so that the sequence the witness test examined is the one every machine runs."""
    K = np.asarray(calib['K']).astype(np.float32).astype(np.float64)
    RT = np.asarray(calib['RT']).astype(np.float32).astype(np.float64)
    C = len(K)
    F = np.zeros((C, C, 3, 3))
    for x in range(C):
        Rx, Tx, Kxi = RT[x][:, :3], RT[x][:, 3], np.linalg.inv(K[x])
        for y in range(C):
            if x == y:
                F[x, y] = 1e-12                                                       # :176-177, never read
                continue
            Ry, Ty = RT[y][:, :3], RT[y][:, 3]
            v = K[y] @ Ry @ Rx.T @ (Tx - Rx @ Ry.T @ Ty)
            skew = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
            F[x, y] = Kxi.T @ (Rx @ Ry.T) @ K[y].T @ skew
    return F.astype(np.float32)


def scenario(monkeypatch, rig, seed, noise=False, rescore=None, P=4, mix=None, cap=None):
    """A 40-frame STRESS sequence on ``rig`` ('S1' / 'S2' / 'S3' or a view count for a synthetic Panoptic rig of P persons), with gross
    keypoint noise (noise=True) and / or its scores redrawn by synth.rescore_frames (rescore = its seed, mix = its class mix).
    seq['F'] = rounded_F of its rig: hand it to FacadeVsOracle and handle_for's cameras."""
    size = rig if isinstance(rig, str) else add_rig(monkeypatch, rig, P)
    seq = synth.make_sequence(size, n_frames=SCENARIO_FRAMES, seed=seed, **dict(STRESS, **(GROSS if noise else {})))
    if rescore is not None:
        seq['frames'] = synth.rescore_frames(seq['frames'], rescore, mix)
    seq['F'] = rounded_F(seq['calib'])
    return seq


def score_class(s):
    """The class of synth.draw_scores that a detection's 17 scores belong to, read from the scores themselves."""
    neg = s < 0
    if neg.all():
        return 'negative'
    if neg.any():
        return 'two_fifths' if (neg.sum() == 12 and np.all(s[neg] == -0.25)) else 'mixed'
    if np.all(s == 0.5):
        return 'half'
    return 'low' if s.max() <= 30 / 64.0 else 'high'


def _rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


class Witness(object):
    """Spies round the oracle's decision points: which branches a sequence drives the ORACLE through, and how far every decision it
    takes lies from its threshold (a comparison of two implementations says nothing about a branch neither took, and is a lottery
    where a decision hangs on the last bits).  Use as a context manager round the oracle run; ``conf`` = its CONF_THRESHOLD."""

    def __init__(self, conf):
        self.conf = conf
        self.dropped = dict(low=0, negative=0, equal=0)    # unmatched detections the confidence filter drops, by class
        self.mixed_split = 0           # mixed detections the filter decides with the plain mean on the other side of the threshold
        self.kept = 0
        self.veto_suppressed = 0       # member cost p > 1 with believe in (0.4, 0.5]: no veto
        self.veto = 0
        self.rejected_updates = self.copied_updates = self.updates = 0
        self.init_calls = self.init_conflicts = self.rejected_hyps = 0
        self.cnt10 = self.cnt11 = self.pairs = 0
        self.margin_cost = self.margin_c = self.margin_aff = self.margin_cmp = np.inf
        self.max_hyps = 0              # most hypotheses formed in one frame
        self.max_tracks = 0            # most tracks held at the end of a frame step, the dying ones included
        self._in_cost = False

    def __enter__(self):
        self._saved = dict(believe=O.believe, hyp_cost=O.hyp_cost, association_affinity=O.association_affinity,
                           greedy_filter=O.greedy_filter)
        self._saved_update, self._saved_init = O.Tracker._triangulate_update, O.Tracker._init_tracks
        init = O.Tracker._init_tracks
        believe, hyp_cost, assoc, greedy, update = (O.believe, O.hyp_cost, O.association_affinity, O.greedy_filter,
                                                    O.Tracker._triangulate_update)
        w = self

        def spy_believe(pose):
            with np.errstate(invalid='ignore'), warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)       # the mean of no score at all is NaN, as in the reference
                b = believe(pose)
            if not w._in_cost:                                        # the confidence filter on an unmatched detection
                s = np.asarray(pose)[:, 2]
                cls = score_class(s)
                if b > w.conf:
                    w.kept += 1
                    if cls == 'mixed' and not s.mean() > w.conf:
                        w.mixed_split += 1
                elif cls in ('low', 'negative'):
                    w.dropped[cls] += 1
                elif b == w.conf:
                    w.dropped['equal'] += 1
            return b

        def spy_cost(member_cams, member_poses, o_cam, o_pose, threshold):
            w._in_cost = True
            try:
                out = hyp_cost(member_cams, member_poses, o_cam, o_pose, threshold)
                bel = O.believe(o_pose)
                for cam, person in zip(member_cams, member_poses):
                    p = hyp_cost([cam], [person], o_cam, o_pose, threshold)[0]        # 0 + p, then p / 1: the member's own cost
                    w.margin_cost = min(w.margin_cost, abs(p - 1))
                    if p > 1:
                        if bel > 0.5:
                            w.veto += 1
                        elif 0.4 < bel <= 0.5:
                            w.veto_suppressed += 1
            finally:
                w._in_cost = False
            return out

        def spy_assoc(reproj, dets, dt, alpha2d, lambda_a):
            diff = reproj[:, None, :, :] - dets[None, :, :, :2]
            c = 1 - np.sqrt(diff[..., 0] ** 2 + diff[..., 1] ** 2) / (alpha2d * np.asarray(dt))[:, None, None]
            cnt = (c > 0).sum(axis=2)
            w.cnt10 += int((cnt == 10).sum())
            w.cnt11 += int((cnt == 11).sum())
            w.pairs += cnt.size
            w.margin_c = min(w.margin_c, float(np.abs(c).min()))
            return assoc(reproj, dets, dt, alpha2d, lambda_a)

        def spy_greedy(cams, aff, mode, pose_j=None, next_pose_j=None):
            keep, mask = greedy(cams, aff, mode, pose_j, next_pose_j)
            V = aff.shape[0]
            iu = np.triu_indices(V, 1)
            if len(iu[0]):
                w.margin_aff = min(w.margin_aff, float(np.abs(np.asarray(aff, dtype=np.float64)[iu]).min()))
            # the pairs the filter compares, walked as O.greedy_filter walks them
            alive = np.ones(V, dtype=bool)
            rows, cols = np.where(np.triu(aff) < 0)
            for r, c in zip(rows, cols):
                if not (alive[r] and alive[c]):
                    continue
                if mode == 'update':
                    a, b = (O.ray_point_distance(cams[k], pose_j[k], next_pose_j) for k in (r, c))
                    drop = r if a > b else c
                else:
                    a, b = float(np.sum(aff[r])), float(np.sum(aff[c]))
                    drop = c if a > b else r
                if a != b:
                    w.margin_cmp = min(w.margin_cmp, _rel_gap(a, b))
                alive[drop] = False
            assert np.array_equal(np.nonzero(alive)[0], keep)
            if mode == 'init':
                w.init_calls += 1
                w.init_conflicts += int(len(rows) > 0)
                w.rejected_hyps += int(len(keep) < 2)
            return keep, mask

        def spy_update(self_, tr, time, cams, Ts, pose_mat):
            pose3d, nviews, ok = update(self_, tr, time, cams, Ts, pose_mat)
            copied = int((np.asarray(nviews) < 2).sum())
            w.updates += 1
            if not ok:
                assert copied > J / 3.0
                w.rejected_updates += 1
            elif 1 <= copied <= 5:
                w.copied_updates += 1
            return pose3d, nviews, ok

        def spy_init(self_, time):
            init(self_, time)
            w.max_hyps = max(w.max_hyps, self_.n_hyp)
            w.max_tracks = max(w.max_tracks, len(self_.tracks))

        O.believe, O.hyp_cost, O.association_affinity, O.greedy_filter = spy_believe, spy_cost, spy_assoc, spy_greedy
        O.Tracker._triangulate_update, O.Tracker._init_tracks = spy_update, spy_init
        return self

    def __exit__(self, *exc):
        for k, v in self._saved.items():
            setattr(O, k, v)
        O.Tracker._triangulate_update, O.Tracker._init_tracks = self._saved_update, self._saved_init
        return False

    def counts(self):
        return dict(dropped=dict(self.dropped), mixed_split=self.mixed_split, kept=self.kept, veto=self.veto,
                    veto_suppressed=self.veto_suppressed, updates=self.updates, rejected_updates=self.rejected_updates,
                    copied_updates=self.copied_updates, init_calls=self.init_calls, init_conflicts=self.init_conflicts,
                    rejected_hyps=self.rejected_hyps, max_hyps=self.max_hyps, max_tracks=self.max_tracks, pairs=self.pairs, cnt10=self.cnt10, cnt11=self.cnt11,
                    margins=dict(cost=self.margin_cost, c=self.margin_c, aff=self.margin_aff, cmp=self.margin_cmp))


def run_oracle(seq, conf=None, witness=False):
    """The oracle alone over a sequence -> (per-frame (ids, camera ids), Witness or None).  conf overrides the rig's CONF_THRESHOLD."""
    cfg, c0 = matcher(seq['meta']['size'])
    conf = c0 if conf is None else conf
    ref = O.OracleIvclabpose(cfg, conf)
    ref.GetCameraParameters(seq['calib'], F=seq['F'])
    w = Witness(conf) if witness else None
    out = []

    def go():
        for t, views in enumerate(seq['frames']):
            pbl, dr = synth.to_dump_results(views)
            b = ref.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
            out.append((list(map(int, b[5])), [list(map(int, c)) for c in b[0]]))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        if w is None:
            go()
        else:
            with w:
                go()
    return out, w


def lapack_worst_error(seq):
    """Worst |X_LAPACK - X_true| (metres) over every system the oracle's DLT solves on ``seq``, X_true from the 50-digit SVD of
    tests/dlt_ref.py, and the number of systems.  Minutes of mpmath: run by hand when a gross-noise scenario is chosen (the figures
    stand beside the cases of test_tracker_scenarios_ref.py); the 1e-6 m bar of FacadeVsOracle.step is fair while this is below 1e-7."""
    import dlt_ref
    solve, worst, n = O.dlt_solve, [0.0], [0]

    def spy(A, mask, nviews, next_pose=None):
        out = solve(A, mask, nviews, next_pose)
        for j in np.nonzero(np.asarray(nviews) >= 2)[0]:
            X, _ = dlt_ref.truth(A[j][np.asarray(mask[j]) == 1])
            worst[0] = max(worst[0], max(abs(float(X[c] - float(out[j, c]))) for c in range(3)))
            n[0] += 1
        return out
    O.dlt_solve = spy
    try:
        run_oracle(seq)
    finally:
        O.dlt_solve = solve
    return worst[0], n[0]


# The scenarios: name -> scenario()'s arguments; cap = the (max_dets, max_tracks) of the handles that run it.  Seeds were chosen on the
# CPU, from the oracle alone, so that every count and margin test_tracker_scenarios_ref.py asserts holds -- among them that no frame
# needs more hypothesis or track slots than cap gives (pam_create: 4 max_dets hypotheses); the counts stand beside its cases.  (The
# golden traces trace_S1s / S2s / S3s hold the sequences S1 703 / 1703, S2 409 / 1409 and S3 406 / 1406, run through the reference by
# tools/make_goldens.py --rescored.)
SCORE_SCENARIOS = {
    'A-S1': dict(rig='S1', seed=714, rescore=1714, cap=(8, 16)),         # 3 views, CONF_THRESHOLD 0.4
    'A-S2': dict(rig='S2', seed=410, rescore=1410, cap=(8, 16)),         # 5 views, 0.5
    'C-12': dict(rig=12, seed=403, rescore=1403, cap=(16, 32)),          # Panoptic thresholds (0.4) from here on, 4 persons
    'D-31': dict(rig=31, seed=405, rescore=1405, cap=(16, 32)),          # also scene 0 of form F
    'E-12': dict(rig=12, seed=404, rescore=1404, cap=(16, 32)),          # scene 0 of form E
}
NOISE_SCENARIOS = {
    'AB-5': dict(rig=5, seed=411, noise=True, cap=(8, 16)),              # forms A (8 / 16) and B (32 / 64)
    'E-12': dict(rig=12, seed=413, noise=True, cap=(16, 32)),            # scene 1 of form E
    'DF-31': dict(rig=31, seed=447, noise=True, P=3, cap=(16, 32)),      # form D and scene 1 of form F; three persons: four leave
                                                                         # more than 32 tracks alive, and the oracle above 20 s
}
BOTH_SCENARIOS = {
    'A-5': dict(rig=5, seed=426, noise=True, rescore=1426, mix=MILD_MIX, cap=(8, 16)),
    'E-12': dict(rig=12, seed=431, noise=True, rescore=1431, cap=(16, 32)),    # scene 2 of form E
    'F-31': dict(rig=31, seed=433, noise=True, rescore=1433, P=3, cap=(16, 32)),   # scene 2 of form F
}
