"""k_frame's score-dependent and noise-driven branches in every launch form, against the CPU oracle and the reference's own traces.

Every comparison of the other tracker tests feeds k_frame keypoint scores from uniform(0.7, 0.95) and, but for one case of form C, 1.5 px
of noise: the confidence filter on unmatched detections, the exclusion of negative scores from a detection's confidence (and the NaN of a
detection without any), the veto that a confidence of at most 0.5 suppresses, negative weights in the hypothesis cost, rejected updates,
joints copied from the prediction, conflicting init filters and rejected hypotheses are not reached there.  Here they are: sequences whose
scores synth.rescore_frames redrew, sequences with 40 px of noise and an outlier in every second pose, and both at once, in forms A to F
(the forms: test_gpu_tracker_matrix.py).  tests/test_tracker_scenarios_ref.py shows on the CPU that each sequence drives the oracle
through these branches, that no decision lies within 1e-9 of its threshold, and that LAPACK itself stays below 1e-7 m on the noisy ones;
the seeds and counts stand there.  Each case asserts the plan it is named after."""
import numpy as np
import pytest

import golden_io as G
import tracker_matrix as M
from trace_driver import run_trace
from pam import synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore:Mean of empty slice', 'ignore:invalid value encountered')]


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib


def _run(seq, cap, form):
    run = M.FacadeVsOracle(seq, *cap, F=seq['F'])
    assert run.handle.plan() == M.PLANS[form]
    for t, views in enumerate(seq['frames']):
        run.step(t, views)
    return run


@pytest.mark.parametrize('size', G.RESCORED)
def test_rescored_golden_traces_through_the_facade(size):
    """The reference's own output on the re-scored traces (form A): ids, view sets, joints_views and camera ids bit-exact, 3D <= 1e-6 m,
    the tracker state identical after every frame, status 0."""
    from pam.ivclabpose import ivclabpose

    def factory(cfg, conf):
        return ivclabpose(person_detector={'NAME': ''}, pose_detector=None, person_matcher=dict(cfg, NAME='Iterative'),
                          conf_threshold=conf, max_dets=8, max_tracks=16)
    nf = 0
    for t, tr, model in run_trace(size, factory, atol3d=1e-6):
        k = 'f%d.st.' % t
        trs = model.tracker.tracks
        assert model.tracker.handle.plan() == M.PLANS['A']
        assert model.tracker.last['status'] == 0
        assert [x.track_id for x in trs] == tr[k + 'ids'].tolist(), (size, t)
        assert [x.state for x in trs] == tr[k + 'state'].tolist()
        assert [x.hits for x in trs] == tr[k + 'hits'].tolist()
        assert [x.age for x in trs] == tr[k + 'age'].tolist()
        assert [x.time_since_update for x in trs] == tr[k + 'tsu'].tolist()
        assert [x.nhist for x in trs] == tr[k + 'nhist'].tolist()
        assert [x.last_time for x in trs] == tr[k + 'last_time'].tolist()
        for i, x in enumerate(trs):
            assert x.order == [int(c) for c in tr[k + 'p2d_order'][i] if c >= 0]
            np.testing.assert_allclose(x.pose3d, tr[k + 'last_pose'][i], rtol=0, atol=1e-6)
            np.testing.assert_allclose(x.velocity_3d, tr[k + 'velocity'][i], rtol=0, atol=1e-6)
        nf += 1
    assert nf == 40


SCORES = [('A', 'A-S1'), ('A', 'A-S2'), ('C', 'C-12'), ('D', 'D-31')]


@pytest.mark.parametrize('form,name', SCORES, ids=['%s-%s' % c for c in SCORES])
def test_rescored_sequence_vs_oracle(monkeypatch, form, name):
    """Fresh re-scored stress sequences: the confidence filter at 0.4 and at 0.5, on it, under it and without a score to average."""
    sc = M.SCORE_SCENARIOS[name]
    run = _run(M.scenario(monkeypatch, **sc), sc['cap'], form)
    assert run.n_out >= 40


NOISE = [('A', 'AB-5', (8, 16)), ('B', 'AB-5', (32, 64)), ('D', 'DF-31', (16, 32))]


@pytest.mark.parametrize('form,name,cap', NOISE, ids=['%s-%s-d%d-t%d' % (c[0], c[1], c[2][0], c[2][1]) for c in NOISE])
def test_gross_noise_sequence_vs_oracle(monkeypatch, form, name, cap):
    """40 px of noise and an outlier joint in every second pose outside form C: rejected updates, joints copied from the prediction,
    conflicting init filters, rejected hypotheses, association counts on either side of the gate."""
    run = _run(M.scenario(monkeypatch, **M.NOISE_SCENARIOS[name]), cap, form)
    assert run.n_out >= 40


def test_gross_noise_and_rescoring_at_once_vs_oracle(monkeypatch):
    """The closest to real footage: noisy keypoints with unreliable scores, form A."""
    sc = M.BOTH_SCENARIOS['A-5']
    run = _run(M.scenario(monkeypatch, **sc), sc['cap'], 'A')
    assert run.n_out >= 20


BATCHED = [('E', 12, 'E-12', 'E-12', 'E-12'), ('F', 31, 'D-31', 'DF-31', 'F-31')]


@pytest.mark.parametrize('form,C,score,noise,both', BATCHED, ids=['%s-c%d' % c[:2] for c in BATCHED])
def test_batched_scenarios_match_single_scenes_and_oracle(lib, monkeypatch, form, C, score, noise, both):
    """Three scenes in one launch -- one re-scored, one with gross noise, one with both: each scene's record equals, frame by frame and
    word for word, what a single-scene handle of the same capacities gives; scene 0's single-scene handle is the facade's, checked
    against the oracle."""
    scs = [M.SCORE_SCENARIOS[score], M.NOISE_SCENARIOS[noise], M.BOTH_SCENARIOS[both]]
    max_dets, max_tracks = scs[0]['cap']
    assert all(sc['cap'] == (max_dets, max_tracks) and sc['rig'] == C for sc in scs)
    seqs = [M.scenario(monkeypatch, **sc) for sc in scs]
    size = seqs[0]['meta']['size']
    S, n_frames = len(seqs), M.SCENARIO_FRAMES
    run = M.FacadeVsOracle(seqs[0], max_dets, max_tracks, F=seqs[0]['F'])
    cams = run.dev.cameras
    hb = M.handle_for(lib, size, cams, max_dets, max_tracks, n_scenes=S)
    assert hb.plan() == M.PLANS[form]
    singles = [M.handle_for(lib, size, cams, max_dets, max_tracks) for _ in range(1, S)]
    assert all(h.plan() == M.PLANS['C' if form == 'E' else 'D'] for h in singles)
    packed = [synth.pack_frames(q['frames'], max_dets) for q in seqs]
    n_tracks = [0] * S
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
        for s in range(S):
            n_tracks[s] += int(oi[s][0])
    assert run.n_out >= 40 and min(n_tracks) >= 40, (run.n_out, n_tracks)
    for h in singles:
        h.close()
    hb.close()


# ---- operators that had golden vectors only: seeded comparisons with the oracle's functions ---------------------------------------------
TOL = 1e-9


def _mask(keep_idx):
    m = 0
    for k in keep_idx:
        m |= 1 << int(k)
    return m


@pytest.fixture(scope='module')
def rig32(lib):
    """A 32-view Panoptic rig: the oracle's cameras and a handle on them (module-wide: the 32 x 32 fundamental matrices take a second)."""
    from oracle import cpu_ref as O
    name, saved = 'M32_4', (dict(synth.SIZES), dict(synth.SIZE_TO_DATASET))
    synth.SIZES[name] = dict(C=32, P=4, w=1920, h=1080, f=1000.0)
    synth.SIZE_TO_DATASET[name] = 'Panoptic'
    try:
        seq = synth.make_sequence(name, n_frames=1, seed=11, outlier_p=0.0, occlusion_every=0, empty_view_every=0, shuffle=False)
        cams = O.make_cameras(seq['calib'])
        h = M.handle_for(lib, name, cams, 8, 16)
        cfg, conf = M.matcher(name)
    finally:
        synth.SIZES.clear(); synth.SIZES.update(saved[0])
        synth.SIZE_TO_DATASET.clear(); synth.SIZE_TO_DATASET.update(saved[1])
    yield dict(cams=cams, h=h, cfg=cfg, seq=seq)
    h.close()


def test_track_affinity_count_gate_and_time_gaps_vs_oracle(rig32):
    """op_track_affinity beyond the goldens' inputs: detections with exactly k = 9 .. 12 joints within the association radius (0.25 alpha2d
    dt from the re-projection, the rest at 3 alpha2d dt) -- 0 up to k = 10, positive from 11 -- at the time gaps 1 and 2, at 0 (the
    division by zero must end as 0, as in the oracle) and at PAM_EXP_TABLE and beyond, where exp is called in place of the table."""
    from oracle import cpu_ref as O
    from pam import _lib
    cams, h, cfg = rig32['cams'], rig32['h'], rig32['cfg']
    rng = np.random.default_rng(41)
    gaps = [1, 2, 0, _lib.PAM_EXP_TABLE - 1, _lib.PAM_EXP_TABLE, _lib.PAM_EXP_TABLE + 6]
    tracks = np.stack([synth.TEMPLATE + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 0.0]) + rng.normal(0, 0.01, (17, 3)) for _ in gaps])
    for cid in (0, 17):
        reproj = O.project_tracks(cams[cid].P, tracks)                              # (n, 17, 2) rows (y, x)
        dets, ks = [], []
        for i, dt in enumerate(gaps):
            for k in (9, 10, 11, 12):
                near = rng.permutation(17)[:k]
                r = np.full(17, 3.0)
                r[near] = 0.25
                r = r * cfg['ALPHA2D'] * max(dt, 1)
                if dt == 0:
                    r[near[:3]] = 0.0                                               # 0 / 0 beside x / 0
                a = rng.uniform(0, 2 * np.pi, 17)
                yx = reproj[i] + (r * np.array([np.sin(a), np.cos(a)])).T
                dets.append(np.concatenate([yx, rng.uniform(0.7, 0.95, (17, 1))], axis=1))
                ks.append(k)
        dets = np.array(dets)
        exp = O.association_affinity(reproj, dets, gaps, cfg['ALPHA2D'], cfg['LAMBDA_A'])
        got = h.op_track_affinity(cid, tracks, gaps, dets)
        np.testing.assert_allclose(got, exp, rtol=TOL, atol=TOL)
        for i, dt in enumerate(gaps):
            own = exp[i, 4 * i:4 * i + 4]                                           # this track's four detections, k = 9 .. 12
            if dt == 0:
                assert np.all(exp[i] == 0) and np.all(got[i] == 0)
            else:
                assert own[0] == 0 and own[1] == 0 and own[2] > 0 and own[3] > 0, (dt, own)
                assert np.all(got[i][exp[i] == 0] == 0)
                pos = exp[i] > 0                                                    # 1e-84 at dt = 64: compared relative to itself
                np.testing.assert_allclose(got[i][pos], exp[i][pos], rtol=TOL, atol=0)


def test_hyp_cost_with_every_score_class_vs_oracle(rig32):
    """op_hyp_cost with members and candidate scored by every class of synth.draw_scores: negative scores enter the cost as weights,
    un-filtered, as in the reference (hypothesis.py:63); the veto needs a member cost above 1 AND a candidate confidence above 0.5 --
    none at exactly 0.5, at 0.4, or without any score >= 0."""
    from oracle import cpu_ref as O
    cams, h, cfg = rig32['cams'], rig32['h'], rig32['cfg']
    views = rig32['seq']['frames'][0]                                               # unshuffled: row p of every view is person p
    rng = np.random.default_rng(43)
    n_veto = n_held = n_half = 0
    for trial, (o_cls, m_cls) in enumerate([(a, b) for a in synth.SCORE_CLASSES for b in synth.SCORE_CLASSES]):
        for same in (True, False, False, False, False):
            cids = rng.permutation(32)[:int(rng.integers(1, 5))]
            o_cid = int(rng.choice([c for c in range(32) if c not in cids]))
            person = int(rng.integers(4))
            other = person if same else (person + 1 + int(rng.integers(3))) % 4
            poses = np.stack([views[c][person][:, [1, 0, 2]] for c in cids])
            o_pose = views[o_cid][other][:, [1, 0, 2]].copy()
            for q in range(len(cids)):
                poses[q, :, 2] = synth.draw_scores(m_cls if q == 0 else str(rng.choice(synth.SCORE_CLASSES)), rng)
            o_pose[:, 2] = synth.draw_scores(o_cls, rng)
            cs = [cams[int(c)] for c in cids]
            with np.errstate(invalid='ignore'):
                exp, veto = O.hyp_cost(cs, list(poses), cams[o_cid], o_pose, cfg['EPI_THRESHOLD'])
                ps = [O.hyp_cost([c], [p], cams[o_cid], o_pose, cfg['EPI_THRESHOLD'])[0] for c, p in zip(cs, poses)]
                bel = O.believe(o_pose)
            assert min(abs(p - 1) for p in ps) > TOL and abs(exp) > 1e-6            # a fair case: no member cost on the threshold
            got, gveto = h.op_hyp_cost(cids, poses, o_cid, o_pose)
            assert abs(got - exp) <= TOL * abs(exp), (o_cls, m_cls, same, got, exp)
            assert bool(gveto) == bool(veto), (o_cls, m_cls, same)
            above = max(ps) > 1
            n_veto += int(veto)
            n_held += int(above and not veto)
            if o_cls == 'half' and above:
                assert bel == 0.5 and not veto and not gveto                        # exactly 0.5 with p > 1: no veto
                n_half += 1
            if o_cls in ('negative', 'two_fifths'):
                assert not veto
    assert n_veto >= 5 and n_held >= 10 and n_half >= 3, (n_veto, n_held, n_half)


def _conflicts(kind, V, rng):
    """Symmetric 0/1 conflict graph on V views: sparse, dense, or chains along a random order of the views."""
    g = np.zeros((V, V), dtype=bool)
    if kind == 'chains':
        order = rng.permutation(V)
        for a, b in zip(order[:-1], order[1:]):
            if rng.uniform() < 0.8:
                g[a, b] = g[b, a] = True
    else:
        g = np.triu(rng.uniform(size=(V, V)) < (0.1 if kind == 'sparse' else 0.7), 1)
        g = g | g.T
    return g


@pytest.mark.parametrize('kind', ['sparse', 'dense', 'chains'])
def test_greedy_filter_random_conflict_graphs_vs_oracle(rig32, kind):
    """op_greedy in both modes for every V from 2 to 32.  Update mode: distinct random ray distances decide.  Init mode: float32
    affinities with magnitudes spread over 2^12, whose row sums depend on the summation order (the device restates NumPy's: eight
    accumulators and a tail for V % 8 != 0), and exact row-sum ties from duplicated rows.  The kept-view masks must be identical,
    bit 31 at V = 32 included."""
    from oracle import cpu_ref as O
    cams, h = rig32['cams'], rig32['h']
    rng = np.random.default_rng(['sparse', 'dense', 'chains'].index(kind) + 47)
    bit31 = dropped = ties = order_matters = 0
    for V in range(2, 33):
        for rep in range(2 if V < 32 else 6):
            g = _conflicts(kind, V, rng)
            cids = rng.permutation(32)[:V]
            cs = [cams[int(c)] for c in cids]
            # update mode
            aff = np.where(g, -rng.uniform(0.1, 1, (V, V)), rng.uniform(0.1, 1, (V, V)))
            aff = np.triu(aff, 1) + np.triu(aff, 1).T + np.eye(V)
            pose_j = np.stack([rng.uniform(0, 1080, V), rng.uniform(0, 1920, V), rng.uniform(0.7, 0.95, V)], axis=1)
            nxt = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0, 2)])
            rays = sorted(O.ray_point_distance(cs[k], pose_j[k], nxt) for k in range(V))
            assert min((b - a) / b for a, b in zip(rays[:-1], rays[1:])) > TOL      # distinct: no comparison hangs on the last bits
            keep, _ = O.greedy_filter(cs, aff, 'update', pose_j, nxt)
            got = h.op_greedy('update', cids, aff, pose_j, nxt)
            assert got == _mask(keep), (kind, V, 'update')
            bit31 += int(V == 32 and (got >> 31) & 1)
            # init mode: strided float32 rows as the reference slices them (affinity_mat[:, :, j])
            a3 = np.zeros((V, V, 3), dtype=np.float32)
            mag = (rng.uniform(1, 2, (V, V)) * 2.0 ** rng.integers(0, 13, (V, V))).astype(np.float32)
            a3[:, :, 1] = np.where(g, -mag, mag)
            a32 = a3[:, :, 1]
            a32[np.arange(V), np.arange(V)] = 1.0                                   # a view never conflicts with itself
            if rep % 2 == 1 and V >= 3:
                # an exact tie between the conflicting views 0 and 1: row 1 is row 0 with columns swapped in pairs that feed two
                # accumulators added to each other first (0 <-> 1, 8 <-> 9, ... inside the blocked part; the first two of a short row)
                a32[0, 1] = -abs(a32[0, 1])
                row = a32[0].copy()
                for b in range(0, V - V % 8 if V >= 8 else 2, 8):
                    row[[b, b + 1]] = row[[b + 1, b]]
                a32[1] = row
                assert np.sum(a32[0]) == np.sum(a32[1]) and a32[1, 1] == 1.0
                ties += 1
            sums = [np.sum(a32[r]) for r in range(V)]
            order_matters += int(any(np.float32(sum(float(x) for x in a32[r])) != sums[r] for r in range(V)))
            keep, _ = O.greedy_filter(cs, a32, 'init')
            got = h.op_greedy('init', cids, np.ascontiguousarray(a32))
            assert got == _mask(keep), (kind, V, 'init', rep)
            bit31 += int(V == 32 and (got >> 31) & 1)
            dropped += int(len(keep) < V)
    assert dropped >= 20 and ties >= 20 and order_matters >= 20, (dropped, ties, order_matters)
    if kind != 'dense':
        assert bit31 >= 1
