"""CPU witness of the scenarios that test_gpu_tracker_scenarios.py runs on the device: the ORACLE alone, with spies round its decision
points (tracker_matrix.Witness).  A comparison of two implementations proves nothing about a branch neither took, and is a lottery where
a decision hangs on the last bits of a sum; so every sequence is shown here to drive the oracle through the branches it is meant for,
often enough, and to keep every decision at least 1e-9 away from its threshold.  The seeds were chosen for that, on the CPU; the counts
they give stand beside the cases.

Score scenarios (synth.rescore_frames), per rig: unmatched detections dropped by the confidence filter in each of the classes low,
negative (the mean over no score is NaN), exactly on the threshold, and -- mixed -- decided with the mean over s >= 0 above the threshold
where the plain mean of all 17 scores is not above it (the reference keeps these: an implementation that averaged every score would drop
them); on the 0.4 rigs vetoes suppressed by a confidence in (0.4, 0.5]; and the filter matters: at least half of the frames emit other
ids or camera ids than with the filter switched off.
Noise scenarios (40 px, every second pose with an outlier), per launch form: updates rejected, updates accepted with copied joints, init
filters with conflicts, rejected hypotheses, association pairs on either side of the count gate.

The 1e-6 m bar of FacadeVsOracle.step under gross noise: as for FALLBACK in test_gpu_tracker_matrix.py, LAPACK's worst error over the
systems the oracle solves on each gross-noise sequence was measured against the 50-digit SVD of tests/dlt_ref.py
(tracker_matrix.lapack_worst_error); the figure stands beside the case and is below 1e-7 m for every one of them."""
import warnings

import numpy as np
import pytest

import golden_io as G
import tracker_matrix as M
from pam import synth

MARGIN = 1e-9


def _golden_seq(size):
    tr = G.load('trace_%s.npz' % size)
    c = G.cameras(size)
    base = str(tr['meta.size'])
    return dict(calib={'P': c['P'], 'K': c['K'], 'RT': c['RT']}, F=c['F'], frames=G.trace_frames(tr), meta=dict(size=base))


def _margins(w, name):
    assert w.margin_cost > MARGIN, (name, w.margin_cost)        # no hypothesis member cost within 1e-9 of 1
    assert w.margin_c > MARGIN, (name, w.margin_c)              # no association term within 1e-9 of 0
    assert w.margin_aff > MARGIN, (name, w.margin_aff)          # no filter affinity within 1e-9 of 0
    assert w.margin_cmp > MARGIN, (name, w.margin_cmp)          # compared ray distances / row sums: bitwise equal or 1e-9 apart


def _fits(w, seq, cap, name):
    """No frame needs more hypothesis or track slots than the handles of the GPU case have (a full handle raises a status bit and
    stops following the reference: a limit of the capacities, not the disagreement these scenarios look for)."""
    max_dets, max_tracks = cap
    C = len(seq['frames'][0])
    assert max(len(v) for views in seq['frames'] for v in views) <= max_dets, name
    assert w.max_hyps <= min(4 * max_dets, C * max_dets), (name, w.max_hyps)
    assert w.max_tracks <= max_tracks, (name, w.max_tracks)


def _assert_scores(w, conf, name):
    assert w.dropped['low'] >= 3 and w.dropped['negative'] >= 3 and w.dropped['equal'] >= 3, (name, w.dropped)
    assert w.mixed_split >= 3, (name, w.mixed_split)
    if conf == 0.4:
        assert w.veto_suppressed >= 3, (name, w.veto_suppressed)


def _assert_noise(w, name):
    assert w.rejected_updates >= 5, (name, w.rejected_updates)     # more than J / 3 joints failed
    assert w.copied_updates >= 20, (name, w.copied_updates)        # accepted with 1 to 5 joints copied from the prediction
    assert w.init_conflicts >= 20, (name, w.init_conflicts)
    assert w.rejected_hyps >= 3, (name, w.rejected_hyps)
    assert w.cnt10 >= 20 and w.cnt11 >= 20, (name, w.cnt10, w.cnt11)


def _filter_matters(seq, out, name):
    base, _ = M.run_oracle(seq, conf=-1)
    differ = sum(a != b for a, b in zip(out, base))
    assert 2 * differ >= len(out), (name, differ)
    return differ


# counts: dropped low / negative / equal, mixed split, vetoes suppressed, frames (of 40) that differ without the filter
SCORE_CASES = [
    'S1s',       # seed 703 / 1703:  11 /  4 /  4,   5,   4, 37      (the golden traces, as stored)
    'S2s',       # seed 409 / 1409:   6 /  7 /  6,   6,   -, 38      (CONF_THRESHOLD 0.5: no veto can be suppressed)
    'S3s',       # seed 406 / 1406:  14 /  9 / 11,   6,  10, 38
    'A-S1',      # seed 714 / 1714:   9 /  4 /  6,   7,   4, 38
    'A-S2',      # seed 410 / 1410:  15 /  7 /  6,   9,   -, 38
    'C-12',      # seed 403 / 1403:  15 /  7 /  9,   8,  15, 38
    'D-31',      # seed 405 / 1405:  40 / 19 / 24,  33, 169, 38
    'E-12',      # seed 404 / 1404:  11 / 10 /  8,  15,   9, 38
]


@pytest.mark.parametrize('name', SCORE_CASES)
def test_score_scenario_reaches_its_branches(monkeypatch, name):
    seq = _golden_seq(name) if name in G.RESCORED else M.scenario(monkeypatch, **M.SCORE_SCENARIOS[name])
    conf = M.matcher(seq['meta']['size'])[1]
    out, w = M.run_oracle(seq, witness=True)
    differ = _filter_matters(seq, out, name)
    print(name, w.counts(), 'differ', differ)
    _assert_scores(w, conf, name)
    _margins(w, name)
    _fits(w, seq, (8, 16) if name in G.RESCORED else M.SCORE_SCENARIOS[name]['cap'], name)
    assert sum(len(o[0]) for o in out) >= 40                        # and tracks are emitted all the same


# counts: updates rejected, accepted with 1-5 copied joints, init filters with a conflict, rejected hypotheses, pairs at cnt 10 / 11,
# most hypotheses / tracks in a frame; LAPACK's worst error against the 50-digit SVD over the systems the oracle solves
NOISE_CASES = [
    'AB-5',      # seed 411:              43,  62,  855, 45,   69 /   60,   6 /  8;   1.8e-9 m over 1 966 systems
    'E-12',      # seed 413:              53, 193,  690, 24,  551 /  437,  10 / 17;   3.6e-9 m over 5 386 systems
    'DF-31',     # seed 447 (3 persons):  26, 239,  799, 30, 1996 / 1562,   9 / 27;   1.6e-8 m over 9 502 systems
]


@pytest.mark.parametrize('name', NOISE_CASES)
def test_noise_scenario_reaches_its_branches(monkeypatch, name):
    seq = M.scenario(monkeypatch, **M.NOISE_SCENARIOS[name])
    out, w = M.run_oracle(seq, witness=True)
    print(name, w.counts())
    _assert_noise(w, name)
    _margins(w, name)
    _fits(w, seq, M.NOISE_SCENARIOS[name]['cap'], name)


# both at once: the noise counts as above without hypotheses / tracks (6 / 8, 8 / 14, 7 / 23), then dropped low / negative / equal, mixed split, vetoes suppressed; LAPACK's worst error
BOTH_CASES = [
    'A-5',       # seed 426 / 1426 (MILD_MIX):   35,  51,  673, 72,   70 /   53;   40 / 33 /  31,  39,  62;   3.2e-9 m over 1 516 systems
    'E-12',      # seed 431 / 1431:              18, 128, 1053, 40,  353 /  269;  137 / 94 / 104, 124, 281;   7.0e-9 m over 3 913 systems
    'F-31',      # seed 433 / 1433 (3 persons):  32, 166,  693, 13, 1479 / 1180;  178 / 81 / 113, 117, 515;   4.6e-9 m over 7 342 systems
]


@pytest.mark.parametrize('name', BOTH_CASES)
def test_combined_scenario_reaches_both_kinds_of_branches(monkeypatch, name):
    seq = M.scenario(monkeypatch, **M.BOTH_SCENARIOS[name])
    conf = M.matcher(seq['meta']['size'])[1]
    out, w = M.run_oracle(seq, witness=True)
    print(name, w.counts())
    _assert_noise(w, name)
    _assert_scores(w, conf, name)
    _margins(w, name)
    _fits(w, seq, M.BOTH_SCENARIOS[name]['cap'], name)


def test_rescore_frames_scores_are_exact_and_coordinates_untouched():
    """Every class of synth.draw_scores: multiples of 1/64 in the stated range, so that the mean is the same double in any summation
    order (NumPy's pairwise mean, np.mean of a list as in the reference, a sequential loop as on the device); the two equality classes
    give exactly 0.5 and exactly the double 0.4; coordinates and detection counts are those of the input, which is left as it was."""
    seq = synth.make_sequence('S2', n_frames=30, seed=5, **M.STRESS)
    before = [[v.copy() for v in views] for views in seq['frames']]
    frames, classes = synth.rescore_frames(seq['frames'], 9, with_classes=True)
    again = synth.rescore_frames(seq['frames'], 9)
    seen = dict.fromkeys(synth.SCORE_CLASSES, 0)
    for views, old, same, cls in zip(frames, before, again, classes):
        for v, o, a, cl in zip(views, old, same, cls):
            assert v.shape == o.shape and np.array_equal(v[:, :, :2], o[:, :, :2]) and np.array_equal(v, a)
            for det, c in zip(v, cl):
                s = det[:, 2]
                seen[c] += 1
                assert M.score_class(s) == c
                assert np.array_equal(s * 64, np.round(s * 64))
                pos = s[s >= 0]
                seq_mean = (sum(float(x) for x in pos) / len(pos)) if len(pos) else float('nan')
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore', RuntimeWarning)
                    means = [np.mean(pos), np.mean(list(pos)), np.mean(pos[::-1])]
                assert all(m == seq_mean or (m != m and seq_mean != seq_mean) for m in means)
                if c == 'high':
                    assert s.min() >= 45 / 64 and s.max() <= 61 / 64
                elif c == 'low':
                    assert s.min() >= 20 / 64 and s.max() <= 30 / 64 and 0.31 < seq_mean < 0.47
                elif c == 'mixed':
                    assert 9 <= (s < 0).sum() <= 11 and pos.min() >= 45 / 64 and seq_mean > 0.5 and s.mean() < 0.4
                elif c == 'negative':
                    assert s.max() < 0 and seq_mean != seq_mean
                elif c == 'half':
                    assert seq_mean == 0.5
                else:
                    assert (s == -0.25).sum() == 12 and pos.sum() == 2.0 and seq_mean == 0.4
    assert min(seen.values()) >= 5, seen
    for views, old in zip(seq['frames'], before):
        assert all(np.array_equal(v, o) for v, o in zip(views, old))
    lows = [d[:, 2].mean() for views in frames for v in views for d in v if M.score_class(d[:, 2]) == 'low']
    assert min(lows) < 0.4 < max(lows) <= 0.5                          # both sides of 0.4, never above 0.5
