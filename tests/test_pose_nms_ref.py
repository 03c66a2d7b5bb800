"""CPU: the OKS-NMS rule of tests/pose_nms_ref.py against an explicit-loop second form (and against each wrong variant one could plant
in it), the closed loop that says why the step exists -- a tracker fed duplicated 2D poses grows ghost ids, fed the filtered ones it does
not notice -- plus the new symbol's binding and the shipped config."""
import ctypes
import math
import os

import numpy as np
import pytest

import pose_nms_ref as R
from oracle import cpu_ref as O
from pam import _lib, synth

VARIANTS = ('transitive', 'slot_order', 'unrescored', 'vis_mask', 'no_eps', 'score_order_out')


def loop_form(rows, area, b, oks_thre=0.9, in_vis_thre=0.2, variant=None):
    """The rule of include/pam.h once more, in scalar Python loops; variant: one of VARIANTS = the same with that one mistake planted.
    -> (kept slots in output order, scores)."""
    n = len(rows)
    sig = [.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]
    var = [float((np.float64(s) / 10.0 * 2) ** 2) for s in sig]
    score = []
    for i in range(n):
        tot, cnt = 0.0, 0
        for j in range(17):
            s = float(rows[i][j][2])
            if s > in_vis_thre:
                tot += s; cnt += 1
        mean = tot / cnt if cnt else 0.0
        score.append(float(b[i]) if variant == 'unrescored' else float(b[i]) * mean)

    def oks(p, q):
        acc, cnt = 0.0, 0
        den = (float(area[p]) + float(area[q])) / 2.0 + (0.0 if variant == 'no_eps' else 2.220446049250313e-16)
        for j in range(17):
            if variant == 'vis_mask' and not (rows[p][j][2] > in_vis_thre and rows[q][j][2] > in_vis_thre):
                continue
            dx, dy = float(rows[p][j][1]) - float(rows[q][j][1]), float(rows[p][j][0]) - float(rows[q][j][0])
            num = (dx * dx + dy * dy) / var[j]
            e = (num / den if den != 0.0 else (math.nan if num == 0.0 or num != num else math.inf)) / 2.0
            acc += math.exp(-e) if e == e else math.nan
            cnt += 1
        return acc / (cnt if variant == 'vis_mask' else 17) if cnt else 0.0
    key = [(-math.inf if s != s else s) for s in score]
    order = list(range(n)) if variant == 'slot_order' else sorted(range(n), key=lambda i: (-key[i], i))
    alive, keep = [True] * n, []
    for i in order:
        if not alive[i]:
            continue
        keep.append(i)
        alive[i] = False
        front = [i]
        while front:                                   # greedy: only the kept row kills; 'transitive': what it kills kills on
            k = front.pop()
            for q in range(n):
                if alive[q] and oks(k, q) > oks_thre:
                    alive[q] = False
                    if variant == 'transitive':
                        front.append(q)
    return (keep if variant == 'score_order_out' else sorted(keep)), score


def test_restatement_equals_the_loop_form_and_every_planted_fault_shows():
    cases = R.hand_cases()
    rows, area, b = cases['chain'][0]
    m = R.oks_matrix(rows, area)
    assert m[0, 1] > 0.9 + 1e-3 and m[1, 2] > 0.9 + 1e-3 and m[0, 2] < 0.9 - 1e-3          # the chain is a chain
    exposed = set()
    for name, ((rows, area, b), target) in cases.items():
        ref = R.nms_view(rows, area, b)
        keep, score = loop_form(rows, area, b)
        assert ref['keep'] == keep, name
        assert np.array_equal(ref['score'], np.array(score)), name
        for v in VARIANTS:
            if loop_form(rows, area, b, variant=v)[0] != keep:
                exposed.add(v)
        assert loop_form(rows, area, b, variant=target)[0] != keep, (name, target)
    assert exposed == set(VARIANTS)
    assert R.nms_view(*cases['chain'][0])['keep'] == [0, 2]
    assert R.nms_view(*cases['late_best'][0])['keep'] == [1, 2]
    assert R.nms_view(*cases['zero_area'][0])['keep'] == [0]
    assert np.array_equal(R.VARS, _lib.OKS_VARS)                                            # the constants the product hands the kernel
    # random views: the two forms agree on keep lists and on every score
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = int(rng.integers(0, 9))
        base = [R.skeleton(100 + trial * 10 + i) for i in range(n)]
        rows = np.stack([R.shifted(base[int(rng.integers(0, i + 1))], float(rng.uniform(0, 8)), float(rng.uniform(0.6, 1))) if i and rng.uniform() < 0.5
                         else base[i] for i in range(n)]) if n else np.zeros((0, 17, 3))
        area, b = rng.uniform(2000, 12000, n), rng.uniform(0.3, 1, n).astype(np.float32)
        ref = R.nms_view(rows, area, b)
        keep, score = loop_form(rows, area, b)
        assert ref['keep'] == keep and np.array_equal(ref['score'], np.array(score))
    # apply(): compaction, the zeroed tail, rows >= n untouched, a clamped count
    det = np.full((2, 5, 17, 3), 7.0)
    det[0, :3] = cases['late_best'][0][0]
    out = R.apply(det, [3, 9], 4, np.full((2, 4), 1e4))
    assert list(out['n_det_out']) == [2, 1] and out['keep_from'].tolist() == [[1, 2, -1, -1], [0, -1, -1, -1]]
    assert np.array_equal(out['det'][0, :2], det[0, 1:3]) and not out['det'][0, 2].any() and np.array_equal(out['det'][0, 3:], det[0, 3:])
    assert not out['det'][1, 1:4].any() and np.array_equal(out['det'][1, 4], det[1, 4])


# ---- the closed loop: duplicates make ghosts, the filter removes them -------------------------------------------------------------------
_RUN = {}


def tracker_run(key, frames):
    """ids and 3D poses the oracle's tracker emits per frame on `frames` (list[frame][view] of (n, 17, 3) (y, x, s))."""
    if key not in _RUN:
        seq = clean_sequence()
        cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
        trk = O.Tracker(O.Params(cfg, conf), O.make_cameras(seq['calib']))
        out = []
        for t, views in enumerate(frames):
            trk.step(t, views)
            got = trk.collect(t)
            out.append(([int(i) for i in got[5]], np.array(got[3])))
        _RUN[key] = out
    return _RUN[key]


def clean_sequence():
    if 'seq' not in _RUN:
        _RUN['seq'] = synth.make_sequence('S2', n_frames=130, seed=3)
    return _RUN['seq']


def duplicated(p):
    """-> (frames with duplicates appended behind each view's real rows, areas per frame and view, person label per row)."""
    rng = np.random.default_rng(11)
    frames, areas, labels = [], [], []
    for views in clean_sequence()['frames']:
        fv, fa, fl = [], [], []
        for d in views:
            rows, lab = [kp for kp in d], list(range(len(d)))
            for i, kp in enumerate(d):
                if rng.uniform() < p:
                    dup = kp.copy()
                    dup[:, :2] += rng.normal(size=(17, 2)) * 2.0
                    dup[:, 2] *= 0.97
                    rows.append(dup); lab.append(i)
            rows = np.stack(rows) if rows else np.zeros((0, 17, 3))
            boxes = [it['bbox'] for it in synth.to_dump_results([rows])[0][0]]
            fa.append(np.array([np.float64(np.float32(bx[2])) * np.float64(np.float32(bx[3])) for bx in boxes]))
            fv.append(rows[:, :, [1, 0, 2]]); fl.append(lab)
        frames.append(fv); areas.append(fa); labels.append(fl)
    return frames, areas, labels


@pytest.mark.parametrize('p', [0.1, 0.3])
def test_duplicates_grow_ghost_ids_and_the_filter_removes_them(p):
    clean = tracker_run('clean', [[d[:, :, [1, 0, 2]] for d in views] for views in clean_sequence()['frames']])
    frames, areas, labels = duplicated(p)
    n_dup = sum(len(l) - len(set(l)) for fl in labels for l in fl)
    assert n_dup > 200 * p / 0.1 * 0.9
    dirty = tracker_run(('dirty', p), frames)
    same = sum(a[0] == b[0] for a, b in zip(clean, dirty))
    print('p = %.1f: %d duplicates, unfiltered %d of %d frames keep the clean ids' % (p, n_dup, same, len(clean)))
    assert same < len(clean) / 2
    filtered, lo_dup, hi_other = [], 1.0, 0.0
    for fv, fa, fl in zip(frames, areas, labels):
        out = []
        for rows, area, lab in zip(fv, fa, fl):
            r = R.nms_view(rows, area, np.ones(len(rows), np.float32), oks_thre=0.9, in_vis_thre=0.2, oks_vars=_lib.OKS_VARS)   # the product's constants
            for i in range(len(rows)):
                for k in range(i + 1, len(rows)):
                    if lab[i] == lab[k]:
                        lo_dup = min(lo_dup, r['oks'][i, k])
                    else:
                        hi_other = max(hi_other, r['oks'][i, k])
            out.append(rows[r['keep']])
        filtered.append(out)
    print('smallest duplicate-vs-original OKS %.4f, largest OKS between two people %.4f' % (lo_dup, hi_other))
    assert lo_dup > 0.9 + 0.02 and hi_other < 0.5                      # conditions on the inputs: the threshold has room on both sides
    clean_in = [[d[:, :, [1, 0, 2]] for d in views] for views in clean_sequence()['frames']]
    assert all(np.array_equal(a, b) for fa_, fb in zip(filtered, clean_in) for a, b in zip(fa_, fb))     # every duplicate gone, nothing else
    got = tracker_run(('filtered', p), filtered)
    assert len(got) == 130 and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(clean, got))


# ---- the binding and the shipped config ---------------------------------------------------------------------------------------------------
def test_symbol_is_bound_and_refuses_bad_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    I, P, L, D = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double
    assert _lib._SIGS['pam_pose_nms'] == (I, [P, I, I, I, P, P, I, P, P, P, P, L, L, P, P, D, D, P, P, P])
    assert 'pam_pose_nms' in _lib.EXPORTS and callable(_lib.pose_nms) and _lib.POSE_NMS_MAX == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pam.h')).read()
    assert 'int pam_pose_nms(' in header
    fn = ctypes.CDLL(_lib.LIB_PATH).pam_pose_nms
    fn.restype, fn.argtypes = _lib._SIGS['pam_pose_nms']
    buf, other = (ctypes.c_int32 * 64)(), (ctypes.c_int32 * 64)()
    p, o = ctypes.cast(buf, P), ctypes.cast(other, P)
    vs = np.ascontiguousarray(R.VARS)
    v = vs.ctypes.data_as(P)
    good = [None, 5, 8, 8, p, p, 20, p, p, p, None, 0, 0, None, v, 0.9, 0.2, o, p, p]
    for at in (4, 5, 7, 8, 9, 14, 17, 18, 19):                          # each mandatory pointer NULL in turn
        a = list(good); a[at] = None
        assert fn(*a) == -1, at
    for at, bad in ((1, 0), (2, 0), (2, 33), (3, 7), (6, -1)):         # no views; max_dets outside 1..32; det_slots < max_dets; n_rows < 0
        a = list(good); a[at] = bad
        assert fn(*a) == -1, (at, bad)
    a = list(good); a[17] = p                                           # the counts filtered into themselves
    assert fn(*a) == -1
    assert list(buf) == [0] * 64 and list(other) == [0] * 64


def test_shipped_config_sets_the_three_keys():
    import pam
    from pam.dataset import GetConfig
    root = os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf')
    p = dict(GetConfig(os.path.join(root, 'model_configs_oksnms.yaml')).POSE_MODELS.HRPOSE)
    assert p['OKS_NMS'] is True and p['OKS_THRE'] == 0.9 and p['IN_VIS_THRE'] == 0.2
    stock = dict(GetConfig(os.path.join(root, 'model_configs.yaml')).POSE_MODELS.HRPOSE)
    assert not {'OKS_NMS', 'OKS_THRE', 'IN_VIS_THRE'} & set(stock)
