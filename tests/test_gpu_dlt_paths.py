"""The device DLT on every solver path against the 50-digit truth of tests/golden/dlt_edges.npz (tests/dlt_ref.py).

Every fixture case goes through ``pam_op_dlt_paths`` with solver 0 (inverse iteration, Jacobi when it does not converge: what k_frame
runs) and solver 1 (Jacobi alone); the wide inputs through the four-way fold / pack / merge form and again unsplit.  Rules, with
eps = 2**-52, amp = 1 + |X_true|^2, rho = s4 / s3:
  accuracy   joints with s3 - s4 > 1e-9 s1:  |X_dev - X_true|_max <= M max(|X_lapack - X_true|_max, 32 eps amp).  LAPACK's own error
             against the truth is the yardstick, not LAPACK's output.
  residual   every finite output, x = [X_dev, 1] normalised:  ||A x|| - s4 <= 8 eps s1.  A non-finite output is allowed only on a
             rank-deficient joint on which LAPACK is non-finite or wrong by more than 1e-3 as well.
  paths      solver 0: rho < 0.04 reports inverse iteration, rho > 0.2 reports Jacobi; in between, and on noise-free joints (s4 <
             1e-12 s1: an exact zero pivot may occur), either.  The issue's band is 0.02 .. 0.3; this one is inside it, as narrow as the
             iteration's arithmetic decides (derivation at dlt_ref.RHO_FAST).  solver 1: always Jacobi.  Fewer than two kept views: path
             0 and next_pose bit for bit.
  table      two-view joints of ages (0, 4) and (0, 9), which the accuracy rule mostly lets off: finite and within 32 eps amp kappa of the
             truth, kappa of the rows with their weights divided out.
  split      the nsplit = 4 and nsplit = 1 outputs of a wide input both meet the accuracy rule; two nsplit = 4 calls are identical.
             That last check pins only that the merge order is FIXED: swapping the order of dlt_merge's parts changes the rounding,
             not the result's quality, and fails nothing here but (if it varied from call to call) the repeatability check.

MEASURED on an MI355X (worst accuracy ratio err_dev / max(err_lapack, 32 eps amp) per family; solver 0 / solver 1):
  well 0.12 / 0.17    wide 0.14 / 0.14    wide, split 0.12 / 0.14    outlier 0.12 / 0.12    aged 0.03 / 0.03    mixed 0.12 / 0.16
  table 0.07 / 0.09   far 0.03 / 0.03     baseline 9.4 / 9.4
Residual (||A x|| - s4) / (eps s1): at most 1.7 (mixed, solver 1); no non-finite output.  Paths: 375 joints must converge, 129 must fall
back (3 of them in the split form), none against the rule.  Two-view table joints against the truth: at most 1.25 of the bound's 32.

M = 4 holds with a factor 20 to spare everywhere but in the baseline family, which needs M = 9.4 and is held to 16 (the ceiling).  No
operation loses digits there: both solvers give the same figure, so it is not the solver; folding the oracle's own rows instead of the
device's gives the same (10.8 in a NumPy restatement), so it is not the row construction; and against the first-order bound of a
backward-stable method, eps amp s1 / (s3 - s4), the device's worst error in that family is 0.14 and LAPACK's 0.21 (printed per family;
elsewhere the device stays below 1.1 where LAPACK reaches 15).  The bar is a ratio of two error SAMPLES of the same size, and over the
300 joints of this family -- s1 / (s3 - s4) of 1e3 .. 1e7 -- LAPACK's sample is, on a few joints, ten times below its typical one.  So the
family is also held to the first-order bound itself, at 2 (FIRST_ORDER_BASELINE), which does not depend on LAPACK's luck.  fp64 rsqrt and
the absence of FMA contraction (-ffp-contract=off) cost nothing measurable.

What the fixture found in the solver (fixed with it): on baseline joints with small rho (s1 / s3 ~ 1e3) the inverse iteration had converged
but its iterates kept moving by 3e-15 .. 7e-15, never meeting the 1e-15 test, and Jacobi ran: 3 joints under the issue's rho < 0.02.
min_right_singular_vector_tri now accepts that state at its last step; by a NumPy restatement of the device code 15 joints of this fixture
return through that clause, 14 of the baseline family, where the first-order bar above watches them, and 1 of the mixed family.

Tried on the device (with the issue's band): the 1e-15 test turned into `e <= 0.0` makes 61 joints that must converge report Jacobi (not
all: many iterations reach a fixed point bit for bit) and the path test fails; one Jacobi rotation off by 1e-9 fails accuracy and
residual for solver 1 in every family.  On the restatement: a weight beyond the table clamped to the table's last entry puts the
(4, 4, 5) call's accuracy ratio at 1e11; a zero weight there leaves every table joint non-finite.
"""
import numpy as np
import pytest

import dlt_ref as D
from oracle import cpu_ref as O
from pam import synth

pytestmark = pytest.mark.gpu

M = 4.0
M_BASELINE = 16.0          # the baseline family alone; see MEASURED
# ... whose bar that does not lean on LAPACK's luck is the first-order one: err <= 2 eps amp s1 / (s3 - s4), a backward error of 2 eps s1
# for a joint of two views -- four rows, each through at most four rotations whose c and s carry a rounding of rsqrt and one of a product
FIRST_ORDER_BASELINE = 2.0


@pytest.fixture(scope='module')
def runs():
    """Every case through the device once per solver (the split ones twice), LAPACK once: list of dicts."""
    from pam import _lib
    cases, P32 = D.load()
    cfg = dict(synth.MATCHER_CFG['Panoptic']); conf = cfg.pop('CONF_THRESHOLD')
    assert cfg['LAMBDA_T'] == D.LAMBDA_T
    rigs, handles = {}, {}
    for name in D.RIGS:
        R = rigs[name] = D.rig(name)
        assert np.array_equal(R['P32'], P32[name])                       # the fixture's cameras are the ones the device gets
        h = handles[name] = _lib.Handle(R['C'], _lib.make_params(cfg, conf))
        h.set_cameras(R['P32'], R['F'], R['RK_INV'], R['position'])
    out = []
    for c in cases:
        h = handles[c['rig']]
        A, mask, nviews = D.systems(c, rigs[c['rig']])
        r = dict(case=c, A=A, mask=mask, cls=D.classify(c), lapack=O.dlt_solve(A, mask, nviews, c['next_pose']), X={}, path={})
        for solver in (0, 1):
            r['X'][solver], r['path'][solver] = h.op_dlt_paths(c['cids'], c['Ts'], c['pose_mat'], c['masks'], c['next_pose'],
                                                               nsplit=c['nsplit'], solver=solver)
        if c['nsplit'] == 4:
            r['again'] = h.op_dlt_paths(c['cids'], c['Ts'], c['pose_mat'], c['masks'], c['next_pose'], nsplit=4, solver=0)
        out.append(r)
    yield out
    for h in handles.values():
        h.close()


def _key(r):
    return r['case']['family'] + ('/split' if r['case']['nsplit'] == 4 else '')


def test_accuracy_against_lapacks_own_error(runs):
    worst, cond, over = {}, {}, []
    for r in runs:
        c, full = r['case'], r['cls']['full']
        bar = M_BASELINE if c['family'] == 'baseline' else M
        # first-order bound of a backward-stable solver: eps s1 / (s3 - s4) in the unit null vector, times amp
        first_order = D.EPS * D.amp(c) * c['s'][:, 0] / (c['s'][:, 2] - c['s'][:, 3])
        for solver in (0, 1):
            ratio = D.accuracy_ratio(r['X'][solver], r['lapack'], c)
            assert np.isfinite(r['X'][solver][full]).all(), (c['index'], solver)       # a full-rank joint has a finite output
            k = (_key(r), solver)
            worst[k] = max(worst.get(k, 0.0), float(ratio[full].max()) if full.any() else 0.0)
            for who, X in (('device', r['X'][solver]), ('lapack', r['lapack'])):
                e = (D.error(X, c) / first_order)[full]
                cond[(k, who)] = max(cond.get((k, who), 0.0), float(e.max()) if full.any() else 0.0)
            over += [(c['index'], int(j), solver, float(ratio[j]), float(r['cls']['rho'][j])) for j in np.nonzero(full & (ratio > bar))[0]]
            if c['family'] == 'baseline':
                fo = D.first_order_ratio(r['X'][solver], c)
                over += [(c['index'], int(j), solver, 'first order', float(fo[j])) for j in np.nonzero(full & (fo > FIRST_ORDER_BASELINE))[0]]
    for k in sorted(worst):
        print('accuracy ratio  %-16s solver %d  worst %.3f   error / (eps amp s1 / (s3 - s4)): device %.3f, lapack %.3f'
              % (k[0], k[1], worst[k], cond[(k, 'device')], cond[(k, 'lapack')]))
    assert not over, over


def test_two_view_table_joints_against_the_truth_directly(runs):
    """Ages (0, 4) and (0, 9): the accuracy rule lets 18 of these 30 joints off as rank-deficient (s3 ~ exp(-5 T)) and LAPACK's normwise
    bound says nothing about the rest, but the truth is well defined and a row-wise stable solver reaches it: every joint finite and
    within 32 eps amp kappa of the truth, kappa = s1 / (s3 - s4) of the rows with their weights divided out (dlt_ref.unweighted_kappa;
    LAPACK is at 5.2 of that bound's 32, test_dlt_ref.py).  What this catches is a weight that is zero, huge or NaN -- X moves with the
    small weight only at second order; the RATIO of two computed weights is what the three-view table calls pin, through the accuracy rule."""
    n = 0
    for r in runs:
        c = r['case']
        if c['family'] != 'table' or c['Ts'][0] != 0:
            continue
        bound = D.EPS * D.amp(c) * D.unweighted_kappa(r['A'], r['mask'])
        solved = r['cls']['solved']
        for solver in (0, 1):
            X = r['X'][solver]
            assert np.isfinite(X[solved]).all(), (c['index'], solver)
            direct = D.error(X, c) / bound
            print('table %s solver %d  error / (eps amp kappa_unweighted): worst %.3f' % (tuple(int(t) for t in c['Ts']), solver, direct[solved].max()))
            assert (direct[solved] <= D.TABLE_DIRECT).all(), (c['index'], solver, direct)
        n += int(solved.sum())
    assert n == 30
    full3 = [r for r in runs if r['case']['family'] == 'table' and len(r['case']['Ts']) == 3]
    assert len(full3) == 2 and all(r['cls']['full'][r['cls']['solved']].all() for r in full3)


def test_residual_and_non_finite_outputs(runs):
    worst, n_bad = {}, 0
    for r in runs:
        c, cls = r['case'], r['cls']
        for solver in (0, 1):
            X = r['X'][solver]
            res = D.residual_ratio(X, r['A'], r['mask'], c)
            k = (_key(r), solver)
            worst[k] = max(worst.get(k, -np.inf), float(np.nanmax(res)))
            finite = np.isfinite(X).all(1)
            for j in np.nonzero(cls['solved'] & ~finite)[0]:
                n_bad += 1
                assert not cls['full'][j], (c['index'], j, solver)
                lap = r['lapack'][j]
                assert not np.isfinite(lap).all() or D.error(r['lapack'], c)[j] > D.LAPACK_WRONG, (c['index'], j, solver)
            assert not (res[cls['solved'] & finite] > D.RESIDUAL).any(), (c['index'], solver, res)
    for k in sorted(worst):
        print('residual / (eps s1)  %-16s solver %d  worst %.3f' % (k[0], k[1], worst[k]))
    print('non-finite outputs: %d' % n_bad)


def test_the_product_rule_takes_the_path_rho_dictates(runs):
    n = {1: 0, 2: 0}
    wrong = []
    for r in runs:
        must, path = r['cls']['must'], r['path'][0]
        assert set(path[r['cls']['solved']]) <= {1, 2}
        for want in (1, 2):
            n[want] += int((must == want).sum())
        wrong += [(r['case']['index'], int(j), float(r['cls']['rho'][j]), int(path[j])) for j in np.nonzero((must > 0) & (path != must))[0]]
    print('joints that must converge: %d, that must fall back: %d; against the rule: %d' % (n[1], n[2], len(wrong)))
    assert n[1] >= 100 and n[2] >= 100
    assert not wrong, wrong


def test_jacobi_alone_reports_jacobi(runs):
    for r in runs:
        assert (r['path'][1][r['cls']['solved']] == 2).all(), r['case']['index']


def test_joints_without_two_views_copy_the_prediction(runs):
    n = 0
    for r in runs:
        idle = ~r['cls']['solved']
        assert idle.sum() == 2
        for solver in (0, 1):
            assert (r['path'][solver][idle] == 0).all()
            assert r['X'][solver][idle].tobytes() == np.ascontiguousarray(r['case']['next_pose'][idle]).tobytes()
        n += int(idle.sum())
    assert n == 2 * len(runs)


def test_split_form_is_repeatable_and_has_its_unsplit_twin(runs):
    """Both forms of a wide input are in test_accuracy_against_lapacks_own_error's loop; here: they ARE the same input, the split form
    covers V = 9, 31, 32, enough joints, a fall-back, and gives the same bits on a second call (the merge order is fixed)."""
    split = [i for i, r in enumerate(runs) if r['case']['nsplit'] == 4]
    assert {9, 31, 32} <= {len(runs[i]['case']['cids']) for i in split}
    n = slow = 0
    for i in split:
        a, b = runs[i], runs[i + 1]
        assert b['case']['nsplit'] == 1 and all(np.array_equal(a['case'][f], b['case'][f]) for f in D.INPUTS)
        X, path = a['again']
        assert X.tobytes() == a['X'][0].tobytes() and np.array_equal(path, a['path'][0])
        n += int(a['cls']['solved'].sum())
        slow += int((a['path'][0] == 2).sum())
    assert n >= 60 and slow >= 1


def test_bad_selector_is_refused(runs):
    from pam import _lib
    c = runs[0]['case']
    R = D.rig(c['rig'])
    cfg = dict(synth.MATCHER_CFG['Panoptic']); conf = cfg.pop('CONF_THRESHOLD')
    h = _lib.Handle(R['C'], _lib.make_params(cfg, conf))
    h.set_cameras(R['P32'], R['F'], R['RK_INV'], R['position'])
    for kw in (dict(nsplit=2), dict(nsplit=0), dict(solver=2), dict(solver=-1)):
        with pytest.raises(_lib.PamError, match='error -1'):
            h.op_dlt_paths(c['cids'], c['Ts'], c['pose_mat'], c['masks'], c['next_pose'], **kw)
    with pytest.raises(_lib.PamError, match='error -1'):
        h.op_dlt_paths(c['cids'] + R['C'], c['Ts'], c['pose_mat'], c['masks'], c['next_pose'])
    h.close()
