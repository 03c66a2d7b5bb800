"""tests/golden/dlt_edges.npz is what tests/dlt_ref.py generates, LAPACK alone meets every bar test_gpu_dlt_paths.py sets for the device,
and the fixture is populated where the rules bite -- all on the CPU, so the bars are known to be reachable before a GPU is involved.

Caps on the fixture (1 054 joints in 62 calls, 930 of them solved):
  * rank-deficient joints (s3 - s4 <= 1e-9 s1, left out of the accuracy rule) are at most 3 % of all joints: 18 = 1.7 %;
  * they occur only in the noise-free baseline family, the noise-free aged-only family and -- WIDER than the issue's list, which cannot hold
    with its own cases -- the two-view table-edge calls.  That is arithmetic, not geometry: two of a joint's four rows carry the weight
    exp(-5 T), so s3 <= sqrt(2) exp(-5 T): 2.9e-9 at T = 4 (3 joints under the 1e-9 s1 gap, 12 over) and 4e-20 at T = 9 (all 15 under).
    Those joints are not let off: every two-view table joint is held to the truth directly (dlt_ref.unweighted_kappa), and the three-view
    table calls are full rank.  On this fixture the two noise-free families have none: the float32 P keeps the two baseline rays 1e-7
    apart, and a common weight leaves the relative gap alone;
  * at least 100 joints must report inverse iteration by rule (375) and at least 100 Jacobi (129);
  * at least 60 joints go through nsplit = 4 (105), and the split form has joints that must fall back (3, from the 30 px calls);
  * joints on which either path is accepted: 426 = 40 %, against the 25 % the issue hoped for.  184 (17 %) are noise-free -- the families'
    11 noise-free calls and the T = 9 call, either path by the issue's own rule.  242 (23 %) lie in the band RHO_FAST .. RHO_SLOW =
    0.04 .. 0.2, already narrowed from the issue's 0.02 .. 0.3 as far as the iteration's arithmetic decides (dlt_ref.py); inside it the
    start vector's luck decides, and a restatement of the device code switches anywhere in 0.078 .. 0.121.  Both shares are asserted."""
import numpy as np

import dlt_ref as D
from oracle import cpu_ref as O


def _fixture():
    cases, P32 = D.load()
    rigs = {name: D.rig(name) for name in D.RIGS}
    return cases, P32, rigs


def test_fixture_regenerates_identically():
    import mpmath
    cases, P32, rigs = _fixture()
    fresh = D.generate()
    assert int(fresh['n_cases']) == len(cases)
    for name in D.RIGS:
        assert np.array_equal(fresh[name + '.P32'], P32[name]) and np.array_equal(rigs[name]['P32'], P32[name])
    with mpmath.workdps(50):
        def mp(hi, lo):
            return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))
        for c in cases:
            k = 'c%02d.' % c['index']
            assert str(fresh[k + 'family']) == c['family'] and str(fresh[k + 'rig']) == c['rig']
            assert int(fresh[k + 'nsplit']) == c['nsplit'] and float(fresh[k + 'noise_px']) == c['noise_px']
            for f in D.INPUTS:
                assert fresh[k + f].dtype == c[f].dtype and fresh[k + f].tobytes() == c[f].tobytes(), (c['index'], f)
            cls = D.classify(c)
            for j in np.nonzero(cls['solved'])[0]:
                s1 = mp(c['s'][j, 0], c['s_lo'][j, 0])
                for e in range(4):
                    assert abs(mp(fresh[k + 's'][j, e], fresh[k + 's_lo'][j, e]) - mp(c['s'][j, e], c['s_lo'][j, e])) <= mpmath.mpf('1e-30') * s1
                if cls['full'][j]:
                    for e in range(3):
                        want = mp(c['X_true'][j, e], c['X_true_lo'][j, e])
                        got = mp(fresh[k + 'X_true'][j, e], fresh[k + 'X_true_lo'][j, e])
                        assert abs(got - want) <= mpmath.mpf('1e-30') * abs(want), (c['index'], j, e)
            assert np.isnan(c['X_true'][~cls['solved']]).all()


def test_lapack_alone_meets_every_bar():
    cases, _, rigs = _fixture()
    for c in cases:
        A, mask, nviews = D.systems(c, rigs[c['rig']])
        X = O.dlt_solve(A, mask, nviews, c['next_pose'])
        cls = D.classify(c)
        assert np.isfinite(X).all()
        # accuracy: the device's bar is M times LAPACK's own error, which LAPACK meets by construction; what it must meet here is the bound
        # that bar leans on, the first-order one of a backward-stable solver, within the 32 the accuracy floor allows for roundings
        assert (D.first_order_ratio(X, c)[cls['full']] <= D.FLOOR).all(), (c['index'], D.first_order_ratio(X, c))
        if c['family'] == 'table' and c['Ts'][0] == 0:
            direct = D.error(X, c) / (D.EPS * D.amp(c) * D.unweighted_kappa(A, mask))
            assert (direct[cls['solved']] <= D.TABLE_DIRECT).all(), (c['index'], direct)
        res = D.residual_ratio(X, A, mask, c)
        assert (res[cls['solved']] <= D.RESIDUAL).all(), (c['index'], res)
        assert X[~cls['solved']].tobytes() == np.ascontiguousarray(c['next_pose'][~cls['solved']]).tobytes()


def test_fixture_is_populated_where_the_rules_bite():
    cases, _, _ = _fixture()
    n = dict(all=0, deficient=0, either=0, noise_free=0, fast=0, slow=0, split=0)
    slow_form = set()
    for c in cases:
        cls = D.classify(c)
        assert (~cls['solved']).sum() == 2                                             # one joint without views, one with a single view
        deficient = cls['solved'] & ~cls['full']
        if deficient.any():
            assert (c['family'] == 'table' and len(c['Ts']) == 2) or (c['noise_px'] == 0.0 and c['family'] in ('baseline', 'aged')), (c['index'], c['family'])
        n['all'] += D.J; n['deficient'] += int(deficient.sum()); n['either'] += int((cls['must'] == -1).sum())
        n['noise_free'] += int(cls['noise_free'].sum())
        n['fast'] += int((cls['must'] == 1).sum()); n['slow'] += int((cls['must'] == 2).sum())
        if c['nsplit'] == 4:
            n['split'] += int(cls['solved'].sum())
        if (cls['must'] == 2).any():
            slow_form.add(c['nsplit'])
    assert n['deficient'] <= 0.03 * n['all'], n
    assert n['fast'] >= 100 and n['slow'] >= 100 and n['split'] >= 60, n
    assert slow_form == {1, 4}
    # see the module docstring: why not 25 % in all
    assert n['noise_free'] <= 0.18 * n['all'] and n['either'] - n['noise_free'] <= 0.25 * n['all'], n
    families = {c['family'] for c in cases}
    assert families == {'well', 'wide', 'outlier', 'aged', 'mixed', 'table', 'far', 'baseline'}
    assert {9, 31, 32} <= {len(c['cids']) for c in cases if c['nsplit'] == 4}
    assert {tuple(c['Ts']) for c in cases if c['family'] == 'table'} == {(0, 4), (0, 9), (4, 4, 5), (9, 10, 9)}
    assert len(cases) == 62 and n['all'] == 1054
