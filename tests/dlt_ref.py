"""The weighted DLT against a 50-digit SVD: the case table of tests/golden/dlt_edges.npz, its generator, and the acceptance rules that
test_dlt_ref.py (LAPACK, on the CPU) and test_gpu_dlt_paths.py (the device solver) share.  A plain module (not a conftest.py).

Every case is one call of ``pam_op_dlt_paths``: 17 joints on one list of views.  The stacked system of a joint is built by the oracle's
own ``O.dlt_rows`` from the float32 ``P`` widened to double (what the device reads) and cut by the joint's keep mask; its truth is
``mpmath.svd_r`` at 50 digits: ``X_true = x[:3] / x[3]`` of the right singular vector of the smallest singular value, and the four
singular values ``s1 >= .. >= s4``.  The fixture stores the truth as double-double pairs (hi + lo, ~32 digits), so that the GPU test
needs no mpmath and the CPU test can still compare a regenerated truth to 1e-30.

Regenerate the fixture with ``python tests/dlt_ref.py`` (fixed seeds; about ten seconds of mpmath).

Families (rings from ``synth.make_rig``: 5 views at 1032 x 776, 32 views at 1920 x 1080; LAMBDA_T = 5):
  well      2-5 of 5 views, noise 0 / 1.5 / 8 px, ages 0..3
  wide      9-32 of 32 views (V = 9, 31, 32 among them), noise 0 / 1.5 / 8 / 30 px, ages 0..3; every input twice: nsplit 4 and nsplit 1
  outlier   2-5 of 5 views, 30 px
  aged      2 views, both of age 3 (every row weighted exp(-15)), noise 0 / 1.5 / 30 px
  mixed     a fresh view beside aged ones: ages (0, 3) and (0, 1, 2), noise 0 / 1.5 px
  table     ages beyond the 4-entry weight table, exp(-lambda_t T) formed on the device.  (0, 4) and (0, 9), two views: X depends on the small
            weight only at second order (2e-9 squared), and the (0, 9) joints are rank-deficient by the 1e-9 gap (s3 <= sqrt(2) exp(-45)), so
            these two calls see only a gross fault (a zero, huge or NaN weight); they are held to the truth directly (TABLE_DIRECT).  (4, 4, 5)
            and (9, 10, 9), three views: every weight is computed, the system is full rank, and a wrong RATIO of the weights fails accuracy
  far       two adjacent cameras of the 32-ring, the point at 10 x, 100 x, 1000 x the rig radius along their common viewing direction
  baseline  two opposite cameras of the 32-ring, the point ON the segment between them (t = 0.3, 0.5): both rays are the same line
            (noise 0 / 0.5 / 1.5 px; the noisy calls over BASELINE_PAIRS seeded camera pairs each)
Every call has one joint without kept views and one with a single kept view (``next_pose`` is copied), at seeded positions."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cpu_ref as O                  # noqa: E402
from pam import synth                            # noqa: E402

J = 17
LAMBDA_T = 5
EPS = 2.0 ** -52
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dlt_edges.npz')
RIGS = {'r5': dict(C=5, w=1032, h=776, f=1000.0), 'r32': dict(C=32, w=1920, h=1080, f=1000.0)}
RADIUS = 5.0                                     # synth.make_rig's ring

# opposite camera pairs (seeded) per (noise, t) of the noisy baseline family: the one family whose s4 / s3 is of order 1 -- both singular
# values are the noise itself -- and so the one that supplies most joints that MUST take the Jacobi fall-back (about 4 in 10 of its joints)
BASELINE_PAIRS = 5

# acceptance rules (the issue's figures; M is the only one with a documented margin, see test_gpu_dlt_paths.py)
RANK_GAP = 1e-9                                  # compared in accuracy: s3 - s4 > RANK_GAP * s1
FLOOR = 32.0                                     # accuracy floor 32 eps amp: the roundings no fp64 solver avoids
RESIDUAL = 8.0                                   # ||A x|| - s4 <= 8 eps s1
# s4 / s3 below RHO_FAST: inverse iteration must converge; above RHO_SLOW: it cannot in 8 steps.  The issue's figures are 0.02 and 0.3;
# these are tighter, so its rule is implied.  With c = the start vector's v3 : v4 ratio, the step at iteration k is about c rho^(2k) and the
# 1e-15 test can be met at k = 7 at the latest.  rho = 0.04: 0.04^14 = 2.7e-20, converges unless c > 3.7e4 (the start within 3e-5 rad of
# orthogonal to the null vector).  rho = 0.2: 0.2^14 = 1.6e-10; the last-step acceptance of a stalled iteration needs the step before it
# under 1e-12, c 0.2^12 <= 1e-12, c <= 2.4e-4 (the start within 2.4e-4 rad of the null vector itself).  A NumPy restatement of the device
# code switches between rho = 0.078 (first Jacobi) and 0.121 (last convergence) on this fixture.
RHO_FAST, RHO_SLOW = 0.04, 0.2
TABLE_DIRECT = 32.0                              # table family: error <= 32 eps amp kappa(unweighted rows), see unweighted_kappa
NOISE_FREE = 1e-12                               # s4 < 1e-12 s1: an exact zero pivot may occur, either path
LAPACK_WRONG = 1e-3                              # a non-finite device output needs LAPACK non-finite or this far from the truth


def rig(name):
    """-> dict(cams = the oracle's camera objects, P32, F, RK_INV, position = what Handle.set_cameras takes).  The DLT reads P alone;
    F is left zero (32 x 32 float32 torch products that nothing here uses)."""
    r = RIGS[name]
    calib = synth.make_rig(r['C'], r['w'], r['h'], r['f'])
    made = O.make_cameras(calib, F=np.zeros((r['C'], r['C'], 3, 3), dtype=np.float32))
    arr = dict(P32=np.stack([c.P for c in made]), K32=np.stack([c.K for c in made]), RT32=np.stack([c.RT for c in made]),
               F=np.stack([c.F for c in made]), RK_INV=np.stack([c.RK_INV for c in made]), position=np.stack([c.position for c in made]))
    cams = O.cameras_from_arrays(arr['P32'], arr['K32'], arr['RT32'], arr['F'], arr['RK_INV'], arr['position'])
    return dict(arr, cams=cams, C=r['C'])


# ---- the case table ---------------------------------------------------------------------------------------------------------------
def _spec():
    """[(family, rig, nsplit, noise_px, kind-specific dict)] in fixture order; a wide input appears twice in a row (nsplit 4, then 1)."""
    s = []
    for noise, n in ((0.0, 1), (1.5, 3), (8.0, 3)):
        s += [('well', 'r5', 1, noise, dict(V=None))] * n
    for V, noise in ((9, 30.0), (31, 8.0), (32, 1.5), (12, 0.0), (9, 1.5), (10, 30.0), (20, 30.0)):
        s += [('wide', 'r32', 4, noise, dict(V=V)), ('wide', 'r32', 1, noise, dict(V=V, same_as_previous=True))]
    s += [('outlier', 'r5', 1, 30.0, dict(V=None))] * 3
    s += [('aged', 'r5', 1, noise, dict(Ts=(3, 3))) for noise in (0.0, 1.5, 30.0)]
    s += [('mixed', 'r5', 1, noise, dict(Ts=Ts)) for Ts in ((0, 3), (0, 1, 2)) for noise in (0.0, 1.5)]
    s += [('table', 'r5', 1, 1.5, dict(Ts=Ts)) for Ts in ((0, 4), (0, 9))]
    s += [('far', 'r32', 1, noise, dict(far=k)) for k in (10.0, 100.0, 1000.0) for noise in (0.0, 1.5)]
    s += [('baseline', 'r32', 1, 0.0, dict(t=(0.3, 0.5)))]
    s += [('baseline', 'r32', 1, noise, dict(t=(t,))) for noise in (0.5, 1.5) for t in (0.3, 0.5)] * BASELINE_PAIRS
    # beyond the table with the weight visible: three aged views whose weights differ by exp(-5); the odd view moves X by its weight
    # ratio squared, 4.5e-5 of the millimetres between the 2- and 3-view solutions, 1e5 times the accuracy bar
    s += [('table', 'r5', 1, 1.5, dict(Ts=Ts)) for Ts in ((4, 4, 5), (9, 10, 9))]
    return s


def _project(P32, cids, X, noise, rng):
    """(V, 17, 3) rows (y, x, score) of the points X (17, 3) through the float32 P widened to double, plus Gaussian pixel noise."""
    pm = np.zeros((len(cids), J, 3))
    for q, cid in enumerate(cids):
        hm = np.concatenate([X, np.ones((J, 1))], 1) @ P32[cid].astype(np.float64).T
        xy = hm[:, :2] / hm[:, 2:3]
        if noise > 0.0:
            xy = xy + rng.normal(0.0, noise, (J, 2))
        pm[q, :, 0], pm[q, :, 1], pm[q, :, 2] = xy[:, 1], xy[:, 0], rng.uniform(0.7, 0.95, J)
    return pm


def _inputs(idx, family, R, noise, kw):
    rng = np.random.default_rng([20240917, idx])
    C = R['C']
    inside = np.stack([rng.uniform(-2.0, 2.0, J), rng.uniform(-2.0, 2.0, J), rng.uniform(0.0, 2.0, J)], 1)
    if family in ('well', 'outlier'):
        V = int(rng.integers(2, C + 1))
        cids = rng.permutation(C)[:V]
        Ts = rng.integers(0, 4, size=V)
        X = inside
    elif family == 'wide':
        V = kw['V']
        cids = rng.permutation(C)[:V]
        Ts = rng.integers(0, 4, size=V)
        X = inside
    elif family in ('aged', 'mixed', 'table'):
        Ts = np.array(kw['Ts'])
        V = len(Ts)
        cids = rng.permutation(C)[:V]
        X = inside
    elif family == 'far':
        c0 = int(rng.integers(C))
        cids = np.array([c0, (c0 + 1) % C])
        Ts = np.zeros(2, dtype=np.int64)
        fwd = np.stack([R['RT32'][c][2, :3].astype(np.float64) for c in cids]).sum(0)
        fwd /= np.linalg.norm(fwd)
        mid = 0.5 * (R['position'][cids[0]] + R['position'][cids[1]])
        X = mid + kw['far'] * RADIUS * fwd + rng.normal(0.0, 0.2, (J, 3))
    else:                                                             # baseline: the rays of both cameras are the segment itself
        c0 = int(rng.integers(C))
        cids = np.array([c0, (c0 + C // 2) % C])
        Ts = np.zeros(2, dtype=np.int64)
        a, b = R['position'][cids[0]], R['position'][cids[1]]
        t = np.array([kw['t'][j % len(kw['t'])] for j in range(J)])[:, None]
        X = a + t * (b - a)
        V = 2
    V = len(cids)
    pm = _project(R['P32'], cids, X, noise, rng)
    masks = np.zeros(J, dtype=np.uint32)
    for j in range(J):
        k = int(rng.integers(2, V + 1))
        for v in rng.permutation(V)[:k]:
            masks[j] |= np.uint32(1) << np.uint32(v)
    j0, j1 = rng.permutation(J)[:2]
    masks[j0] = 0                                                     # no kept view, one kept view: next_pose is copied
    masks[j1] = np.uint32(1) << np.uint32(rng.integers(V))
    return dict(cids=cids.astype(np.int32), Ts=np.asarray(Ts, dtype=np.int32), pose_mat=pm, masks=masks,
                next_pose=rng.normal(0.0, 1.0, (J, 3)), points=X)


def mask_matrix(masks, V):
    """keep bit masks (17,) -> (mask (17, 2V) 0/1, nviews (17,)) as O.dlt_solve takes them."""
    bits = (np.asarray(masks, dtype=np.uint64)[:, None] >> np.arange(V, dtype=np.uint64)[None, :]) & 1
    return np.repeat(bits.astype(np.int64), 2, axis=1), bits.sum(1).astype(np.int64)


def systems(case, R):
    """-> (A (17, 2V, 4) of O.dlt_rows, mask (17, 2V), nviews (17,))."""
    cs = [R['cams'][int(c)] for c in case['cids']]
    A = O.dlt_rows(cs, case['pose_mat'], [int(t) for t in case['Ts']], LAMBDA_T)
    mask, nviews = mask_matrix(case['masks'], len(cs))
    return A, mask, nviews


def truth(A):
    """(m, 4) float64 -> (X_true (3,), s (4,)) as mpmath numbers at 50 digits."""
    import mpmath
    with mpmath.workdps(50):
        M = mpmath.matrix(A.tolist())
        _, S, Vt = mpmath.svd_r(M, compute_uv=True)
        order = sorted(range(4), key=lambda i: -S[i])
        s = [S[i] for i in order]
        x = [Vt[order[3], c] for c in range(4)]
        return [x[c] / x[3] for c in range(3)], s


def _dd(v):
    """mpmath number -> (hi, lo) doubles with hi + lo = v to ~32 digits."""
    import mpmath
    hi = float(v)
    if not math.isfinite(hi):
        return hi, 0.0
    return hi, float(v - mpmath.mpf(hi))


def generate(with_truth=True):
    """-> dict name -> array: the whole fixture."""
    rigs = {k: rig(k) for k in RIGS}
    out = {'n_cases': np.int64(0)}
    spec = _spec()
    prev = None
    for idx, (family, rname, nsplit, noise, kw) in enumerate(spec):
        R = rigs[rname]
        if kw.get('same_as_previous'):
            case = dict(prev)
        else:
            case = _inputs(idx, family, R, noise, kw)
            A, mask, nviews = systems(case, R)
            Xh, Xl = np.full((J, 3), np.nan), np.zeros((J, 3))
            sh, sl = np.full((J, 4), np.nan), np.zeros((J, 4))
            if with_truth:
                import mpmath
                with mpmath.workdps(50):
                    for j in range(J):
                        if nviews[j] < 2:
                            continue
                        X, s = truth(A[j][mask[j] == 1])
                        for c in range(3):
                            Xh[j, c], Xl[j, c] = _dd(X[c])
                        for c in range(4):
                            sh[j, c], sl[j, c] = _dd(s[c])
            case.update(X_true=Xh, X_true_lo=Xl, s=sh, s_lo=sl)
            prev = case
        k = 'c%02d.' % idx
        out[k + 'family'] = np.array(family); out[k + 'rig'] = np.array(rname)
        out[k + 'nsplit'] = np.int64(nsplit); out[k + 'noise_px'] = np.float64(noise)
        for f in ('cids', 'Ts', 'pose_mat', 'masks', 'next_pose', 'X_true', 'X_true_lo', 's', 's_lo'):
            out[k + f] = case[f]
    out['n_cases'] = np.int64(len(spec))
    for rname, R in rigs.items():
        out[rname + '.P32'] = R['P32']
    return out


INPUTS = ('cids', 'Ts', 'pose_mat', 'masks', 'next_pose')


def load(path=FIXTURE):
    """-> list of case dicts (the fields of the fixture, plus 'index')."""
    z = np.load(path)
    cases = []
    for idx in range(int(z['n_cases'])):
        k = 'c%02d.' % idx
        c = {f[len(k):]: z[f] for f in z.files if f.startswith(k)}
        c.update(index=idx, family=str(c['family']), rig=str(c['rig']), nsplit=int(c['nsplit']), noise_px=float(c['noise_px']))
        cases.append(c)
    return cases, {r: z[r + '.P32'] for r in RIGS}


# ---- the acceptance rules -----------------------------------------------------------------------------------------------------------
def classify(case):
    """Per-joint flags from the stored truth: solved (>= 2 kept views), full (compared in accuracy), rho, noise_free, and the path the
    product rule must report: 0 copied, 1 inverse iteration, 2 Jacobi, -1 either."""
    s = case['s']
    solved = np.array([bin(int(m)).count('1') >= 2 for m in case['masks']])
    with np.errstate(invalid='ignore', divide='ignore'):
        full = solved & (s[:, 2] - s[:, 3] > RANK_GAP * s[:, 0])
        rho = s[:, 3] / s[:, 2]
        noise_free = solved & (s[:, 3] < NOISE_FREE * s[:, 0])
    must = np.full(J, -1)
    must[~solved] = 0
    must[solved & ~noise_free & (rho < RHO_FAST)] = 1
    must[solved & ~noise_free & (rho > RHO_SLOW)] = 2
    return dict(solved=solved, full=full, rho=rho, noise_free=noise_free, must=must)


def error(X, case):
    """max_k |X - X_true| per joint (17,), against the double-double truth."""
    with np.errstate(invalid='ignore'):
        return np.abs((X - case['X_true']) - case['X_true_lo']).max(1)


def amp(case):
    return 1.0 + (case['X_true'] ** 2).sum(1)


def accuracy_ratio(X, X_lapack, case):
    """err(X) / max(err(LAPACK), 32 eps amp) per joint: the accuracy rule is ratio <= M on the joints classify() calls full."""
    with np.errstate(invalid='ignore'):
        return error(X, case) / np.maximum(error(X_lapack, case), FLOOR * EPS * amp(case))


def unweighted_kappa(A, mask):
    """s1 / (s3 - s4) of each joint's rows with the age weights divided out (unit rows) (17,).  The device folds rows in list order, so
    with the fresh view first the Givens QR is row-wise backward stable: every row is perturbed by a few eps of ITS OWN norm, however
    small its weight, and the null vector moves as that of the unweighted rows would.  LAPACK's normwise bound eps s1 / (s3 - s4) is void
    on such graded systems (s3 ~ exp(-45)); this one is not."""
    k = np.full(J, np.nan)
    for j in range(J):
        if mask[j].sum() >= 4:
            B = A[j][mask[j] == 1]
            s = np.linalg.svd(B / np.linalg.norm(B, axis=1)[:, None], compute_uv=False)
            k[j] = s[0] / (s[2] - s[3])
    return k


def first_order_ratio(X, case):
    """err / (eps amp s1 / (s3 - s4)) per joint: the error against the first-order bound of a backward-stable solver."""
    s = case['s']
    with np.errstate(invalid='ignore', divide='ignore'):
        return error(X, case) / (EPS * amp(case) * s[:, 0] / (s[:, 2] - s[:, 3]))


def residual_ratio(X, A, mask, case):
    """(||A x|| - s4) / (eps s1) per joint with x = [X, 1] normalised; the residual rule is ratio <= 8 wherever X is finite."""
    r = np.full(J, np.nan)
    for j in range(J):
        if mask[j].sum() < 4 or not np.isfinite(X[j]).all():
            continue
        x = np.append(X[j], 1.0)
        x /= np.linalg.norm(x)
        r[j] = (np.linalg.norm(A[j][mask[j] == 1] @ x) - case['s'][j, 3]) / (EPS * case['s'][j, 0])
    return r


if __name__ == '__main__':
    fx = generate()
    np.savez_compressed(FIXTURE, **fx)
    print('wrote %s: %d cases, %d bytes' % (FIXTURE, int(fx['n_cases']), os.path.getsize(FIXTURE)))
