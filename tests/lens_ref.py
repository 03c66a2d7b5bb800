"""A float64 NumPy restatement of the lens model of include/pam.h -- Brown-Conrady, OpenCV / Panoptic order (k1, k2, p1, p2, k3) on
normalised coordinates, K = (fx, fy, cx, cy, skew) -- written from the model's definition and sharing no code with pam.lens, Camera or
the kernel; the coefficient sets, grids and the synthetic trace that the CPU and the GPU tests of the lens step share.  A plain module
(not a conftest.py); nothing here touches a device.

Truth is by construction: ideal points go through the closed-form forward model, the inverse must give them back.  The forward model
itself is pinned by ``forward_mp``, the same closed form at 50 digits (mpmath, as tests/dlt_ref.py pins its SVD).

Points are rows (x, y) in pixels, x the column.  ``fault`` plants one of FAULTS into the function it is given to."""
import numpy as np

# name: K5 = (fx, fy, cx, cy, skew), frame (w, h), dist = (k1, k2, p1, p2, k3)
SETS = {
    'hd': dict(k=(1395.0, 1392.0, 951.0, 561.0, 0.0), wh=(1920, 1080), dist=(-0.286, 0.195, -0.0004, 0.0006, 0.018)),
    'vga': dict(k=(745.0, 745.0, 375.0, 226.0, 0.0), wh=(640, 480), dist=(-0.325, 0.05, -0.0008, 0.0011, 0.11)),
    'barrel': dict(k=(600.0, 600.0, 640.0, 360.0, 0.0), wh=(1280, 720), dist=(-0.35, 0.15, 0.001, -0.001, -0.03)),
    'pincushion': dict(k=(1000.0, 1000.0, 640.0, 360.0, 0.0), wh=(1280, 720), dist=(0.12, 0.05, 0.002, 0.001, 0.0)),
}
ORDER = ('hd', 'vga', 'barrel', 'pincushion')
ITERS = 8
TOL_PX = 1e-9                # the round trip's bound, pixels (about 1000 x the float64 floor of the four sets)
RESID = 1e-9                 # largest final residual of a point that counts as inverted, normalised units
MIN_DET = 0.2                # grid points: Jacobian determinant of the forward model at the ideal point
FAULTS = ('swap_p', 'no_k3', 'swap_xy', 'iters2')


def lens_row(name):
    """The 10 doubles of a set as the device table holds them."""
    s = SETS[name]
    return np.array(s['k'] + s['dist'], dtype=np.float64)


def to_norm(k, xy):
    fx, fy, cx, cy, skew = k
    xy = np.asarray(xy, dtype=np.float64)
    yn = (xy[..., 1] - cy) / fy
    return np.stack([(xy[..., 0] - cx - skew * yn) / fx, yn], axis=-1)


def to_px(k, n):
    fx, fy, cx, cy, skew = k
    return np.stack([fx * n[..., 0] + skew * n[..., 1] + cx, fy * n[..., 1] + cy], axis=-1)


def _coef(dist, fault):
    k1, k2, p1, p2, k3 = [float(v) for v in dist]
    if fault == 'swap_p':
        p1, p2 = p2, p1
    if fault == 'no_k3':
        k3 = 0.0
    return k1, k2, p1, p2, k3


def forward(dist, n, fault=None):
    """ideal normalised (.., 2) -> distorted normalised (.., 2)"""
    k1, k2, p1, p2, k3 = _coef(dist, fault)
    x, y = n[..., 0], n[..., 1]
    r2 = x ** 2 + y ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    tx = 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
    ty = p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    return np.stack([x * radial + tx, y * radial + ty], axis=-1)


def jacobian(dist, n, fault=None):
    """-> (.., 2, 2): d(xd, yd) / d(x, y)"""
    k1, k2, p1, p2, k3 = _coef(dist, fault)
    x, y = n[..., 0], n[..., 1]
    r2 = x ** 2 + y ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    slope = k1 + 2 * k2 * r2 + 3 * k3 * r2 ** 2               # d radial / d r2
    Jm = np.empty(n.shape[:-1] + (2, 2))
    Jm[..., 0, 0] = radial + 2 * x ** 2 * slope + 2 * p1 * y + 6 * p2 * x
    Jm[..., 0, 1] = 2 * x * y * slope + 2 * p1 * x + 2 * p2 * y
    Jm[..., 1, 0] = Jm[..., 0, 1]
    Jm[..., 1, 1] = radial + 2 * y ** 2 * slope + 6 * p1 * y + 2 * p2 * x
    return Jm


def det2(Jm):
    return Jm[..., 0, 0] * Jm[..., 1, 1] - Jm[..., 0, 1] * Jm[..., 1, 0]


def inverse(dist, d, iters=ITERS, fault=None):
    """distorted normalised (.., 2) -> (ideal normalised (.., 2), ok (..)): Newton from the distorted point, `iters` steps whatever
    happens; ok is False where an iterate's determinant was not > 0 or the residual after the last step exceeds RESID."""
    if fault == 'iters2':
        iters = 2
    d = np.asarray(d, dtype=np.float64)
    n = d.copy()
    ok = np.ones(d.shape[:-1], dtype=bool)
    with np.errstate(all='ignore'):
        for _ in range(iters):
            e = forward(dist, n, fault) - d
            Jm = jacobian(dist, n, fault)
            dt = det2(Jm)
            ok &= dt > 0
            step = np.stack([Jm[..., 1, 1] * e[..., 0] - Jm[..., 0, 1] * e[..., 1],
                             Jm[..., 0, 0] * e[..., 1] - Jm[..., 1, 0] * e[..., 0]], axis=-1) / dt[..., None]
            n = n - step
        ok &= np.all(np.abs(forward(dist, n, fault) - d) <= RESID, axis=-1)
    return n, ok


def distort_px(k, dist, xy, fault=None):
    """ideal pixels (.., 2) -> raw-image pixels (.., 2)"""
    return to_px(k, forward(dist, to_norm(k, xy), fault))


def undistort_px(k, dist, xy, fault=None):
    """raw-image pixels (.., 2) -> (ideal pixels (.., 2), ok): a point that is not finite or cannot be inverted keeps its coordinates"""
    xy = np.asarray(xy, dtype=np.float64)
    if fault == 'swap_xy':
        xy = xy[..., ::-1]
    if not np.any(np.asarray(dist, dtype=np.float64) != 0):
        return xy.copy(), np.ones(xy.shape[:-1], dtype=bool)
    with np.errstate(all='ignore'):
        n, ok = inverse(dist, to_norm(k, xy), fault=fault)
        ok &= np.all(np.isfinite(xy), axis=-1)
        out = to_px(k, n)
    return np.where(ok[..., None], out, xy), ok


def grid(name, step=None, reach=0.6):
    """Ideal pixels (N, 2) of a set on a regular grid (about 60 steps across the frame) that reaches `reach` frame sizes beyond the frame:
    those whose distorted image lies in the frame plus 10 % and whose Jacobian determinant is >= MIN_DET (there and on the way there)."""
    s = SETS[name]
    w, h = s['wh']
    step = step or w / 60.0
    xs = np.arange(-reach * w, (1 + reach) * w + step, step)
    ys = np.arange(-reach * h, (1 + reach) * h + step, step)
    pts = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    n = to_norm(s['k'], pts)
    raw = to_px(s['k'], forward(s['dist'], n))
    inside = (raw[:, 0] >= -0.1 * w) & (raw[:, 0] <= 1.1 * w) & (raw[:, 1] >= -0.1 * h) & (raw[:, 1] <= 1.1 * h)
    # the model folds where the determinant reaches 0; beyond the fold ideal points far outside land inside the frame again, and further
    # out the determinant is positive once more (both of its factors have changed sign).  Those are not points of the lens: the
    # determinant has to hold on the whole segment from the principal point's ray to the point.
    near = np.ones(len(pts), dtype=bool)
    for t in np.linspace(0.0, 1.0, 33)[1:]:
        near &= det2(jacobian(s['dist'], t * n)) >= MIN_DET
    return pts[inside & near]


def forward_mp(dist, x, y, digits=50):
    """The forward model of one normalised point at `digits` digits -> (xd, yd) mpmath numbers (the doubles are taken exactly)."""
    import mpmath
    with mpmath.workdps(digits):
        k1, k2, p1, p2, k3 = [mpmath.mpf(float(v)) for v in dist]
        x, y = mpmath.mpf(float(x)), mpmath.mpf(float(y))
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        return (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)


def forward_bound(dist, x, y):
    """A bound on the float64 forward model's distance from forward_mp, per coordinate: every term of the closed form is a product of at
    most 9 factors and the sums have at most 6 terms, so each coordinate carries at most 16 roundings, each relative to the sum of the
    terms' MAGNITUDES (the running-error bound of a polynomial): 16 * 2^-53 / (1 - 16 * 2^-53) * that sum; doubled for margin on the
    bound itself, not on the result."""
    k1, k2, p1, p2, k3 = [abs(float(v)) for v in dist]
    ax, ay = abs(x), abs(y)
    r2 = ax * ax + ay * ay
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    mx = ax * rad + 2 * p1 * ax * ay + p2 * (r2 + 2 * ax * ax)
    my = ay * rad + p1 * (r2 + 2 * ay * ay) + 2 * p2 * ax * ay
    return 32 * 2.0 ** -53 * mx, 32 * 2.0 ** -53 * my


# ---- the synthetic trace the GPU pipeline tests run: an S1 scene (3 cameras) whose keypoints are pushed through the VGA-like lens on the
# rig's own K.  The seed is chosen so that the CPU oracle makes the same decisions on the undistorted rows as on the ideal ones on every
# frame (test_lens_ref.py checks it): a condition on the input, not a tolerance.
TRACE = dict(size='S1', n_frames=20, seed=3, occlusion_every=5, empty_view_every=7, birth_death_frame=6)
TRACE_DIST = SETS['vga']['dist']


def trace():
    """-> dict(seq, K5 (C, 5), dist (C, 5), lens (C, 10), ideal, raw): ideal / raw = per frame per view (n, 17, 3) rows (x, y, score), raw
    the ideal rows pushed through the forward model in float64."""
    from pam import synth
    seq = synth.make_sequence(TRACE['size'], **{k: v for k, v in TRACE.items() if k != 'size'})
    K = np.asarray(seq['calib']['K']).astype(np.float32).astype(np.float64)          # the float32 K the product holds
    K5 = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 0, 1]], axis=1)
    dist = np.tile(np.asarray(TRACE_DIST, dtype=np.float64), (len(K), 1))
    raw = []
    for views in seq['frames']:
        out = []
        for c, d in enumerate(views):
            r = np.array(d, dtype=np.float64, copy=True)
            if len(r):
                r[..., :2] = distort_px(K5[c], dist[c], r[..., :2])
            out.append(r)
        raw.append(out)
    return dict(seq=seq, K5=K5, dist=dist, lens=np.concatenate([K5, dist], axis=1), ideal=seq['frames'], raw=raw)


def undistort_views(K5, dist, views):
    """per view (n, 17, 3) rows (x, y, score), raw -> ideal (a copy)"""
    out = []
    for c, d in enumerate(views):
        r = np.array(d, dtype=np.float64, copy=True)
        if len(r):
            r[..., :2], _ = undistort_px(K5[c], dist[c], r[..., :2])
        out.append(r)
    return out
