"""The lens model of include/pam.h on the host, in NumPy float64: Brown-Conrady in the OpenCV / Panoptic order (k1, k2, p1, p2, k3) on
normalised coordinates, K upper-triangular with skew.  The expressions are the ones csrc/pam_lens.hpp evaluates on the device (there
without fused multiply-adds), the inverse is the same 8 Newton steps from the distorted point.

A camera is a row of 10 doubles (``_lib.lens_table``): fx, fy, cx, cy, skew, k1, k2, p1, p2, k3.  Not in the reference: its
Camera.undistort_points is an identity stub (/root/reference/src/ivclabpose.py:55-60)."""
import numpy as np

from ._lib import LENS_ITERS, LENS_TOL


def normalise(row, u, w):
    """pixels (u = column, w = row) -> normalised (x, y)"""
    y = (w - row[3]) / row[1]
    x = (u - row[2] - row[4] * y) / row[0]
    return x, y


def pixels(row, x, y):
    return row[0] * x + row[4] * y + row[2], row[1] * y + row[3]


def forward(row, x, y):
    """ideal normalised (x, y) -> distorted (xd, yd), closed form"""
    k1, k2, p1, p2, k3 = row[5:10]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y


def inverse(row, dx, dy, iters=LENS_ITERS):
    """distorted normalised (dx, dy) -> (x, y, ok): Newton with the analytic Jacobian from the distorted point, always `iters` steps;
    ok is False where an iterate's determinant was not > 0 or the final residual exceeds LENS_TOL in either coordinate."""
    k1, k2, p1, p2, k3 = row[5:10]
    dx, dy = np.asarray(dx, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    x, y = dx.copy(), dy.copy()
    ok = np.ones(dx.shape, dtype=bool)
    with np.errstate(all='ignore'):
        for _ in range(iters):
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            drad = k1 + r2 * (2.0 * k2 + 3.0 * r2 * k3)
            ex = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - dx
            ey = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - dy
            a = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
            b = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
            d = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
            det = a * d - b * b
            ok &= det > 0.0
            x, y = x - (d * ex - b * ey) / det, y - (a * ey - b * ex) / det
        fx, fy = forward(row, x, y)
        ok &= (np.abs(fx - dx) <= LENS_TOL) & (np.abs(fy - dy) <= LENS_TOL)
    return x, y, ok


def is_pinhole(row):
    return not np.any(np.asarray(row[5:10]) != 0.0)


def undistort_uw(row, u, w):
    """raw-image pixels -> ideal pixels; a point that is not finite or cannot be inverted keeps its coordinates.  -> (u, w, ok)"""
    u, w = np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if is_pinhole(row):
        return u.copy(), w.copy(), np.ones(u.shape, dtype=bool)
    with np.errstate(all='ignore'):
        dx, dy = normalise(row, u, w)
        x, y, ok = inverse(row, dx, dy)
        ok &= np.isfinite(u) & np.isfinite(w)
        uu, ww = pixels(row, x, y)
    return np.where(ok, uu, u), np.where(ok, ww, w), ok


def distort_uw(row, u, w):
    """ideal pixels -> raw-image pixels"""
    u, w = np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if is_pinhole(row):
        return u.copy(), w.copy()
    x, y = normalise(row, u, w)
    xd, yd = forward(row, x, y)
    return pixels(row, xd, yd)


def undistort_rows(row, yxs):
    """(n, 17, 3) rows (y, x, score) of one camera -> a copy with (y, x) undistorted, the scores as they were"""
    out = np.array(yxs, dtype=np.float64, copy=True)
    if out.size:
        out[..., 1], out[..., 0], _ = undistort_uw(row, out[..., 1], out[..., 0])
    return out
