"""pam_overlay_tracks restated from the text of include/pam.h in NumPy scalars and Python ints (a plain helper, imported like
overlay_ref.py; no GPU, no library): tracks in list order -> the fixed-layout primitive table of every view, the per-view counts, and
``margin``, the smallest distance of any ``8 v + 0.5`` it floored from an integer (a comparison with the device is only meaningful
while no coordinate sits on a rounding boundary).  It shares no code with csrc/pam_overlay_tracks.hip or pam.visualization; only the
COCO limb list and the two colour tables (data) come from there, as in overlay_ref.py.

A track is a dict(track_id, pose3d (17, 3) float64, emitted); a view is a dict(P (3, 4), w, h, lens=None | 10 doubles (fx, fy, cx, cy,
skew, k1, k2, p1, p2, k3))."""
import math

import numpy as np

from pam import visualization as V
import overlay_ref as R

ROWS = 36                    # rows of one track in one view: 19 limbs + 17 joints
COORD_MAX = 1 << 18
NULL_ROW = (0, 0, 0, 0, -1, 0, 0, 0)


def palette():
    """25 words B | G << 8 | R << 16: the 8 limb colours, then the 17 joint colours."""
    word = lambda c: int(c[2]) | (int(c[1]) << 8) | (int(c[0]) << 16)
    return [word(c) for c in V._palette('tab20', 8)] + [word(c) for c in V._palette('gist_rainbow', 17)]


def style(w, h):
    """-> (8 * radius, 4 * limb width): the half-widths of a joint and of a limb in 1/8 pixel."""
    radius = max(2, int(round(min(w, h) / 150.0)))            # Python rounds ties to even
    return 8 * radius, 4 * (radius // 2 + 1)


def lens_forward_pixels(L, u, w):
    """(u, w) of the ideal image -> the raw image: normalise, forward, pixels of include/pam.h, in that order of operations."""
    fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 = [float(x) for x in L]
    y = (w - cy) / fy
    x = (u - cx - skew * y) / fx
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + skew * yd + cx, fy * yd + cy


class Margin(object):
    def __init__(self):
        self.value = float('inf')

    def floor(self, v):
        t = 8.0 * v + 0.5
        q = math.floor(t)
        if abs(q) <= COORD_MAX + 1:                  # beyond that the coordinate drops out whichever way it rounds
            self.value = min(self.value, t - q, q + 1 - t)
        return q


def joint(P, X, lens, margin):
    """-> (qx, qy) in 1/8 pixel, or None when the joint cannot be drawn."""
    p = [float(np.float32(x)) for x in np.asarray(P).reshape(12)]
    X0, X1, X2 = float(X[0]), float(X[1]), float(X[2])
    h0 = p[0] * X0 + p[1] * X1 + p[2] * X2 + p[3]
    h1 = p[4] * X0 + p[5] * X1 + p[6] * X2 + p[7]
    h2 = p[8] * X0 + p[9] * X1 + p[10] * X2 + p[11]
    if not h2 > 0.0:
        return None
    ih = 1.0 / h2
    u, w = h0 * ih, h1 * ih
    if lens is not None and any(float(c) != 0.0 for c in lens[5:10]):
        u, w = lens_forward_pixels(lens, u, w)
    if not (math.isfinite(u) and math.isfinite(w)) or not (math.isfinite(8.0 * u + 0.5) and math.isfinite(8.0 * w + 0.5)):
        return None
    qx, qy = margin.floor(u), margin.floor(w)
    return (qx, qy) if abs(qx) <= COORD_MAX and abs(qy) <= COORD_MAX else None


def table(tracks, views, cap, emitted_only=True, colours=None):
    """-> dict(prims (n_views, cap, 8) int32 -- the colour word's bits in an int32, as the device tensor holds them --, count (n_views,)
    int32, margin)."""
    colours = palette() if colours is None else colours
    limbs = V.joints_dict()['coco']['skeleton']
    margin = Margin()
    prims = np.empty((len(views), cap, 8), dtype=np.int64)
    prims[:] = NULL_ROW
    count = np.zeros(len(views), dtype=np.int32)
    for v, view in enumerate(views):
        joint_hw, limb_hw = style(view['w'], view['h'])
        rows = []
        for tr in tracks:
            if emitted_only and not tr['emitted']:
                continue
            q = [joint(view['P'], X, view.get('lens'), margin) for X in np.asarray(tr['pose3d'], dtype=np.float64).reshape(17, 3)]
            for a, b in limbs:
                if q[a] is not None and q[b] is not None:
                    rows.append((q[a][0], q[a][1], q[b][0], q[b][1], limb_hw, colours[int(tr['track_id']) % 8], 0, 0))
            for j in range(17):
                if q[j] is not None:
                    rows.append((q[j][0], q[j][1], q[j][0], q[j][1], joint_hw, colours[8 + j], 0, 0))
        assert len(rows) <= cap
        if rows:
            prims[v, :len(rows)] = rows
        count[v] = len(rows)
    return dict(prims=(prims & 0xFFFFFFFF).astype(np.uint32).view(np.int32), count=count, margin=margin.value)


def paint(frame, rows, count):
    """The first ``count`` rows of one view's range painted into a copy of the BGR frame by overlay_ref's rasteriser."""
    prims = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]),
              (int(r[5]) & 255, (int(r[5]) >> 8) & 255, (int(r[5]) >> 16) & 255)) for r in np.asarray(rows)[:int(count)]]
    return R.paint(frame, prims)
