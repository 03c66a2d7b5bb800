"""The overlay rasteriser of include/pam.h restated in NumPy and Python ints (a plain helper, imported like image_ref.py; no GPU, no
library).  ``primitives`` builds a view's table from the lists the host drawing takes -- per person the limbs, then the joints --
and ``draw`` paints it: the last primitive of the table that covers a pixel gives it its colour, a pixel none covers keeps its value.
It shares no code with csrc/pam_overlay.hip or visualization.overlay_table; only the two colour tables (data) and the COCO limb list
come from pam.visualization."""
import math

import numpy as np

from pam import visualization as V

COORD_MAX = 1 << 18


def style(w, h):
    """-> (joint radius, limb width) in pixels"""
    radius = max(2, int(round(min(w, h) / 150.0)))
    return radius, max(1, radius // 2 + 1)


def quantise(v):
    """A coordinate in 1/8 pixel, None when it cannot be drawn."""
    v = float(v)
    if not math.isfinite(v):
        return None
    q = math.floor(8.0 * v + 0.5)
    return q if abs(q) <= COORD_MAX else None


def primitives(people, w, h, threshold=0.0, skeleton=None):
    """people: [(rows (17, 3) of (y, x, confidence), person_index)] -> [(ax, ay, bx, by, hw, (b, g, r))] in painter's order."""
    skeleton = V.joints_dict()['coco']['skeleton'] if skeleton is None else skeleton
    radius, width = style(w, h)
    limb_colours, joint_colours = V._palette('tab20', 8), V._palette('gist_rainbow', 17)
    out = []
    for rows, pid in people:
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        q = []
        for y, x, c in rows:
            qx, qy = quantise(x), quantise(y)
            q.append((qx, qy) if (c > threshold and qx is not None and qy is not None) else None)
        r, g, b = limb_colours[int(pid) % len(limb_colours)]
        for i, j in skeleton:
            if q[i] is not None and q[j] is not None:
                out.append((q[i][0], q[i][1], q[j][0], q[j][1], 4 * width, (b, g, r)))
        for j, at in enumerate(q):
            if at is not None:
                r, g, b = joint_colours[j % len(joint_colours)]
                out.append((at[0], at[1], at[0], at[1], 8 * radius, (b, g, r)))
    return out


def inside(prim, px, py):
    """Python ints throughout: is pixel (px, py) inside the capsule?"""
    ax, ay, bx, by, hw = [int(v) for v in prim[:5]]
    X, Y = 8 * int(px), 8 * int(py)
    dx, dy, qx, qy = bx - ax, by - ay, X - ax, Y - ay
    dd, t = dx * dx + dy * dy, qx * dx + qy * dy
    if t <= 0:
        return qx * qx + qy * qy <= hw * hw
    if t >= dd:
        return (X - bx) ** 2 + (Y - by) ** 2 <= hw * hw
    cr = qx * dy - qy * dx
    return abs(cr) < (1 << 31) and cr * cr <= hw * hw * dd


def mask(prim, w, h):
    """-> (y0, x0, bool array): the pixels of the w x h frame the capsule covers, over its bounding box clipped to the frame (int64)."""
    ax, ay, bx, by, hw = [int(v) for v in prim[:5]]
    x0, x1 = max(0, (min(ax, bx) - hw) // 8), min(w - 1, (max(ax, bx) + hw) // 8 + 1)
    y0, y1 = max(0, (min(ay, by) - hw) // 8), min(h - 1, (max(ay, by) + hw) // 8 + 1)
    if x1 < x0 or y1 < y0:
        return 0, 0, np.zeros((0, 0), dtype=bool)
    Y, X = np.meshgrid(8 * np.arange(y0, y1 + 1, dtype=np.int64), 8 * np.arange(x0, x1 + 1, dtype=np.int64), indexing='ij')
    dx, dy, qx, qy = bx - ax, by - ay, X - ax, Y - ay
    dd, t = dx * dx + dy * dy, qx * dx + qy * dy
    cr = qx * dy - qy * dx
    side = (np.abs(cr) < (1 << 31)) & (np.where(np.abs(cr) < (1 << 31), cr, 0) ** 2 <= hw * hw * dd)
    m = np.where(t <= 0, qx * qx + qy * qy <= hw * hw, np.where(t >= dd, (X - bx) ** 2 + (Y - by) ** 2 <= hw * hw, side))
    return y0, x0, m


def paint(frame, prims):
    """A new frame with the table painted in order."""
    out = np.array(frame, copy=True)
    h, w = out.shape[:2]
    for p in prims:
        y0, x0, m = mask(p, w, h)
        if m.size:
            out[y0:y0 + m.shape[0], x0:x0 + m.shape[1]][m] = p[5]
    return out


def draw(frame, people, threshold=0.0):
    """BGR uint8 (H, W, 3), the view's people -> the frame with their skeletons drawn."""
    return paint(frame, primitives(people, frame.shape[1], frame.shape[0], threshold))
