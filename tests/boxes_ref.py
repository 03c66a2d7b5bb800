"""Float64 NumPy restatements of the two box rules of include/pam.h: pam_track_boxes (person boxes from the tracker state) and
pam_crop_table (detector-layout box lists -> crop table), plus the gate the closed-loop tests put between the detections and the tracker.
Shared by the CPU and the GPU tests; nothing here touches a device."""
import numpy as np

J = 17
RULE = dict(grow=1.25, pad_px=8.0, min_size_px=8.0, max_gap=3)


def predict_pose(pose3d, velocity, gap):
    """k_frame's P4a expression: a float32 product, added in double."""
    step = np.asarray(velocity).astype(np.float32) * np.float32(gap)
    return np.asarray(pose3d, dtype=np.float64) + step.astype(np.float64)


def project(P, X):
    """P (3, 4) float32, X (17, 3) float64 -> u, v, h2 (17,) float64, the sums taken left to right as project_point takes them."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    h = [P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1] + P[r, 2] * X[:, 2] + P[r, 3] for r in range(3)]
    ih = 1.0 / h[2]
    return h[0] * ih, h[1] * ih, h[2]


def track_boxes(P, tracks, frame_id, frame_w, frame_h, max_det, grow=1.25, pad_px=8.0, min_size_px=8.0, max_gap=3):
    """P (C, 3, 4) float32; tracks: list, in list order, of dicts with pose3d (17, 3), velocity (17, 3), last_time, track_id.
    -> dict(boxes (C, max_det, 5) float32, count (2C,) int32, ids (C, max_det) int32, info (2,) int32, margin = the smallest distance of
    any in-front or drop decision from its threshold, boxes64 = per view the unrounded [x1, y1, x2, y2, track_id] rows before the
    max_det clamp)."""
    C = len(P)
    boxes = np.zeros((C, max_det, 5), dtype=np.float32)
    ids = np.full((C, max_det), -1, dtype=np.int32)
    count = np.zeros(2 * C, dtype=np.int32)
    info = np.zeros(2, dtype=np.int32)
    margin = np.inf
    rows64 = [[] for _ in range(C)]
    grow, pad_px, min_size_px = float(np.float32(grow)), float(np.float32(pad_px)), float(np.float32(min_size_px))
    for tr in tracks:
        gap = int(frame_id) - int(tr['last_time'])
        if not 0 <= gap <= max_gap:
            continue
        info[1] += 1
        X = predict_pose(tr['pose3d'], tr['velocity'], gap)
        for v in range(C):
            x, y, h2 = project(P[v], X)
            margin = min(margin, float(np.abs(h2).min()))
            if not np.all(h2 > 0):
                continue
            cx, cy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
            hx, hy = 0.5 * grow * (x.max() - x.min()) + pad_px, 0.5 * grow * (y.max() - y.min()) + pad_px
            x1, y1 = max(cx - hx, 0.0), max(cy - hy, 0.0)
            x2, y2 = min(cx + hx, float(frame_w)), min(cy + hy, float(frame_h))
            margin = min(margin, abs((x2 - x1) - min_size_px), abs((y2 - y1) - min_size_px))
            if x2 - x1 < min_size_px or y2 - y1 < min_size_px:
                continue
            n = int(count[C + v])
            if n < max_det:
                boxes[v, n] = (x1, y1, x2, y2, 1.0)
                ids[v, n] = tr['track_id']
            rows64[v].append([x1, y1, x2, y2, tr['track_id']])
            count[C + v] = n + 1
    count[:C] = np.minimum(count[C:], max_det)
    info[0] = 1 if np.any(count[C:] > max_det) else 0
    return dict(boxes=boxes, count=count, ids=ids, info=info, margin=margin,
                boxes64=[np.array(r, dtype=np.float64).reshape(-1, 5) for r in rows64])


def xywh_row(row, frame_w, frame_h):
    """One detector row -> (x, y, w, h) float32: clamp, subtract in double, round once."""
    a, b, c, d = (float(row[0]), float(row[1]), float(row[2]), float(row[3]))
    x1, y1 = (a if a > 0 else 0.0), (b if b > 0 else 0.0)
    x2, y2 = (float(frame_w) if frame_w < c else c), (float(frame_h) if frame_h < d else d)
    return np.array([x1, y1, x2 - x1, y2 - y1], dtype=np.float64).astype(np.float32)


def crop_table(boxes, count, frame_w, frame_h, max_dets, cap, views=None, n_views=None):
    """boxes (G, max_det_in, 5) float32, count (>= G,) -> dict(view_of, slot_of (cap,) int32, xywh (cap, 4) float32, n_det (n_views,)
    int32, info (4,) int32) as pam_crop_table writes them."""
    boxes = np.asarray(boxes, dtype=np.float32)
    src = list(range(n_views if n_views is not None else boxes.shape[0])) if views is None else [int(g) for g in views]
    max_det_in = boxes.shape[1]
    bits, rows, n_det, wanted = 0, [], [], 0
    for i, g in enumerate(src):
        raw = int(count[g])
        k = min(min(max(raw, 0), max_det_in), max_dets)
        if k != raw:
            bits |= 1
        wanted += k
        k = min(k, cap - len(rows))
        n_det.append(k)
        rows += [(i, s, xywh_row(boxes[g, s], frame_w, frame_h)) for s in range(k)]
    if wanted > cap:
        bits |= 2
    total = len(rows)
    pad = rows[-1] if rows else (0, 0, np.array([0.0, 0.0, float(frame_w), float(frame_h)], dtype=np.float32))
    rows += [pad] * (cap - total)
    return dict(view_of=np.array([r[0] for r in rows], dtype=np.int32), slot_of=np.array([r[1] for r in rows], dtype=np.int32),
                xywh=np.stack([r[2] for r in rows]).astype(np.float32), n_det=np.array(n_det, dtype=np.int32),
                info=np.array([total, wanted, bits, 0], dtype=np.int32))


def gate_detections(dets_xy, boxes, min_inside=15):
    """The closed loop's gate for one view: dets_xy (n, 17, 3) rows (x, y, score), boxes (k, >= 4) rows (x1, y1, x2, y2).  Every box
    takes, among the detections with at least min_inside keypoints inside it, the one whose keypoint centre is nearest the box's centre;
    -> the sorted indices of the detections taken (their original order)."""
    taken = set()
    for b in boxes:
        best, best_d = -1, np.inf
        for k, d in enumerate(dets_xy):
            inside = (d[:, 0] >= b[0]) & (d[:, 0] <= b[2]) & (d[:, 1] >= b[1]) & (d[:, 1] <= b[3])
            if int(inside.sum()) < min_inside:
                continue
            cx, cy = 0.5 * (d[:, 0].min() + d[:, 0].max()), 0.5 * (d[:, 1].min() + d[:, 1].max())
            dist = np.hypot(cx - 0.5 * (b[0] + b[2]), cy - 0.5 * (b[1] + b[3]))
            if dist < best_d:
                best, best_d = k, dist
        if best >= 0:
            taken.add(best)
    return sorted(taken)


def oracle_tracks(tracker):
    """The oracle tracker's list (oracle.cpu_ref.Tracker.tracks) in the form track_boxes takes."""
    return [dict(pose3d=t.hist[-1], velocity=t.velocity, last_time=t.hist_t[-1], track_id=t.track_id) for t in tracker.tracks]
