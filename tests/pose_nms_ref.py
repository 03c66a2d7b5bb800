"""Float64 restatement of pam_pose_nms (include/pam.h): the rescoring + greedy OKS-NMS of the HRNet / Simple Baselines test protocol
(TEST.OKS_THRE / TEST.IN_VIS_THRE), per view, on the tracker's (y, x, score) rows.  NumPy only; shares no code with the kernel."""
import numpy as np

SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
VARS = (SIGMAS * 2) ** 2
EPS = 2.220446049250313e-16          # np.spacing(1)
J = 17


def rescore(rows, b, in_vis_thre):
    """rows (n, 17, 3) (y, x, s), b (n,) box scores -> (n,) float64: b * mean of the joint scores above in_vis_thre (0 when none is),
    summed in joint order."""
    out = np.zeros(len(rows))
    for i in range(len(rows)):
        tot, cnt = np.float64(0.0), 0
        for j in range(J):
            s = np.float64(rows[i, j, 2])
            if s > in_vis_thre:
                tot = tot + s
                cnt += 1
        mean = tot / np.float64(cnt) if cnt else np.float64(0.0)
        with np.errstate(invalid='ignore'):
            out[i] = np.float64(b[i]) * mean
    return out


def oks_matrix(rows, area, oks_vars=VARS):
    """(n, n) OKS of every pair: all 17 joints, no visibility mask."""
    n = len(rows)
    out = np.zeros((n, n))
    with np.errstate(all='ignore'):
        for p in range(n):
            for q in range(n):
                dx = rows[p, :, 1] - rows[q, :, 1]
                dy = rows[p, :, 0] - rows[q, :, 0]
                e = (dx * dx + dy * dy) / oks_vars / ((area[p] + area[q]) / 2.0 + EPS) / 2.0
                ex, acc = np.exp(-e), np.float64(0.0)
                for j in range(J):
                    acc = acc + ex[j]
                out[p, q] = acc / np.float64(J)
    return out


def order_of(score):
    """Descending score, equal scores by lower slot; a NaN score goes last."""
    key = np.where(np.isnan(score), -np.inf, score)
    return sorted(range(len(score)), key=lambda i: (-key[i], i))


def nms_view(rows, area, b, oks_thre=0.9, in_vis_thre=0.2, oks_vars=VARS):
    """One view.  -> dict(keep = kept slots ascending, score (n,), oks (n, n))."""
    n = len(rows)
    score = rescore(rows, b, in_vis_thre)
    oks = oks_matrix(rows, area, oks_vars)
    alive = np.ones(n, dtype=bool)
    keep = []
    for i in order_of(score):
        if not alive[i]:
            continue
        keep.append(i)
        alive[i] = False
        with np.errstate(invalid='ignore'):
            alive &= ~(oks[i] > oks_thre)              # (NaN > t is False: a NaN OKS kills nothing)
    return dict(keep=sorted(keep), score=score, oks=oks)


def areas_from_rows(n_views, max_dets, view_of, slot_of, xywh):
    """(V, max_dets) float64 crop areas (double)w * (double)h from the crop rows (float32 boxes); 0 where no row names the slot."""
    area = np.zeros((n_views, max_dets))
    xywh = np.asarray(xywh, dtype=np.float32).reshape(-1, 4)
    for r in range(len(view_of)):
        v, s = int(view_of[r]), int(slot_of[r])
        if 0 <= v < n_views and 0 <= s < max_dets:
            area[v, s] = np.float64(xywh[r, 2]) * np.float64(xywh[r, 3])
    return area


def apply(det, n_det_in, max_dets, area, b=None, oks_thre=0.9, in_vis_thre=0.2, oks_vars=VARS):
    """det (V, det_slots, 17, 3) float64, n_det_in (V,), area (V, max_dets), b (V, max_dets) float32 box scores or None (1.0) ->
    dict(det (a filtered copy), n_det_out (V,) int32, keep_from (V, max_dets) int32, pose_score (V, max_dets) float64, oks: per view
    the (n, n) matrix)."""
    det = np.array(det, dtype=np.float64)
    V = det.shape[0]
    n_out = np.zeros(V, dtype=np.int32)
    keep_from = np.full((V, max_dets), -1, dtype=np.int32)
    pose_score = np.zeros((V, max_dets))
    oks = []
    for v in range(V):
        n = min(max(int(n_det_in[v]), 0), max_dets)
        rows = det[v, :n].copy()
        bb = np.ones(n, dtype=np.float32) if b is None else np.asarray(b, dtype=np.float32)[v, :n]
        r = nms_view(rows, area[v, :n], bb, oks_thre, in_vis_thre, oks_vars)
        k = len(r['keep'])
        det[v, :k] = rows[r['keep']]
        det[v, k:n] = 0.0
        n_out[v] = k
        keep_from[v, :k] = r['keep']
        pose_score[v, :k] = r['score'][r['keep']]
        oks.append(r['oks'])
    return dict(det=det, n_det_out=n_out, keep_from=keep_from, pose_score=pose_score, oks=oks)


def threshold_margin(oks_list, oks_thre):
    """Smallest |oks - oks_thre| over every off-diagonal pair of every view (inf when there is no pair; NaN entries do not count)."""
    best = np.inf
    for m in oks_list:
        n = len(m)
        if n > 1:
            d = np.abs(m - oks_thre)[~np.eye(n, dtype=bool)]
            d = d[~np.isnan(d)]
            if len(d):
                best = min(best, float(d.min()))
    return best


# ---- hand-built cases (tests/test_pose_nms_ref.py, tests/test_gpu_pose_nms.py) ------------------------------------------------------------
def skeleton(seed=0, size=100.0):
    rng = np.random.default_rng(seed)
    rows = np.zeros((17, 3))
    rows[:, :2] = rng.uniform(0.1 * size, 0.9 * size, (17, 2))
    rows[:, 2] = rng.uniform(0.5, 0.95, 17)
    return rows


def shifted(row, dx, scale=1.0):
    out = row.copy()
    out[:, 1] += dx
    out[:, 2] *= scale
    return out


def hand_cases():
    """name -> (rows (n, 17, 3) (y, x, s), area (n,), b (n,) float32), the variant each one is built to expose"""
    a = skeleton(1)
    far = skeleton(2); far[:, :2] += 400.0
    big = np.full(3, 100.0 * 100.0)
    cases = {}
    # A kills B, B would kill C, A does not: greedy keeps A and C
    cases['chain'] = (np.stack([a, shifted(a, 3.0, 0.9), shifted(a, 6.0, 0.8)]), big, np.ones(3, np.float32)), 'transitive'
    # a duplicate pair whose better-scored copy sits in the HIGHER slot, behind a stranger
    cases['late_best'] = (np.stack([shifted(a, 1.0, 0.9), far, a]), big, np.ones(3, np.float32)), 'slot_order'
    # equal box scores, the joint scores decide who of the pair stays
    cases['rescored'] = (np.stack([shifted(a, 1.0, 0.7), a]), big[:2], np.ones(2, np.float32)), 'unrescored'
    # two people whose confident joints coincide and whose unsure joints (below in_vis_thre) lie far apart: all 17 count, so no kill
    p, q = a.copy(), a.copy()
    p[9:, 2], q[9:, 2] = 0.1, 0.05
    q[9:, 1] += 60.0
    cases['unsure_joints'] = (np.stack([p, q]), big[:2], np.ones(2, np.float32)), 'vis_mask'
    # the same row twice with zero-area boxes: 0 / (0 + eps) = 0, OKS 1; without the epsilon 0 / 0
    cases['zero_area'] = (np.stack([a, a.copy()]), np.zeros(2), np.array([1.0, 0.5], np.float32)), 'no_eps'
    # two strangers, the better one in slot 1: both stay, in SLOT order
    cases['strangers'] = (np.stack([shifted(a, 0.0, 0.8), far]), big[:2], np.ones(2, np.float32)), 'score_order_out'
    return cases
