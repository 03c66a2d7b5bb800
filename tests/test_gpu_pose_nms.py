"""pam_pose_nms on the GPU against tests/pose_nms_ref.apply: counts and keep table exact, scores and kept rows bit-equal, the tail
zero, everything beyond untouched.  Every case first asserts on the CPU that no reference OKS lies within 1e-9 of the threshold: the
device's exp may differ from NumPy's in the last bits, so the inputs keep every decision away from them."""
import numpy as np
import pytest
import torch

import pose_nms_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678


def person_box(row):
    """(x, y, w, h) float32 round a (y, x, s) row: 1.25 x the keypoints' bounding box (synth.to_dump_results)."""
    y0, x0, y1, x1 = row[:, 0].min(), row[:, 1].min(), row[:, 0].max(), row[:, 1].max()
    return np.array([x0 - 0.125 * (x1 - x0), y0 - 0.125 * (y1 - y0), 1.25 * (x1 - x0), 1.25 * (y1 - y0)], dtype=np.float32)


def crowd(n, seed, dup=0.4):
    """n rows: strangers (skeletons 400 px apart) and, with probability dup, copies of an earlier row shifted by 0.5 .. 2 px (OKS far
    above 0.9) or 15 px (far below), with joint scores scaled."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if i and rng.uniform() < dup:
            src = rows[int(rng.integers(0, i))]
            rows.append(R.shifted(src, float(rng.choice([0.5, 1.0, 2.0, 15.0])), float(rng.uniform(0.6, 1.0))))
        else:
            s = R.skeleton(seed * 1000 + i)
            s[:, :2] += 400.0 * i
            rows.append(s)
    return np.stack(rows) if rows else np.zeros((0, 17, 3))


def run(view_rows, max_dets, det_slots=None, n_det_in=None, boxes=None, score=None, score_form=None, views=None, pad_rows=0,
        oks_thre=0.9, in_vis_thre=0.2):
    """view_rows: per view (n, 17, 3); boxes: per view (n, 4) float32 (None: person_box); score: per view (n,) float32 (None: NULL);
    score_form: 'table' (V, max_dets) strides (max_dets, 1) | 'list' a detector-layout (G, max_det, 5) list read at + 4; views: the map
    from local view to the list's image (the list then has more images, in another order)."""
    from pam import _lib
    dev = torch.device('cuda:0')
    V = len(view_rows)
    det_slots = det_slots or max_dets
    det = np.full((V, det_slots, 17, 3), SENTINEL)
    for v, rows in enumerate(view_rows):
        det[v, :len(rows)] = rows
    n_in = np.array([len(r) for r in view_rows] if n_det_in is None else n_det_in, dtype=np.int32)
    view_of, slot_of, xywh = [], [], []
    for v, rows in enumerate(view_rows):
        for s in range(len(rows)):
            view_of.append(v); slot_of.append(s)
            xywh.append(person_box(rows[s]) if boxes is None else boxes[v][s])
    for _ in range(pad_rows):                                       # a bucket's spare rows repeat the last real one
        view_of.append(view_of[-1]); slot_of.append(slot_of[-1]); xywh.append(xywh[-1])
    if not view_of:                                                 # the table of a frame without boxes: (view 0, slot 0, the whole frame)
        view_of, slot_of, xywh = [0], [0], [np.array([0, 0, 360, 288], dtype=np.float32)]
    view_of, slot_of = np.array(view_of, dtype=np.int32), np.array(slot_of, dtype=np.int32)
    xywh = np.stack(xywh).astype(np.float32)
    b = t_score = t_views = None
    strides = (0, 0)
    if score is not None:
        b = np.ones((V, max_dets), dtype=np.float32)
        for v, s in enumerate(score):
            b[v, :min(len(s), max_dets)] = s[:max_dets]
        if score_form == 'list':
            G = V + 2 if views is not None else V
            lst = np.full((G, max_dets, 5), -3.0, dtype=np.float32)
            for v in range(V):
                lst[views[v] if views is not None else v, :, 4] = b[v]
            t_list = torch.from_numpy(lst).to(dev)
            t_score, strides = t_list.data_ptr() + 16, (5 * max_dets, 5)
        else:
            tab = b if views is None else np.full((V + 2, max_dets), -3.0, dtype=np.float32)
            if views is not None:
                for v in range(V):
                    tab[views[v]] = b[v]
            t_score, strides = torch.from_numpy(np.ascontiguousarray(tab)).to(dev), (max_dets, 1)
        if views is not None:
            t_views = torch.tensor(views, dtype=torch.int32, device=dev)
    area = R.areas_from_rows(V, max_dets, view_of, slot_of, xywh)
    ref = R.apply(det, n_in, max_dets, area, b, oks_thre, in_vis_thre)
    assert R.threshold_margin(ref['oks'], oks_thre) > 1e-9
    t_det = torch.from_numpy(det).to(dev)
    out = dict(n_det_out=torch.full((V,), -7, dtype=torch.int32, device=dev), keep_from=torch.full((V, max_dets), -7, dtype=torch.int32, device=dev),
               pose_score=torch.full((V, max_dets), -7.0, dtype=torch.float64, device=dev))
    _lib.pose_nms(torch.cuda.current_stream().cuda_stream, t_det, torch.from_numpy(n_in).to(dev), torch.from_numpy(view_of).to(dev),
                  torch.from_numpy(slot_of).to(dev), torch.from_numpy(xywh).to(dev), out['n_det_out'], out['keep_from'], out['pose_score'],
                  max_dets=max_dets, score=t_score, score_strides=strides, views=t_views, oks_thre=oks_thre, in_vis_thre=in_vis_thre)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got['det'] = t_det.cpu().numpy()
    assert got['n_det_out'].tolist() == ref['n_det_out'].tolist()
    assert got['keep_from'].tolist() == ref['keep_from'].tolist()
    assert np.array_equal(got['pose_score'], ref['pose_score'], equal_nan=True)
    for v in range(V):
        n, k = min(max(int(n_in[v]), 0), max_dets), int(ref['n_det_out'][v])
        assert got['det'][v, :k].tobytes() == ref['det'][v, :k].tobytes(), v              # kept rows, bit for bit
        assert not got['det'][v, k:n].any(), v                                           # rows [kept, n) are zero
        assert got['det'][v, n:].tobytes() == det[v, n:].tobytes(), v                    # rows >= n untouched
    return got, ref


@pytest.mark.parametrize('max_dets', [8, 16, 32])
def test_counts_zero_one_two_and_full(max_dets):
    got, ref = run([crowd(0, 1), crowd(1, 2), crowd(2, 3, dup=1.0), crowd(max_dets, 4)], max_dets)
    assert got['n_det_out'][0] == 0 and got['n_det_out'][1] == 1 and 0 < got['n_det_out'][3] < max_dets


def test_device_counts_above_max_dets_and_negative():
    rows = [crowd(8, 5), crowd(8, 6), crowd(3, 7)]
    got, _ = run(rows, 8, n_det_in=[13, -3, 3])
    assert got['n_det_out'][1] == 0 and got['keep_from'][1].tolist() == [-1] * 8


@pytest.mark.parametrize('n_views', [1, 5, 31])
def test_views_with_mixed_counts(n_views):
    counts = np.random.default_rng(n_views).integers(0, 17, n_views).tolist()
    counts[0] = 16
    got, ref = run([crowd(c, 10 + v) for v, c in enumerate(counts)], 16)
    assert int(got['n_det_out'].sum()) < sum(counts)                                     # something was removed


def test_view_records_with_a_count_row_that_must_survive():
    got, _ = run([crowd(8, 20), crowd(5, 21), crowd(0, 22)], 8, det_slots=9)
    assert (got['det'][:, 8] == SENTINEL).all()


def test_slot_zero_killed_every_row_moves_down_one():
    """The compaction stores row s + 1 over row s for every s: a store issued before every lane has read shows as a torn row."""
    rows = crowd(32, 30, dup=0.0)
    rows[0] = R.shifted(rows[5], 1.0, 0.7)
    got, ref = run([rows], 32)
    assert got['keep_from'][0].tolist() == list(range(1, 32)) + [-1]


def test_every_row_a_copy_of_one():
    one = R.skeleton(40)
    got, _ = run([np.stack([one] * 32), np.stack([one] * 3)], 32, score=[np.linspace(0.2, 0.9, 32).astype(np.float32), np.ones(3, np.float32)])
    assert got['n_det_out'].tolist() == [1, 1] and got['keep_from'][0, 0] == 31 and got['keep_from'][1, 0] == 0


def test_hand_cases_chain_equal_scores_unseen_rows_and_zero_areas():
    cases = R.hand_cases()
    names = sorted(cases)
    rows = [cases[k][0][0] for k in names]
    boxes = [np.stack([np.array([0, 0, np.sqrt(a), np.sqrt(a)], dtype=np.float32) for a in cases[k][0][1]]) for k in names]
    score = [cases[k][0][2] for k in names]
    got, ref = run(rows, 8, boxes=boxes, score=score)
    assert got['keep_from'][names.index('chain')].tolist()[:3] == [0, 2, -1]             # not transitive
    assert got['n_det_out'][names.index('zero_area')] == 1                                # 0 / (0 + eps): OKS 1
    # equal scores: three copies with the same score, the lowest slot stays; a stranger with the same score keeps its place
    a = R.skeleton(50)
    far = a.copy(); far[:, :2] += 400.0
    got, _ = run([np.stack([far, a, a.copy(), a.copy()])], 8)
    assert got['keep_from'][0].tolist()[:3] == [0, 1, -1] and got['pose_score'][0, 0] == got['pose_score'][0, 1]
    # a row with every joint below in_vis_thre (score 0.0), one with -inf and NaN joint scores (they fail the comparison)
    dim = R.skeleton(51); dim[:, 2] = 0.1
    odd = R.skeleton(52); odd[:, :2] += 400.0; odd[3, 2] = -np.inf; odd[4, 2] = np.nan
    got, _ = run([np.stack([dim, odd, R.shifted(dim, 1.0)])], 8)
    assert got['pose_score'][0, 0] == 0.0 and got['n_det_out'][0] == 2 and got['pose_score'][0, 1] > 0


@pytest.mark.parametrize('form,mapped', [('table', False), ('table', True), ('list', False), ('list', True)])
def test_box_scores_as_a_strided_grid(form, mapped):
    rng = np.random.default_rng(60)
    rows = [crowd(8, 61, dup=0.6), crowd(6, 62, dup=0.6), crowd(8, 63, dup=0.6)]
    score = [rng.uniform(0.3, 1.0, len(r)).astype(np.float32) for r in rows]
    got, ref = run(rows, 8, score=score, score_form=form, views=[4, 0, 2] if mapped else None)
    plain, _ = run(rows, 8)                                                               # NULL scores: 1.0
    assert got['keep_from'].tolist() != plain['keep_from'].tolist()                       # the scores decided who of a pair stays


def test_crop_rows_padded_with_repeats():
    rows = [crowd(8, 70), crowd(5, 71)]
    a, _ = run(rows, 8, pad_rows=0)
    b, _ = run(rows, 8, pad_rows=7)
    assert a['det'].tobytes() == b['det'].tobytes() and a['keep_from'].tolist() == b['keep_from'].tolist()
