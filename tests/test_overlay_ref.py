"""tests/overlay_ref.py, the integer rasteriser of the device overlay restated (no GPU): its pixel sets against brute force and
against the shapes they must be, the painter's order, what drops out of a table, and visualization.overlay_table -- the table the
device is given -- against the restatement's own."""
import numpy as np

import overlay_ref as R
from pam import visualization as V


def pose(x=20.0, y=20.0, c=1.0):
    """17 joints on one point."""
    return np.tile(np.array([y, x, c], dtype=np.float64), (17, 1))


def spread(w, h, seed, c=1.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-5, h + 5, 17), rng.uniform(-5, w + 5, 17), np.full(17, c)], axis=1)


def covered(prim, w, h):
    y0, x0, m = R.mask(prim, w, h)
    out = np.zeros((h, w), dtype=bool)
    out[y0:y0 + m.shape[0], x0:x0 + m.shape[1]] = m
    return out


def test_a_disc_is_the_brute_force_pixel_set():
    for (cx, cy, r) in ((20.0, 15.0, 2), (20.3, 15.7, 3), (0.0, 0.0, 4), (39.5, 29.5, 5), (-1.0, 12.0, 2)):
        qx, qy = R.quantise(cx), R.quantise(cy)
        prim = (qx, qy, qx, qy, 8 * r, (1, 2, 3))
        want = np.array([[(8 * x - qx) ** 2 + (8 * y - qy) ** 2 <= 64 * r * r for x in range(40)] for y in range(30)])
        assert np.array_equal(covered(prim, 40, 30), want)
        assert np.array_equal(want, np.array([[R.inside(prim, x, y) for x in range(40)] for y in range(30)]))
        assert want.any()


def test_an_axis_aligned_limb_is_a_rectangle_plus_two_caps():
    w, h, hw = 60, 40, 12                                                # half-width 1.5 pixels
    a, b = (8 * 10, 8 * 20), (8 * 40, 8 * 20)
    got = covered((a[0], a[1], b[0], b[1], hw, (0, 0, 0)), w, h)
    want = np.zeros((h, w), dtype=bool)
    want[19:22, 10:41] = True                                            # |y - 20| <= 1.5 between the end points
    for ex in (10, 40):
        for y in range(h):
            for x in range(w):
                if (8 * (x - ex)) ** 2 + (8 * (y - 20)) ** 2 <= hw * hw:
                    want[y, x] = True
    assert np.array_equal(got, want)
    assert got[20, 9] and got[20, 41] and not got[20, 8] and not got[18, 25]      # caps reach one pixel past the ends
    vert = covered((a[1], a[0], b[1], b[0], hw, (0, 0, 0)), h, w)                 # the transposed limb
    assert np.array_equal(vert, want.T)


def test_numpy_masks_equal_python_ints_on_slanted_limbs():
    rng = np.random.default_rng(3)
    for _ in range(12):
        ax, ay, bx, by = [int(v) for v in rng.integers(-80, 480, 4)]
        prim = (ax, ay, bx, by, int(rng.integers(1, 40)), (0, 0, 0))
        want = np.array([[R.inside(prim, x, y) for x in range(50)] for y in range(50)])
        assert np.array_equal(covered(prim, 50, 50), want)


def test_a_zero_length_limb_is_a_disc_of_the_half_width():
    w, h = 300, 300                                                      # radius 2, width 2: half-width 8 eighths = one pixel
    p = pose(20.0, 20.0)
    prims = R.primitives([(p, 0)], w, h)
    assert len(prims) == 19 + 17 and all(q[:2] == q[2:4] for q in prims)
    assert {q[4] for q in prims[:19]} == {8} and {q[4] for q in prims[19:]} == {16}
    limb = covered(prims[0], w, h)
    assert limb.sum() == 5 and limb[20, 20] and limb[19, 20] and limb[20, 21] and not limb[19, 19]


def test_style_follows_the_frame_size():
    assert R.style(1032, 776) == (5, 3) and R.style(360, 288) == (2, 2) and R.style(64, 48) == (2, 2) and R.style(1920, 1080) == (7, 4)
    assert R.style(1032, 776) == V.overlay_style(1032, 776) and R.style(97, 61) == V.overlay_style(97, 61)


def test_painters_order_between_two_overlapping_persons():
    w, h = 64, 48
    a = pose(); a[:, 1] = np.linspace(10, 50, 17); a[:, 0] = 20.0        # along a row: joint 8 at (30, 20)
    b = pose(); b[:, 1] = 30.0; b[:, 0] = np.linspace(5, 40, 17)         # down a column: joint 7 at (30, 20.3)
    frame = np.full((h, w, 3), 9, dtype=np.uint8)
    ab, ba = R.draw(frame, [(a, 0), (b, 1)]), R.draw(frame, [(b, 1), (a, 0)])
    joint = lambda j: tuple(int(c) for c in V._palette('gist_rainbow', 17)[j][::-1])
    limb = lambda pid: tuple(int(c) for c in V._palette('tab20', 8)[pid][::-1])
    assert tuple(ab[20, 30]) == joint(7) and tuple(ba[20, 30]) == joint(8)        # the crossing: the person drawn last shows
    only_a, only_b = R.draw(frame, [(a, 0)]), R.draw(frame, [(b, 1)])
    hit_a, hit_b = (only_a != 9).any(axis=2), (only_b != 9).any(axis=2)
    assert (hit_a & hit_b).sum() > 9
    assert np.array_equal(ab[hit_b], only_b[hit_b]) and np.array_equal(ab[hit_a & ~hit_b], only_a[hit_a & ~hit_b])
    assert np.array_equal(ba[hit_a], only_a[hit_a]) and np.array_equal(ba[hit_b & ~hit_a], only_b[hit_b & ~hit_a])
    assert (ab[~(hit_a | hit_b)] == 9).all()
    # within one person the joints lie over the limbs: shoulder and elbow alone, 30 pixels apart
    c = pose(c=0.0); c[5] = (20.0, 10.0, 1.0); c[7] = (20.0, 40.0, 1.0)
    got = R.draw(frame, [(c, 2)])
    assert tuple(got[20, 10]) == joint(5) and tuple(got[20, 40]) == joint(7) and tuple(got[20, 25]) == limb(2)
    assert tuple(got[20, 12]) == joint(5) and tuple(got[20, 13]) == limb(2) and tuple(got[18, 25]) == (9, 9, 9)
    assert (frame == 9).all()                                            # the input is left alone


def test_nan_off_range_and_low_confidence_joints_drop_out_with_their_limbs():
    w, h = 64, 48
    p = spread(w, h, 1)
    full = R.primitives([(p, 0)], w, h)
    assert len(full) == 36
    for bad in (np.nan, np.inf, -np.inf, 40000.0, -32768.2):
        q = p.copy(); q[5, 1] = bad                                      # the left shoulder: limbs 5-11, 5-6, 5-7, 0-5
        got = R.primitives([(q, 0)], w, h)
        assert len(got) == 36 - 4 - 1, bad
        assert got == [x for k, x in enumerate(full) if k not in (5, 7, 8, 17, 19 + 5)]
    q = p.copy(); q[5, 2] = 0.3
    assert len(R.primitives([(q, 0)], w, h, threshold=0.3)) == 31        # the confidence must be ABOVE the threshold
    assert len(R.primitives([(q, 0)], w, h, threshold=0.29)) == 36
    assert R.quantise(32768.0) == 1 << 18 and R.quantise(32768.1) is None and R.quantise(-32768.0) == -(1 << 18)
    assert R.quantise(0.0624) == 0 and R.quantise(0.0625) == 1 and R.quantise(-0.0625) == 0 and R.quantise(-0.07) == -1


def test_an_empty_table_leaves_the_frame_alone():
    frame = np.random.default_rng(0).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    assert np.array_equal(R.draw(frame, []), frame)
    assert np.array_equal(R.draw(frame, [(pose(c=0.0), 0)]), frame)
    assert np.array_equal(R.draw(frame, [(pose(x=-500.0, y=-500.0), 0)]), frame)       # drawable, but covers no pixel


def test_overlay_table_is_the_restatements_table():
    sizes = [(64, 48), (97, 61), (1032, 776)]
    people = [[(spread(w, h, 10 * v + k), k + 5) for k in range(3)] for v, (w, h) in enumerate(sizes)]
    people[1][1][0][3, 0] = np.nan
    people[2][0][0][:, 2] = np.linspace(0, 1, 17)
    table, ranges = V.overlay_table(people, sizes, confidence_threshold=0.25)
    assert table.dtype == np.int32 and table.shape[1] == 8 and ranges[0][0] == 0
    for (first, count), ppl, (w, h) in zip(ranges, people, sizes):
        want = R.primitives(ppl, w, h, threshold=0.25)
        got = [tuple(int(x) for x in row[:5]) + ((int(row[5]) & 255, (int(row[5]) >> 8) & 255, (int(row[5]) >> 16) & 255),)
               for row in table[first:first + count]]
        assert got == want
    assert sum(c for _, c in ranges) == len(table)
    empty, ranges = V.overlay_table([[], []], sizes[:2])
    assert empty.shape == (0, 8) and ranges == [(0, 0), (0, 0)]


def test_track_rows_are_the_rows_draw_tracks_draws():
    """visualization.track_rows (what draw_tracks(device=True) hands the device) against the host draw_tracks: drawing the rows per view
    with draw_points_and_skeleton gives draw_tracks' images; joints behind a camera carry confidence 0, tracks not emitted are left out."""
    class Cam(object):
        def __init__(self, P):
            self.P = P

        def projectPoints(self, X):
            x = self.P @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T
            return np.stack([x[1] / x[2], x[0] / x[2]], axis=1)           # rows (y, x)

    class Track(object):
        def __init__(self, tid, X, emitted=True, filtered=None):
            self.track_id, self.pose3d, self.emitted, self.pose3d_filtered = tid, X, emitted, filtered

    rng = np.random.default_rng(2)
    cams = [Cam(np.array([[60.0, 0, 32, 0], [0, 60.0, 24, 0], [0, 0, 1, 0]])), Cam(np.array([[50.0, 0, 30, 5], [0, 50.0, 20, 0], [0, 0, 1, 0.5]]))]
    X = np.concatenate([rng.uniform(-0.4, 0.4, (17, 2)), rng.uniform(1.5, 3.0, (17, 1))], axis=1)
    behind = X.copy(); behind[3, 2] = -2.0
    tracks = [Track(4, X), Track(5, X + 0.1, emitted=False), Track(6, X - 0.2, filtered=behind)]
    rows = V.track_rows(cams, tracks)
    assert [len(r) for r in rows] == [2, 2] and [pid for _, pid in rows[0]] == [4, 6]
    assert rows[0][1][0][3, 2] == 0.0 and rows[0][1][0][2, 2] == 1.0 and rows[0][0][0][:, 2].all()
    frames = [np.zeros((48, 64, 3), dtype=np.uint8), np.zeros((48, 64, 3), dtype=np.uint8)]
    want = V.draw_tracks(frames, cams, tracks)
    for v in range(2):
        im = frames[v]
        for r, pid in rows[v]:
            im = V.draw_points_and_skeleton(im, r, V.joints_dict()['coco']['skeleton'], person_index=pid, points_color_palette='gist_rainbow',
                                            skeleton_color_palette='tab20', points_palette_samples=17, confidence_threshold=0.0)
        assert np.array_equal(im, want[v]) and im.any()
