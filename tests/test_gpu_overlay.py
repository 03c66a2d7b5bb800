"""The overlay rasteriser on a real MI355X (csrc/pam_overlay.hip through visualization.draw_overlay_device) against the integer
restatement (tests/overlay_ref.py) with array_equal, the frames between sentinel bands: primitives across tile borders (tiles are
64 x 16 pixels) and across all four frame borders, joints outside the frame, eight overlapping persons, three views of different sizes
in one launch, a table longer than one culling pass, and an empty table."""
import numpy as np
import pytest

from pam import _lib
from pam import visualization as V
import guarded_mem as GM
import overlay_ref as R

pytestmark = pytest.mark.gpu
BAND = 2 * GM.GUARD


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class BandedFrame(object):
    """A BGR frame at an odd device address between two bands of `fill`."""

    def __init__(self, torch, frame, fill, shift=1):
        n = frame.size
        self.raw = torch.full((BAND + shift + n + BAND,), fill, dtype=torch.uint8, device='cuda:0')
        self.lo, self.n, self.fill = BAND + shift, n, fill
        self.tensor = self.raw[self.lo:self.lo + n].view(frame.shape)
        self.tensor.copy_(torch.from_numpy(frame))

    def damaged(self):
        return int((self.raw[:self.lo] != self.fill).sum() + (self.raw[self.lo + self.n:] != self.fill).sum())


def background(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def person(w, h, seed, margin=12.0):
    """17 joints scattered over the frame and `margin` pixels beyond every border."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-margin, h + margin, 17), rng.uniform(-margin, w + margin, 17), rng.uniform(0.2, 1.0, 17)], axis=1)


def check(torch, frames, people, threshold=0.0):
    """One launch over all views; every view against the restatement, the bands intact -> the drawn frames."""
    out = []
    for fill in (0xE5, 0x1A):
        banded = [BandedFrame(torch, f, fill, shift=1 + v) for v, f in enumerate(frames)]
        V.draw_overlay_device([b.tensor for b in banded], people, confidence_threshold=threshold)
        torch.cuda.synchronize()
        for v, (b, f) in enumerate(zip(banded, frames)):
            got, want = b.tensor.cpu().numpy(), R.draw(f, people[v], threshold)
            assert b.damaged() == 0, v
            assert np.array_equal(got, want), (v, int((got != want).any(axis=2).sum()))
            out.append(got)
    return out


@pytest.mark.parametrize('size', [(64, 48), (97, 61)])
def test_persons_across_tile_and_frame_borders_equal_the_restatement(torch, size):
    w, h = size
    frame = background(w, h, 1)
    people = [[(person(w, h, 10 + k), k) for k in range(3)]]
    got = check(torch, [frame], people, threshold=0.3)[0]
    changed = (got != frame).any(axis=2)
    assert changed[0].any() and changed[-1].any() and changed[:, 0].any() and changed[:, -1].any()      # all four borders are touched
    assert changed[15:17].all(axis=0).any() and (w <= 64 or changed[:, 63:65].all(axis=1).any())         # and tile borders crossed
    assert 0.05 < changed.mean() < 0.95


def test_joints_far_outside_the_frame_and_undrawable_ones(torch):
    w, h = 97, 61
    p = person(w, h, 3, margin=0.0); p[:, 2] = 1.0
    p[0, :2] = (-300.0, -200.0); p[5, :2] = (30.0, 5000.0); p[6, :2] = (np.nan, 10.0); p[11, :2] = (20.0, 40000.0); p[12, 1] = np.inf
    p[1, :2] = (-1.0, -1.0); p[2, :2] = (61.0, 97.0)                     # discs centred just outside two corners
    check(torch, [background(w, h, 2)], [[(p, 4)]])


def test_eight_overlapping_persons_keep_the_painters_order(torch):
    w, h = 97, 61
    rng = np.random.default_rng(5)
    base = person(w, h, 6, margin=0.0); base[:, 2] = 1.0
    people = [[(base + np.concatenate([rng.uniform(-3, 3, (17, 2)), np.zeros((17, 1))], axis=1), pid) for pid in (3, 1, 4, 1, 5, 9, 2, 6)]]
    frame = background(w, h, 7)
    got = check(torch, [frame], people)[0]
    reverse = R.draw(frame, people[0][::-1])
    assert not np.array_equal(got, reverse)                              # the order matters on this input


def test_three_views_of_different_sizes_in_one_launch(torch):
    sizes = [(64, 48), (97, 61), (200, 150)]
    frames = [background(w, h, 20 + v) for v, (w, h) in enumerate(sizes)]
    people = [[(person(w, h, 30 + 5 * v + k), k) for k in range(2 + v)] for v, (w, h) in enumerate(sizes)]
    people[1] = []                                                       # a view without anybody in the middle
    got = check(torch, frames, people, threshold=0.25)
    assert np.array_equal(got[1], frames[1]) and not np.array_equal(got[2], frames[2])


def test_a_table_longer_than_one_culling_pass(torch):
    w, h = 97, 61
    people = [[(person(w, h, 100 + k, margin=2.0), k) for k in range(20)]]          # up to 720 primitives: two passes of 512
    table, ranges = V.overlay_table(people, [(w, h)])
    assert ranges[0][1] > 512
    check(torch, [background(w, h, 9)], people)


def test_an_empty_table_leaves_the_frame_bit_identical(torch):
    lib = _lib.load()
    frame = background(97, 61, 11)
    nobody = person(97, 61, 12); nobody[:, 2] = 0.0
    for people in ([[]], [[(nobody, 0)]]):
        got = check(torch, [frame], people)
        assert all(np.array_equal(g, frame) for g in got)
    b = BandedFrame(torch, frame, 0x3C)
    view = (_lib.PamOverlayView * 1)()
    view[0].dev_bgr, view[0].width, view[0].height, view[0].prim_first, view[0].prim_count = b.tensor.data_ptr(), 97, 61, 0, 0
    assert lib.pam_overlay_draw(None, 1, view, None, 0) == 0
    torch.cuda.synchronize()
    assert b.damaged() == 0 and np.array_equal(b.tensor.cpu().numpy(), frame)


def test_draw_refuses_what_it_cannot_run_before_any_launch(torch):
    lib = _lib.load()
    frame = torch.zeros((16, 16, 3), dtype=torch.uint8, device='cuda:0')
    prims = torch.zeros((4, 8), dtype=torch.int32, device='cuda:0')

    def call(n=1, table=prims.data_ptr(), n_prims=4, **kw):
        view = (_lib.PamOverlayView * 1)()
        v = dict(dev_bgr=frame.data_ptr(), width=16, height=16, prim_first=0, prim_count=4)
        v.update(kw)
        for k, x in v.items():
            setattr(view[0], k, x)
        return lib.pam_overlay_draw(None, n, view, table, n_prims)

    assert call() == 0
    for kw in (dict(n=0), dict(n=33), dict(dev_bgr=None), dict(width=0), dict(height=65536), dict(prim_first=-1), dict(prim_count=-1),
               dict(prim_first=1), dict(prim_count=5), dict(table=None), dict(table=prims.data_ptr() + 4), dict(n_prims=-1)):
        assert call(**kw) == -1, kw
    assert lib.pam_overlay_draw(None, 1, None, prims.data_ptr(), 4) == -1
    torch.cuda.synchronize()


def test_draw_tracks_device_form_draws_the_reprojected_tracks(torch):
    """draw_tracks(device=True): the tracks' 3D poses re-projected per view (visualization.track_rows), drawn in place by one launch."""
    class Cam(object):
        def __init__(self, P):
            self.P = P

        def projectPoints(self, X):
            x = self.P @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T
            return np.stack([x[1] / x[2], x[0] / x[2]], axis=1)

    class Track(object):
        def __init__(self, tid, X, emitted=True, filtered=None):
            self.track_id, self.pose3d, self.emitted, self.pose3d_filtered = tid, X, emitted, filtered

    rng = np.random.default_rng(2)
    cams = [Cam(np.array([[60.0, 0, 32, 0], [0, 60.0, 24, 0], [0, 0, 1, 0]])), Cam(np.array([[80.0, 0, 48, 5], [0, 80.0, 30, 0], [0, 0, 1, 0.5]]))]
    X = np.concatenate([rng.uniform(-0.4, 0.4, (17, 2)), rng.uniform(1.5, 3.0, (17, 1))], axis=1)
    behind = X.copy(); behind[3, 2] = -2.0
    tracks = [Track(4, X), Track(5, X + 0.1, emitted=False), Track(6, X - 0.2, filtered=behind)]
    frames = [background(64, 48, 40), background(97, 61, 41)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    assert V.draw_tracks(dev, cams, tracks, device=True) is dev
    torch.cuda.synchronize()
    rows = V.track_rows(cams, tracks)
    for v in range(2):
        want = R.draw(frames[v], rows[v])
        assert np.array_equal(dev[v].cpu().numpy(), want) and not np.array_equal(want, frames[v])
