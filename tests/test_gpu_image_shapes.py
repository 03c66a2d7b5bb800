"""GPU: the image-side kernels (csrc/pam_crop.hip, csrc/pam_head.hip) through the C ABI against the float64 restatements of tests/image_ref.py, at the
shapes of every network that ships on them: head channels 32 / 48 / 256 (HRNet-W32, HRNet-W48, PoseResNet), heat-maps 64 x 48 and
96 x 72 plus ragged sizes, crops at 256 x 192 and 384 x 288.  Every output sits between sentinel guard bands; rows of crops that a call
does not cover must keep their sentinel.  Tolerances are the derived ones of image_ref (FMA-chain bound, bf16 half-ulp + coordinate
slack) and the suite's 1e-3-cell figure of the soft decode; each case prints one PARITY line with its worst error / tolerance.

A map with no value above -inf decodes as cell 0 (np.argmax); an antialias window wider than 24 taps keeps the taps nearest the centre;
an antialias box wholly outside the frame reads nothing outside it."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import image_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096                 # elements of guard band on each side of an output
RESOLUTIONS = [(256, 192), (384, 288)]
J = R.J


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib.load()


def parity(test, where, **figures):
    print('PARITY ' + json.dumps(dict(test=test, family='image', where=where, **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in figures.items()})))


SENTINEL = {torch.float32: -7.0, torch.float64: -7.0, torch.bfloat16: -7.0, torch.uint8: 0xA5}


class Guarded(object):
    """`numel` elements between two bands of GUARD sentinel elements; the payload starts as sentinel too."""

    def __init__(self, numel, dtype, dev):
        self.s = SENTINEL[dtype]
        self.buf = torch.full((numel + 2 * GUARD,), self.s, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + numel]

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == self.s).all()) and bool((self.buf[-GUARD:] == self.s).all())

    def untouched(self, t):
        return bool((t == self.s).all())


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def up(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.to(dtype) if dtype is not None else t


def rows_to_index(rows, boxes, h, w):
    """det rows (n, 17, 3) float64 (y, x, score) -> flat cell indices (n, 17): the cell whose box mapping (image_ref.decode64) gives
    exactly that (y, x).  A row that is no cell's image fails here: the box mapping is checked with the arg-max."""
    n = rows.shape[0]
    ytab, _ = R.decode64(np.broadcast_to(np.arange(h), (n, h)), np.zeros((n, 1)), boxes, h, w)
    _, xtab = R.decode64(np.zeros((n, 1)), np.broadcast_to(np.arange(w), (n, w)), boxes, h, w)
    idx = np.empty((n, J), dtype=np.int64)
    for i in range(n):
        for j in range(J):
            py = np.nonzero(ytab[i] == rows[i, j, 0])[0]; px = np.nonzero(xtab[i] == rows[i, j, 1])[0]
            assert py.size == 1 and px.size == 1, ('row is not the image of a cell', i, j, rows[i, j].tolist())
            idx[i, j] = py[0] * w + px[0]
    return idx


class Head(object):
    """Device copies of one head case and the calls on it, every output guarded."""

    def __init__(self, lib, dev, feat, wt, b, boxes):
        self.lib, self.dev = lib, dev
        self.nf, self.h, self.w, self.C = feat.shape
        self.P = self.h * self.w
        self.f = up(feat, dev, torch.bfloat16)                    # (nf, h, w, C): NHWC memory; the values are bf16 already
        assert np.array_equal(self.f.float().cpu().numpy(), feat)
        self.wt, self.b, self.boxes = up(wt, dev), up(b, dev), up(boxes, dev)
        self.view_of = (torch.arange(self.nf, dtype=torch.int32, device=dev) % 3).contiguous()
        self.slot_of = (torch.arange(self.nf, dtype=torch.int32, device=dev) // 3).contiguous()
        self.slots = (self.nf + 2) // 3

    def heatmaps(self):
        out = Guarded(self.nf * self.P * J, torch.float32, self.dev)
        rc = self.lib.pam_head_heatmaps(stream(self.dev), self.nf * self.P, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J, out.ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert out.intact()
        return out.t.reshape(self.nf, self.P, J)

    def decode(self, n, heat=False, beta=None):
        """-> det rows of the first n crops (n, 17, 3) float64 numpy, kp (n, 17, 3), heat (nf, P, 17) or None; the rows, keypoints and
        heat-maps of crops >= n and every guard band must still hold their sentinel."""
        soft = beta is not None
        need = int((self.lib.pam_head_decode_soft_scratch_bytes if soft else self.lib.pam_head_decode_scratch_bytes)(n, self.h, self.w))
        scratch = Guarded(need, torch.uint8, self.dev)
        det = Guarded(3 * self.slots * J * 3, torch.float64, self.dev)
        kp = Guarded(self.nf * J * 3, torch.float32, self.dev)
        hm = Guarded(self.nf * self.P * J, torch.float32, self.dev) if heat else None
        head = (stream(self.dev), n, self.h, self.w, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J)
        tail = (hm.ptr() if heat else None, self.view_of.data_ptr(), self.slot_of.data_ptr(), self.boxes.data_ptr(), self.slots, det.ptr(), kp.ptr(), scratch.ptr())
        rc = self.lib.pam_head_decode_soft(*(head + (C.c_float(beta),) + tail)) if soft else self.lib.pam_head_decode(*(head + tail))
        assert rc == 0
        torch.cuda.synchronize()
        assert scratch.intact() and det.intact() and kp.intact() and (hm is None or hm.intact())
        d = det.t.reshape(3, self.slots, J, 3)
        rows = torch.stack([d[i % 3, i // 3] for i in range(self.nf)])
        assert det.untouched(rows[n:]) and kp.untouched(kp.t.reshape(self.nf, J, 3)[n:])
        spare = 3 * self.slots - self.nf                         # (view, slot) pairs no crop maps to
        assert spare == 0 or det.untouched(torch.stack([d[i % 3, i // 3] for i in range(self.nf, 3 * self.slots)]))
        h3 = hm.t.reshape(self.nf, self.P, J) if heat else None
        assert h3 is None or hm.untouched(h3[n:])
        return rows[:n].cpu().numpy(), kp.t.reshape(self.nf, J, 3)[:n].cpu().numpy(), h3


def check_hard(name, where, rows, kp, heat32, hm64, bound, boxes, h, w):
    """Hard-decode rows against image_ref.argmax_check; the score is the kernel's own float32 heat-map value at the returned cell."""
    n = rows.shape[0]
    idx = rows_to_index(rows, boxes[:n], h, w)
    res = R.argmax_check(hm64[:n], bound[:n], idx)
    assert res['wrong'] == [], (name, where, res['wrong'][:5])
    assert res['undecided'] <= 0.01 * res['maps'], (name, where, res['undecided'])
    want_score = np.take_along_axis(heat32[:n].transpose(0, 2, 1), idx[:, :, None], axis=2)[:, :, 0].astype(np.float64)
    assert np.array_equal(rows[:, :, 2], want_score), (name, where)
    assert np.array_equal(kp[:, :, 0].astype(np.float64), rows[:, :, 1]) and np.array_equal(kp[:, :, 1].astype(np.float64), rows[:, :, 0])
    assert np.array_equal(kp[:, :, 2].astype(np.float64), rows[:, :, 2])
    return idx, res


def check_soft(name, where, rows, kp, heat32, hm64, bound, boxes, h, w, beta, joints=None):
    """Soft-decode rows, two assertions per case.
    (a) Against a float64 softmax of the float32 maps the kernel itself computes: 1e-3 of a heat-map cell (+ 1e-4 px), the suite's
        figure for __expf and the tile merge.
    (b) Against soft64 on the FLOAT64 maps: the same 1e-3 of a cell plus image_ref.soft_slack, the distance soft64 itself can move
        when every value moves by its float32 FMA bound -- the kernel's values differ from the float64 ones by up to that, and beta
        amplifies it (at 256 channels and beta 25 by more than 1e-3 of a cell).
    -> (worst error / tolerance of (b), of (a))."""
    n = rows.shape[0]
    joints = list(range(J)) if joints is None else joints
    b = boxes[:n].astype(np.float64)
    cell_y, cell_x = b[:, 3:4] / h, b[:, 2:3] / w                       # frame pixels per heat-map cell
    sy, sx = R.soft_slack(hm64[:n][:, joints], bound[:n][:, joints], beta, h, w)
    worst = []
    for maps, ky, kx in ((hm64[:n], sy, sx), (heat32[:n].transpose(0, 2, 1).astype(np.float64), 0.0, 0.0)):
        ey, ex, _ = R.soft64(maps[:, joints], beta, h, w)
        wy, wx = ey * cell_y + b[:, 1:2], ex * cell_x + b[:, 0:1]
        tol_y, tol_x = (1e-3 + ky) * cell_y + 1e-4, (1e-3 + kx) * cell_x + 1e-4
        worst.append(float(max((np.abs(rows[:, joints, 0] - wy) / tol_y).max(), (np.abs(rows[:, joints, 1] - wx) / tol_x).max())))
    parity(name, where, beta=beta, soft_ratio=worst[0], soft_ratio_own_maps=worst[1], soft_slack_cells=float(np.max([sy[np.isfinite(sy)].max(initial=0.0), sx[np.isfinite(sx)].max(initial=0.0)])))
    assert worst[1] <= 1.0 and worst[0] <= 1.0, (name, where, beta, worst)
    assert np.array_equal(rows[:, joints, 2], heat32[:n].max(1)[:, joints].astype(np.float64)), (name, where)
    assert np.allclose(kp[:, :, 0], rows[:, :, 1], atol=1e-4) and np.allclose(kp[:, :, 1], rows[:, :, 0], atol=1e-4)
    return worst


HEAD_CASES = [(c, hw, n) for c in R.HEAD_CHANNELS for hw in R.HEAD_MAPS for n in R.HEAD_CROPS]


@pytest.mark.parametrize('C_,hw,n', HEAD_CASES, ids=['C%d-%dx%d-n%d' % (c, hw[0], hw[1], n) for c, hw, n in HEAD_CASES])
def test_head_kernels_vs_fp64(lib, dev, C_, hw, n):
    """pam_head_heatmaps and pam_head_decode with and without heat-maps on seeded random features: every heat-map element within the
    FMA-chain bound of head64, the two kernels' maps bit-identical, keypoints through argmax_check.  At 5 crops the feature batch holds
    7: the rows of crops 5 and 6 stay untouched."""
    h, w = hw
    name = 'head C%d %dx%d n%d' % (C_, h, w, n)
    feat, wt, b, boxes = R.head_case_inputs(C_, h, w, n)
    hm64, bound = R.head64(feat, wt, b)
    hd = Head(lib, dev, feat, wt, b, boxes)
    heat_a = hd.heatmaps()
    a = heat_a.cpu().numpy()                                          # (nf, P, 17)
    ratio = float((np.abs(a.transpose(0, 2, 1).astype(np.float64) - hm64) / bound).max())
    rows, kp, heat_b = hd.decode(n, heat=True)
    assert torch.equal(heat_b[:n], heat_a[:n]), name                 # k_head and k_head_argmax: the same FMA chain, bit for bit
    idx, res = check_hard(name, 'heat', rows, kp, a, hm64, bound, boxes, h, w)
    rows2, kp2, _ = hd.decode(n, heat=False)
    assert np.array_equal(rows2, rows) and np.array_equal(kp2, kp), name
    parity(name, 'hard', fma_ratio=ratio, undecided=res['undecided'], maps=res['maps'])
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize('C_,hw,n', HEAD_CASES, ids=['C%d-%dx%d-n%d' % (c, hw[0], hw[1], n) for c, hw, n in HEAD_CASES])
def test_head_soft_decode_vs_fp64(lib, dev, C_, hw, n):
    """pam_head_decode_soft at beta 0.7 / 4 / 25 on the inputs of test_head_kernels_vs_fp64: positions through check_soft (1e-3 of a
    cell against a float64 softmax of the kernel's own float32 maps; the same plus soft64's own sensitivity against the float64 maps),
    the score and the optional heat-maps bit-identical to pam_head_heatmaps."""
    h, w = hw
    name = 'head C%d %dx%d n%d' % (C_, h, w, n)
    feat, wt, b, boxes = R.head_case_inputs(C_, h, w, n)
    hm64, bound = R.head64(feat, wt, b)
    hd = Head(lib, dev, feat, wt, b, boxes)
    heat_a = hd.heatmaps()
    a = heat_a.cpu().numpy()
    for beta in R.SOFT_BETAS:
        rs, ks, heat_s = hd.decode(n, heat=True, beta=beta)
        assert torch.equal(heat_s[:n], heat_a[:n]), (name, beta)
        check_soft(name, 'soft', rs, ks, a, hm64, bound, boxes, h, w, beta)
        rs2, _, _ = hd.decode(n, heat=False, beta=beta)
        assert np.array_equal(rs2, rs), (name, beta)


SEAM_CASES = [(c, hw) for c in R.HEAD_CHANNELS for hw in R.HEAD_MAPS]


@pytest.mark.parametrize('C_,hw', SEAM_CASES, ids=['C%d-%dx%d' % (c, hw[0], hw[1]) for c, hw in SEAM_CASES])
def test_head_decode_ties_across_tile_seams(lib, dev, C_, hw):
    """Exact ties planted through the features (image_ref.seam_inputs): last pixel of tile t against the first of tile t + 1 for
    t = 0, 7, 15 (the 8-tile groups of k_argmax_finish), tile 0 against the last (ragged) tile, a unique maximum in the last valid
    pixel, a constant map, a map of -3e30 and a map of -inf: the first index wins, an all -inf map decodes as cell 0.  The heat-maps
    the pass writes, decoded again by pam_decode_heatmaps in both layouts, give the same rows."""
    h, w = hw
    name = 'seams C%d %dx%d' % (C_, h, w)
    feat, wt, b, boxes, cases = R.seam_inputs(C_, h, w)
    n = feat.shape[0]
    hm64, bound = R.head64(feat, wt, b)
    hd = Head(lib, dev, feat, wt, b, boxes)
    a = hd.heatmaps().cpu().numpy()
    rows, kp, heat = hd.decode(n, heat=True)
    assert np.array_equal(heat.cpu().numpy(), a, equal_nan=True)
    idx, res = check_hard(name, 'seams', rows, kp, a, hm64, bound, boxes, h, w)
    for crop, what, px in cases:
        assert idx[crop, 5] == px[0], (name, what, int(idx[crop, 5]))
    assert np.all(idx[:, 3] == 0) and np.all(idx[:, 9] == 0), name           # constant maps (their bias; -3e30)
    assert np.all(idx[:, 7] == 0) and np.all(rows[:, 7, 2] == -np.inf), (name, '-inf map', idx[:, 7].tolist())
    assert np.all(rows[:, 3, 2] == np.float64(b[3])) and np.all(rows[:, 9, 2] == np.float64(np.float32(-3.0e30)))
    rows2, kp2, _ = hd.decode(n, heat=False)
    assert np.array_equal(rows2, rows) and np.array_equal(kp2, kp)
    parity(name, 'hard', cases=[c[1] for c in cases], undecided=res['undecided'], maps=res['maps'])
    for nchw in (0, 1):
        src = heat.permute(0, 2, 1).contiguous() if nchw else heat.contiguous()
        det = Guarded(3 * hd.slots * J * 3, torch.float64, dev)
        kpd = Guarded(n * J * 3, torch.float32, dev)
        assert lib.pam_decode_heatmaps(stream(dev), n, src.data_ptr(), nchw, h, w, hd.view_of.data_ptr(), hd.slot_of.data_ptr(),
                                       hd.boxes.data_ptr(), hd.slots, det.ptr(), kpd.ptr()) == 0
        torch.cuda.synchronize()
        assert det.intact() and kpd.intact()
        d = det.t.reshape(3, hd.slots, J, 3)
        got = torch.stack([d[i % 3, i // 3] for i in range(n)]).cpu().numpy()
        assert np.array_equal(got, rows), (name, 'pam_decode_heatmaps nchw=%d' % nchw)
        assert np.array_equal(kpd.t.reshape(n, J, 3).cpu().numpy(), kp)


@pytest.mark.parametrize('C_,hw', SEAM_CASES, ids=['C%d-%dx%d' % (c, hw[0], hw[1]) for c, hw in SEAM_CASES])
def test_head_soft_decode_on_seam_ties(lib, dev, C_, hw):
    """The soft decode on the planted maps of the test above: equal maxima in two different tiles give the mean of the two cells
    (1e-3 of a cell), a constant map the centre of the grid; every joint but the map of -inf through check_soft."""
    h, w = hw
    name = 'seams C%d %dx%d' % (C_, h, w)
    feat, wt, b, boxes, cases = R.seam_inputs(C_, h, w)
    n = feat.shape[0]
    hm64, bound = R.head64(feat, wt, b)
    hd = Head(lib, dev, feat, wt, b, boxes)
    a = hd.heatmaps().cpu().numpy()
    soft_joints = [j for j in range(J) if j != 7]                     # softmax of a map of -inf is not defined
    for beta in R.SOFT_BETAS:
        rs, ks, _ = hd.decode(n, heat=False, beta=beta)
        check_soft(name, 'soft seams', rs, ks, a, hm64, bound, boxes, h, w, beta, joints=soft_joints)
        for crop, what, px in cases:
            bx = boxes[crop].astype(np.float64)
            cy, cx = np.mean([p // w for p in px]), np.mean([p % w for p in px])
            assert abs(rs[crop, 5, 0] - (cy / h * bx[3] + bx[1])) <= 1e-3 * bx[3] / h + 1e-4, (name, what, beta)
            assert abs(rs[crop, 5, 1] - (cx / w * bx[2] + bx[0])) <= 1e-3 * bx[2] / w + 1e-4, (name, what, beta)
        c = boxes[:n].astype(np.float64)                              # constant maps (joint 3: its bias; joint 9: -3e30): the centre
        for j in (3, 9):
            assert np.all(np.abs(rs[:, j, 0] - ((h - 1) / 2.0 / h * c[:, 3] + c[:, 1])) <= 1e-3 * c[:, 3] / h + 1e-4), (name, j, beta)
            assert np.all(np.abs(rs[:, j, 1] - ((w - 1) / 2.0 / w * c[:, 2] + c[:, 0])) <= 1e-3 * c[:, 2] / w + 1e-4), (name, j, beta)


DECODE_CASES = [(hw, layout) for hw in R.DECODE_MAPS for layout in ('nhwc', 'nchw')]


@pytest.mark.parametrize('hw,layout', DECODE_CASES, ids=['%dx%d-%s' % (hw[0], hw[1], l) for hw, l in DECODE_CASES])
def test_decode_heatmaps_ties_across_tiles_and_waves(lib, dev, hw, layout):
    """pam_decode_heatmaps on seeded float32 maps with planted exact ties (image_ref.decode_inputs): across the 1024-pixel tiles of
    k_decode_nhwc, across 64-lane waves, tile 0 against the last tile, the last pixel, constant maps, a map of -inf (cell 0).  The
    values are float32 data, so np.argmax of them is exact and every row must match bit for bit.  41 x 27 has an odd float count per
    crop: crop 1 starts misaligned, a full tile goes down the scalar staging path and an 83-pixel tile follows."""
    h, w = hw
    name = 'decode %dx%d %s' % (h, w, layout)
    hm, boxes, cases = R.decode_inputs(h, w)
    n, P = hm.shape[0], h * w
    src = up(hm if layout == 'nchw' else hm.transpose(0, 2, 1), dev)
    view_of = (torch.arange(n, dtype=torch.int32, device=dev) % 3).contiguous()
    slot_of = (torch.arange(n, dtype=torch.int32, device=dev) // 3).contiguous()
    slots = (n + 2) // 3
    det = Guarded(3 * slots * J * 3, torch.float64, dev)
    kp = Guarded(n * J * 3, torch.float32, dev)
    b_dev = up(boxes, dev)
    assert lib.pam_decode_heatmaps(stream(dev), n, src.data_ptr(), 1 if layout == 'nchw' else 0, h, w, view_of.data_ptr(), slot_of.data_ptr(),
                                   b_dev.data_ptr(), slots, det.ptr(), kp.ptr()) == 0
    torch.cuda.synchronize()
    assert det.intact() and kp.intact()
    d = det.t.reshape(3, slots, J, 3)
    got = torch.stack([d[i % 3, i // 3] for i in range(n)]).cpu().numpy()
    idx = np.argmax(hm.astype(np.float64), axis=2)
    for crop, what, px in cases:
        assert idx[crop, 5] == px[0], what
    y, x = R.decode64(idx // w, idx % w, boxes, h, w)
    want = np.stack([y, x, np.take_along_axis(hm, idx[:, :, None], axis=2)[:, :, 0].astype(np.float64)], axis=2)
    wrong = [(int(i), int(j), got[i, j].tolist(), want[i, j].tolist()) for i, j in zip(*np.nonzero((got != want).any(2)))]
    parity(name, 'hard', cases=[c[1] for c in cases], wrong=len(wrong), maps=n * J)
    assert not wrong, (name, wrong[:5])
    k = kp.t.reshape(n, J, 3).cpu().numpy().astype(np.float64)
    assert np.array_equal(k[:, :, 0], want[:, :, 1]) and np.array_equal(k[:, :, 1], want[:, :, 0]) and np.array_equal(k[:, :, 2], want[:, :, 2])
    spare = 3 * slots - n
    assert spare == 0 or det.untouched(torch.stack([d[i % 3, i // 3] for i in range(n, 3 * slots)]))


# ---- crop kernel ---------------------------------------------------------------------------------------------------------------------
def run_crops(lib, dev, frames, view_of, boxes, res, out_c, n_total, antialias):
    """pam_preprocess_crops_ex into a guarded (n_total, H, W, out_c) bf16 buffer -> float64 numpy (n_total, out_c, H, W)."""
    H, W = res
    n = len(boxes)
    fr = [up(frames[v], dev) for v in range(frames.shape[0])]
    ptrs = torch.tensor([f.data_ptr() for f in fr], dtype=torch.int64, device=dev)
    out = Guarded(n_total * H * W * out_c, torch.bfloat16, dev)
    v_dev, b_dev = up(view_of, dev), up(boxes, dev)               # named: the tables must outlive the launch
    rc = lib.pam_preprocess_crops_ex(stream(dev), n, n_total, ptrs.data_ptr(), frames.shape[1], frames.shape[2], v_dev.data_ptr(),
                                     b_dev.data_ptr(), H, W, out_c, out.ptr(), 1 if antialias else 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.reshape(n_total, H, W, out_c).permute(0, 3, 1, 2).double().cpu().numpy()


def check_crops(lib, dev, case, res, antialias):
    name = '%s -> %dx%d' % ((case[0],) + res)
    frames, view_of, boxes = R.crop_case_inputs(case)
    n = len(boxes)
    val, tol = R.preprocess64(frames, view_of, boxes, res, antialias=antialias)
    got8 = run_crops(lib, dev, frames, view_of, boxes, res, 8, n + 2, antialias)
    got3 = run_crops(lib, dev, frames, view_of, boxes, res, 3, n + 1, antialias)
    assert np.array_equal(got8[:, :3], np.concatenate([got3, got3[-1:]])), name            # the two forms hold the same RGB
    assert not got8[:, 3:].any(), name                                                     # RGB + 5 zero channels
    assert all(np.array_equal(got8[k], got8[n - 1]) for k in range(n, n + 2)), name        # a bucket's spare rows repeat the last crop
    worst, bad = R.crop_check(got8[:n, :3], val, tol)
    per_box = [round(float((np.abs(got8[i, :3] - val[i]) / tol[i]).max()), 4) for i in range(n)]
    parity(name, 'antialias' if antialias else 'bilinear', ratio=worst, out_of_tolerance=bad, per_box=per_box)
    assert bad == 0, (name, worst, per_box)


@pytest.mark.parametrize('case', R.CROP_CASES, ids=[c[0] for c in R.CROP_CASES])
@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_crop_kernel_vs_fp64(lib, dev, case, res):
    """pam_preprocess_crops_ex (plain bilinear) against preprocess64 per pixel: both output sizes, 3- and 8-channel outputs, more output
    rows than boxes, frames down to 4 x 1 pixels and with 3 * W odd (the packed 8-byte row load and its fallback), 1 x 1 boxes, boxes
    wholly outside the frame, boxes ending on the last pixel, fractional boxes."""
    check_crops(lib, dev, case, res, False)


@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_crop_kernel_antialias_vs_fp64(lib, dev, res):
    """The antialias path: integer, fractional and frame-leaving boxes, down-scaling just inside the 11.5 the 24-tap window holds, and
    13 x, where the window is cut to the 24 taps nearest the centre (preprocess64 states that cut; a one-sided cut is out of tolerance
    on these inputs: tests/test_image_ref.py)."""
    for case in R.AA_CASES + [R.aa_limit_case(res), R.aa_limit_case(res, 13.0)]:
        check_crops(lib, dev, case, res, True)


# ---- predict() of the 256 x 192 networks ---------------------------------------------------------------------------------------------
PREDICT_CASES = [(32, 'HRNet', (256, 192), 32), (50, 'PoseResNet', (256, 192), 256), (50, 'PoseResNet', (384, 288), 256)]


@pytest.mark.parametrize('c,model_name,res,channels', PREDICT_CASES, ids=['w32-256x192', 'r50-256x192', 'r50-384x288'])
def test_predict_equals_the_hand_driven_chain(lib, c, model_name, res, channels):
    """As test_gpu_image.test_predict_s3_sized_call_through_the_graph_buckets does for W48: 5 views x 7 persons = 35 crops -> batches of
    20 + 15 (padded to 16), hipGraph replays.  Every crop of the call -- a fortiori a two-crop subset with one crop from the padded
    batch -- equals bit for bit the chain driven by hand on a second, eager network object: crop kernel (the two picked crops within
    preprocess64's tolerance at THIS resolution) -> conv stack -> pam_head_heatmaps, maps of res / 4 -> np.argmax + box mapping.  A
    wrong resolution, map size or head table on predict()'s path cannot pass.

    The hand-driven chain runs the call's own batches (20 crops, then 15 in a 16-crop buffer), not two crops alone: PoseResNet's
    features are bit-exact for a given batch size only (the layer2-4 convolutions choose their tile by the batch's pixel
    count), and on random weights one bf16 ulp moves the arg-max of a near-flat map by tens of pixels."""
    from pam import hrnet, selfcheck
    net = hrnet.HRNetPose(c, 17, None, model_name=model_name, resolution=res, use_graph=True, max_dets=8, graph_bucket=4)
    dev = net.device
    name = 'predict %s-%d %dx%d' % ((model_name, c) + res)
    rng = np.random.default_rng(3)
    fh, fw = 540, 960
    frames_np = rng.integers(0, 256, (5, fh, fw, 3), dtype=np.uint8)
    frames = [torch.from_numpy(frames_np[v]).to(dev) for v in range(5)]
    pbl = []
    for v in range(5):
        persons = []
        for p in range(7):
            w, h = rng.uniform(60, 160), rng.uniform(150, 310)
            x0, y0 = rng.uniform(-15, fw - w + 15), rng.uniform(-15, fh - h + 15)
            persons.append(dict(image_id=0, category_id=1, score=0.9, bbox=[float(x0), float(y0), float(w), float(h)], data=frames[v], feature=[]))
        pbl.append(persons)
    dump = net.predict(pbl, batch_size=20)
    assert [len(d) for d in dump] == [7] * 5 and sorted(k[0] for k in net._graphs) == [16, 20]
    assert dump.device_valid() and tuple(dump.device_det.shape) == (5, 8, 17, 3)
    crops = [(v, p) for v in range(5) for p in range(7)]
    view_np = np.array([v for v, _ in crops], dtype=np.int32)
    boxes_np = np.array([pbl[v][p]['bbox'] for v, p in crops], dtype=np.float32)
    view_of, boxes = torch.from_numpy(view_np).to(dev), torch.from_numpy(boxes_np).to(dev)
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    eager = hrnet.HRNetPose(c, 17, None, model_name=model_name, resolution=res, use_graph=False, max_dets=8)
    assert tuple(eager.head_w.shape) == (17, channels) and torch.equal(eager.head_w, net.head_w) and torch.equal(eager.head_b, net.head_b)
    hh, ww = res[0] // 4, res[1] // 4
    pick = [3, 33]                                                # crop 3 (first batch) and crop 33 (second, padded batch)
    val, tol = R.preprocess64(frames_np, view_np[pick], boxes_np[pick], res)
    want, worst = [], 0.0
    for s, e, rows in ((0, 20, 20), (20, 35, 16)):
        x = eager.input_buffer(rows)
        assert tuple(x.shape) == (rows, 8) + res
        eager.preprocess(ptrs, fh, fw, view_of[s:e].contiguous(), boxes[s:e].contiguous(), x)
        with torch.no_grad():
            hm = eager.heatmaps(x)                                # pam_head_heatmaps
            f = eager.features(x)
            hm_replay = net.heatmaps(x).clone()                   # the replaying object's own heat-maps of the same batch
        torch.cuda.synchronize()
        assert tuple(hm.shape) == (rows, 17, hh, ww) and tuple(f.shape) == (rows, channels, hh, ww)
        assert torch.equal(hm_replay, hm)
        for k, i in enumerate(pick):
            if s <= i < e:
                r, bad = R.crop_check(x[i - s:i - s + 1, :3].double().cpu().numpy(), val[k:k + 1], tol[k:k + 1])
                assert bad == 0 and not bool(x[:, 3:].any()), (name, i, r)
                worst = max(worst, r)
        m = hm[:e - s].permute(0, 2, 3, 1).reshape(e - s, hh * ww, 17).cpu().numpy().transpose(0, 2, 1)      # (crops, 17, P) float32
        idx = np.argmax(m.astype(np.float64), axis=2)
        y, xx = R.decode64(idx // ww, idx % ww, boxes_np[s:e], hh, ww)
        rows_ = np.stack([y, xx, np.take_along_axis(m, idx[:, :, None], axis=2)[:, :, 0].astype(np.float64)], axis=2)     # (y, x, score)
        ref = selfcheck.reference_decode(hm[:e - s], boxes[s:e]).cpu().numpy()
        diff = np.argwhere((ref != rows_).any(2))
        assert diff.size == 0, (name, [(int(i), int(j), ref[i, j].tolist(), rows_[i, j].tolist(), int((m[i, j] == m[i, j].max()).sum())) for i, j in diff[:4]])
        want.append(rows_)
    want = np.concatenate(want)
    for i, (v, p) in enumerate(crops):
        kp = np.asarray(dump[v][p]['keypoints']).reshape(17, 3)   # (x, y, score)
        got = np.stack([kp[:, 1], kp[:, 0], kp[:, 2]], axis=1)
        assert np.array_equal(got, want[i]), (name, i, np.abs(got - want[i]).max())
        assert np.array_equal(dump.device_det[v, p].cpu().numpy(), want[i])
        assert np.array_equal(np.asarray(dump[v][p]['keypoints_score']), kp[:, 2])
    parity(name, 'predict', crop_ratio=worst, crops_equal=len(crops))
