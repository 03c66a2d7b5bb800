"""GPU: the DARK decode (pam_head_decode_dark) through the C ABI against the float64 restatement of tests/dark_ref.py, then through
HRNetPose.predict.  Every output sits between guard bands; rows a call does not cover keep their sentinel; every case prints a PARITY
line.  The inputs, their derived bounds and the share of undecided cases are those tests/test_dark_ref.py checks on the CPU, and the
check applied to the kernel's positions (dark_ref.judge) is the one that rejects the wrong decoders there."""
import json

import numpy as np
import pytest
import torch

import dark_ref as D
import image_ref as R
from test_gpu_flip import FlipHead, _net_case, _pbl, bits, rows_to_cells, NET_BOXES
from test_gpu_image_shapes import Guarded, stream

pytestmark = pytest.mark.gpu

J = R.J


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib.load()


def parity(test, where, **figures):
    print('PARITY ' + json.dumps(dict(test=test, family='dark', where=where, **{k: (round(v, 7) if isinstance(v, float) else v) for k, v in figures.items()})))


class DarkHead(FlipHead):
    """FlipHead (device copies of one case: rows [0, n) plain, [n, 2n) mirrored, one spare; guarded outputs) with the new entry point."""

    def dark(self, flags, k, heat=False):
        """-> det rows (n, 17, 3) float64, kp (n, 17, 3), heat (n, P, 17) or None."""
        n = self.n
        need = int(self.lib.pam_head_decode_dark_scratch_bytes(n, self.h, self.w))
        assert need == int(self.lib.pam_head_decode_scratch_bytes(n, self.h, self.w))
        scratch = Guarded(need, torch.uint8, self.dev)
        det = Guarded(3 * self.slots * J * 3, torch.float64, self.dev)
        kp = Guarded(self.rows * J * 3, torch.float32, self.dev)
        hm = Guarded(self.rows * self.P * J, torch.float32, self.dev) if heat else None
        rc = self.lib.pam_head_decode_dark(stream(self.dev), n, n, self.h, self.w, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J,
                                           flags, k, hm.ptr() if heat else None, self.view_of.data_ptr(), self.slot_of.data_ptr(),
                                           self.boxes.data_ptr(), self.slots, det.ptr(), kp.ptr(), scratch.ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert scratch.intact() and det.intact() and kp.intact() and (hm is None or hm.intact())
        d = det.t.reshape(3, self.slots, J, 3)
        rows = torch.stack([d[i % 3, i // 3] for i in range(3 * self.slots)])
        assert det.untouched(rows[n:]) and kp.untouched(kp.t.reshape(self.rows, J, 3)[n:])
        h3 = hm.t.reshape(self.rows, self.P, J) if heat else None
        assert h3 is None or hm.untouched(h3[n:])
        return rows[:n].cpu().numpy(), kp.t.reshape(self.rows, J, 3)[:n].cpu().numpy(), (h3[:n].cpu().numpy() if heat else None)


def cells_of(rows, boxes, h, w):
    """det rows (y, x, score) -> positions in cells (py, px) and the float32 rounding of the box mapping in cells (half a float32 ulp of
    the stored coordinate, through the inverse of image_ref.decode64's scale)."""
    b = np.asarray(boxes, dtype=np.float64)
    py = (rows[:, :, 0] - b[:, 1:2]) / b[:, 3:4] * h
    px = (rows[:, :, 1] - b[:, 0:1]) / b[:, 2:3] * w
    with np.errstate(invalid='ignore'):                                # (1e-9 cell: the float64 roundings of this inversion itself)
        return py, px, 0.5 * R.ulp32(rows[:, :, 0]) * h / b[:, 3:4] + 1e-9, 0.5 * R.ulp32(rows[:, :, 1]) * w / b[:, 2:3] + 1e-9


def check_dark(name, where, hd, flags, k, M, bd, boxes, cap=True):
    """One pam_head_decode_dark call against pam_head_decode_flip with the same merge flags and against dark64 on the float64 map:
    * cell and score exactly as pam_head_decode_flip returns them (the score's bits; outside the inside rule the whole row's bits),
      the cell accepted by image_ref.argmax_check;
    * decided positions within their derived bound plus the float32 rounding of the box mapping, undecided ones within the widest
      answer the derivation allows (dark_ref.judge), undecided inside cases (arg-max included) at most 1 % (cap=False, the planted
      crops: their other joints' maps carry no blob and are mostly undecided; the caller asserts the planted joint's case instead);
    * kp = the det rows in float32 (x, y, score); nothing read from the spare feature row (it holds 1e30: every finite map's row is finite);
    * the heat output bit-equal to pam_head_decode_flip's, and the keypoints the same with and without it.
    -> idx, result of dark64."""
    n, h, w = hd.n, hd.h, hd.w
    frows, fkp, fheat, _ = hd.decode(flags, heat=True)
    rows, kp, _ = hd.dark(flags, k)
    rows2, kp2, heat = hd.dark(flags, k, heat=True)
    assert rows.tobytes() == rows2.tobytes() and kp.tobytes() == kp2.tobytes(), (name, where, 'the heat-map pointer changed the keypoints')
    assert np.array_equal(bits(heat), bits(fheat)), (name, where, 'heat output differs from pam_head_decode_flip')
    idx, oy0, ox0 = rows_to_cells(frows, boxes[:n], h, w)
    assert not oy0.any() and not ox0.any()
    flatM, flatB = M.reshape(n, J, -1), bd.reshape(n, J, -1)
    am = R.argmax_check(flatM, flatB, idx)
    assert am['wrong'] == [], (name, where, am['wrong'][:5])
    assert np.array_equal(bits(rows[:, :, 2]), bits(frows[:, :, 2])), (name, where, 'score bits')
    res = D.dark64(M, bd, idx, k)
    ins = res['inside']
    assert rows[~ins].tobytes() == frows[~ins].tobytes(), (name, where, 'a winner outside the inside rule moved')
    py, px, sy, sx = cells_of(rows, boxes[:n], h, w)
    fin = np.isfinite(flatM.max(2))
    assert np.isfinite(rows[fin]).all(), (name, where, 'non-finite keypoint of a finite map')
    verdict = D.judge(py, px, idx, res, w, sy, sx)
    assert verdict['wrong'] == [], (name, where, verdict['wrong'][:5])
    undecided = ins & ~(res['decided'] & D.argmax_decided(M, bd))
    assert not cap or undecided.sum() <= 0.01 * ins.sum(), (name, where, int(undecided.sum()), int(ins.sum()))
    assert np.array_equal(kp[:, :, 0].astype(np.float64), rows[:, :, 1]) and np.array_equal(kp[:, :, 1].astype(np.float64), rows[:, :, 0])
    assert np.array_equal(kp[:, :, 2].astype(np.float64), rows[:, :, 2])
    dec = ins & res['decided']
    off = np.maximum(np.abs(py - idx // w), np.abs(px - idx % w))
    parity(name, where, flags=flags, k=k, cases=int(idx.size), inside=int(ins.sum()), undecided=int(undecided.sum()),
           worst_over_allowance=verdict['worst'], max_bound=float(res['bound'][dec].max(initial=0.0)), max_offset=float(off[ins].max(initial=0.0)),
           max_error=float(np.maximum(np.abs(py - (idx // w + res['oy'])), np.abs(px - (idx % w + res['ox'])))[dec].max(initial=0.0)))
    return idx, res, (py, px)


RANDOM_CASES = [(c, hw, k, n) for c in D.DARK_CHANNELS for hw, k in D.DARK_MAPS for n in D.DARK_CROPS]


@pytest.mark.parametrize('C_,hw,k,n', RANDOM_CASES, ids=['C%d-%dx%d-k%d-n%d' % (c, hw[0], hw[1], k, n) for c, hw, k, n in RANDOM_CASES])
def test_dark_head_vs_fp64(lib, dev, C_, hw, k, n):
    """pam_head_decode_dark with flags 0, MERGE and MERGE | SHIFT on the seeded random-blob features (a batch of 2n + 1 rows, the spare
    one at 1e30), with and without a heat-map pointer."""
    h, w = hw
    name = 'C%d %dx%d k%d n%d' % (C_, h, w, k, n)
    feat, wt, b, boxes, _ = D.dark_inputs(C_, h, w, n)
    hd = DarkHead(lib, dev, feat, wt, b, boxes)
    moved = 0
    for flags in D.DARK_FLAGS:
        M, bd = D.reference(feat, wt, b, n, flags)
        idx, res, (py, px) = check_dark('test_dark_head_vs_fp64', name, hd, flags, k, M, bd, boxes)
        moved += int((np.abs(py - idx // w)[res['inside']] > 0.01).sum())
    assert moved > 0 or hw == (7, 5)                                   # the option does something: sub-cell offsets reached the rows


PLANTS = [((96, 72), 17), ((64, 48), 11), ((33, 17), 11), ((33, 17), 17), ((7, 5), 11)]


@pytest.mark.parametrize('hw,k', PLANTS, ids=['%dx%d-k%d' % (hw[0], hw[1], k) for hw, k in PLANTS])
def test_dark_head_planted_cases(lib, dev, hw, k):
    """The planted crops of dark_ref.planted_inputs (one crop per case), flags 0, MERGE, MERGE | SHIFT: winners on both sides of the
    inside rule along both axes (outside: the plain keypoint, bit for bit), a window hanging over both map edges at once, a winner in
    the last tile, a window across a tile seam, a plateau of identical feature vectors (the first cell wins), joint 7 with a bias of
    -inf (cell 0, score -inf), a lone spike on a negative map (no offset: exactly the plain keypoint), a blob only the mirrored crop
    carries (joint 6, at a column that reads it)."""
    h, w = hw
    for flags in D.DARK_FLAGS:
        feat, wt, b, boxes, cases = D.planted_inputs(h, w, k, flags)
        n = len(cases)
        hd = DarkHead(lib, dev, feat, wt, b, boxes)
        M, bd = D.reference(feat, wt, b, n, flags)
        name = 'planted %dx%d k%d' % (h, w, k)
        idx, res, (py, px) = check_dark('test_dark_head_planted_cases', name, hd, flags, k, M, bd, boxes, cap=False)
        frows = hd.decode(flags)[0]
        rows = hd.dark(flags, k)[0]
        am = D.argmax_decided(M, bd)
        assert (idx[:, 7] == 0).all() and np.isneginf(rows[:, 7, 2]).all() and rows[:, 7].tobytes() == frows[:, 7].tobytes()
        for i, cname, e in cases:
            j, where = e['joint'], (name, cname, flags)
            if 'among' in e:
                assert idx[i, j] in e['among'], where
                continue
            assert idx[i, j] == e['cell'] and bool(res['inside'][i, j]) == e['inside'], where
            same = rows[i, j].tobytes() == frows[i, j].tobytes()
            if e.get('zero') or not e['inside']:
                assert same, where
            elif cname != 'plateau':
                assert not same and res['decided'][i, j] and am[i, j], where


def test_bad_arguments_are_refused(lib, dev):
    """An even k, k = 7, k = 19 and the QUARTER flag give PAM_E_ARG and touch nothing; n == 0 is PAM_OK."""
    feat, wt, b, boxes, _ = D.dark_inputs(32, 7, 5, 1)
    hd = DarkHead(lib, dev, feat, wt, b, boxes)
    det = Guarded(3 * hd.slots * J * 3, torch.float64, dev)
    scratch = Guarded(int(lib.pam_head_decode_dark_scratch_bytes(1, 7, 5)), torch.uint8, dev)

    def call(n=1, flags=0, k=11):
        return lib.pam_head_decode_dark(stream(dev), n, n, 7, 5, hd.f.data_ptr(), 32, hd.wt.data_ptr(), hd.b.data_ptr(), J, flags, k, None,
                                        hd.view_of.data_ptr(), hd.slot_of.data_ptr(), hd.boxes.data_ptr(), hd.slots, det.ptr(), None, scratch.ptr())
    for kw in (dict(k=10), dict(k=12), dict(k=7), dict(k=19), dict(flags=4), dict(flags=5), dict(flags=7), dict(flags=2)):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(n=0, flags=3, k=17) == 0
    torch.cuda.synchronize()
    assert det.intact() and scratch.intact() and det.untouched(det.t) and scratch.untouched(scratch.t)


@pytest.mark.parametrize('flip', [False, True], ids=['plain', 'flip'])
def test_predict_under_dark(flip):
    """PoseResNet-50 at 256 x 192, 2 views, 3 boxes, dark=True with and without flip_test.  predict() has no heat-map argument, so the
    test re-issues the dump's decode -- head_decode on the replay's features with heat= -- and requires the same rows bit for bit; the
    maps that call wrote, read in float64, then give official_dark's keypoints (and dark64's), which the dump's must equal within the
    map-level bound: the float32 map is the kernel's own, so only float64 roundings remain (bound: 64 x 2^-53 |M| per cell through
    dark64's derivation) plus the float32 rounding of the box mapping.  The head bias is first set so that every map value is at least 1
    (found from a first forward): a seeded random network's maps straddle zero, outside DARK's domain.  With dark=False the same object then returns pam_head_decode_flip's rows, bit for bit,
    without a new capture."""
    net, frames = _net_case(dict(args=(50, 17, None), model_name='PoseResNet', dark=True, flip_test=flip))
    assert net.dark and net.decode_flags() == (3 if flip else 0) and net.blur_kernel is None
    net.predict(_pbl(frames, NET_BOXES))
    f0 = net.features(net.input_buffer(4))
    lowest = torch.einsum('nchw,jc->njhw', f0.float(), net.head_w.float()).amin(dim=(0, 2, 3))
    net.head_b.copy_(1.0 - lowest)
    dump = net.predict(_pbl(frames, NET_BOXES))
    caps = net.captures
    n, dev = 3, net.device
    f = net.features(net.input_buffer(4))
    nf, c, h, w = f.shape
    assert nf == (8 if flip else 4) and (h, w) == (64, 48) and net.dark_blur_kernel(h) == 11
    boxes = torch.tensor([bx for v in NET_BOXES for bx in v], dtype=torch.float32, device=dev)
    view_of = torch.tensor([0, 0, 1], dtype=torch.int32, device=dev); slot_of = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    got = dump.device_det.clone()

    def again():
        det = torch.zeros_like(got); kp = torch.zeros((n, J, 3), dtype=torch.float32, device=dev)
        heat = torch.zeros((n, J, h, w), dtype=torch.float32, device=dev).contiguous(memory_format=torch.channels_last)
        net.head_decode(f, view_of, slot_of, boxes, det, kp, heat=heat, n=n)
        torch.cuda.synchronize()
        return det, kp, heat
    det, kp, heat = again()
    for v, s in ((0, 0), (0, 1), (1, 0)):
        assert torch.equal(got[v, s], det[v, s])
    listed = np.asarray([it['keypoints'] for v in dump for it in v], dtype=np.float32).reshape(n, J, 3)
    assert np.array_equal(listed, kp.cpu().numpy())
    rows = torch.stack([det[0, 0], det[0, 1], det[1, 0]]).cpu().numpy()
    M = heat.cpu().numpy().astype(np.float64)                          # (n, 17, h, w): the map the decode ran on, the kernel's own bits
    assert (M > 0.5).all()
    bd = 64.0 * 2.0 ** -53 * np.abs(M)
    idx = M.reshape(n, J, -1).argmax(2)
    res = D.dark64(M, bd, idx, 11)
    bx = boxes.cpu().numpy()
    py, px, sy, sx = cells_of(rows, bx, h, w)
    verdict = D.judge(py, px, idx, res, w, sy, sx)
    assert verdict['wrong'] == [], verdict['wrong'][:5]
    off = D.official_dark(M, 11)
    dec = res['inside'] & res['decided']
    assert dec.sum() >= 0.5 * res['inside'].sum() and dec.sum() > 0, (int(dec.sum()), int(res['inside'].sum()))
    ey, ex = np.abs(py - off[..., 1]), np.abs(px - off[..., 0])
    assert (ey[dec] <= (res['bound'] + sy)[dec] + 1e-10).all() and (ex[dec] <= (res['bound'] + sx)[dec] + 1e-10).all()
    assert np.array_equal(bits(rows[:, :, 2]), bits(M.reshape(n, J, -1)[np.arange(n)[:, None], np.arange(J)[None, :], idx]))
    parity('test_predict_under_dark', 'flip' if flip else 'plain', inside=int(res['inside'].sum()), decided=int(dec.sum()),
           worst_over_allowance=verdict['worst'], max_vs_official=float(max(ey[dec].max(), ex[dec].max())),
           max_offset=float(np.maximum(np.abs(py - idx // w), np.abs(px - idx % w))[dec].max()))
    # dark off: the parent's decode on the same object
    net.dark = False
    dump_off = net.predict(_pbl(frames, NET_BOXES))
    assert net.captures == caps
    want = torch.zeros_like(got)
    scratch = torch.empty((int(net.lib.pam_head_decode_flip_scratch_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    assert net.lib.pam_head_decode_flip(stream(dev), n, n, h, w, f.data_ptr(), c, net.head_w.data_ptr(), net.head_b.data_ptr(), J, net.decode_flags(),
                                        None, view_of.data_ptr(), slot_of.data_ptr(), boxes.data_ptr(), want.shape[1], want.data_ptr(), None,
                                        scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    for v, s in ((0, 0), (0, 1), (1, 0)):
        assert torch.equal(dump_off.device_det[v, s], want[v, s]) and not torch.equal(want[v, s], got[v, s])
