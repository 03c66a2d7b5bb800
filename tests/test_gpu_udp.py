"""GPU: the UDP crop launch (pam_preprocess_crops_udp) and the UDP decode (pam_head_decode_udp) through the C ABI against the float64
restatements of tests/udp_ref.py.  Every output sits in guarded memory; rows a call does not cover keep their sentinel; every case
prints a PARITY line.  The inputs, their derived bounds and the share of undecided cases are those tests/test_udp_ref.py checks on the
CPU, and the checks applied to the kernels' results (image_ref.crop_check, dark_ref.judge) are the ones that reject the wrong variants
there."""
import json

import numpy as np
import pytest
import torch

import affine_ref as A
import dark_ref as D
import guarded_mem as G
import image_ref as R
import udp_ref as U
from image_ref import bf16_bits_to_f64, bf16_rne, crop_check
from test_gpu_affine_crop import PoisonedFrames, SENT32, up as up_frames
from test_gpu_flip import FlipHead, bits, rows_to_cells
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
    print('PARITY ' + json.dumps(dict(test=test, family='udp', where=where, **{k: (round(v, 7) if isinstance(v, float) else v) for k, v in figures.items()})))


# ---- crop --------------------------------------------------------------------------------------------------------------------------------
class Launch(object):
    """One pam_preprocess_crops_udp call into a fresh arena: out (n_total, H, W, out_c) bf16 and an effective-box table of n + 2 rows."""

    def __init__(self, lib, dev, pf, frame_hw, view_of, boxes, res, out_c, n_total, flip, antialias, scale=A.BOX_SCALE):
        H, W = res
        n = len(boxes)
        self.arena = G.GuardArena(dev, 2 * n_total * H * W * out_c + 16 * (n + 2) + 16 * G.GUARD + 8 * G.ALIGN)
        out = self.arena.alloc(n_total, out_c, H, W)
        eff = self.arena.alloc(n + 2, 8, 1, 1)                       # 16 bytes a row: 4 float32
        v_dev, b_dev = up_frames(np.asarray(view_of, dtype=np.int32), dev), up_frames(np.asarray(boxes, dtype=np.float32), dev)
        rc = lib.pam_preprocess_crops_udp(stream(dev), n, n_total, flip, pf.ptrs.data_ptr(), frame_hw[0], frame_hw[1], v_dev.data_ptr(),
                                          b_dev.data_ptr(), scale, H, W, out_c, out.data_ptr(), antialias, eff.data_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert self.arena.violations() == []
        assert self.arena.unwritten()[0] == 0, 'output elements never written'
        self.bits = self.arena.payload(self.arena.allocs[0]).reshape(n_total, H, W, out_c).cpu().numpy()
        self.eff_bits = self.arena.payload(self.arena.allocs[1]).cpu().numpy().view(np.uint32).reshape(n + 2, 4)
        self.n = n

    def values(self, rows=None):
        """(rows, 3, H, W) float64 of the first three channels."""
        b = self.bits[:self.n if rows is None else rows, :, :, :3]
        return bf16_bits_to_f64(b.view(np.uint16)).transpose(0, 3, 1, 2)


CASES = U.case_list()
IDS = ['%dx%d->%dx%d' % (c[0] + c[1]) for c in CASES]


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('k', range(len(CASES)), ids=IDS)
def test_udp_crops_against_crop_udp64(lib, dev, k, antialias):
    """Every case box (inside, down-scaled, half outside, fully outside, zero-sized, NaN), plain and antialias, 3- and 8-channel outputs,
    frames between bands of poison: values within crop_udp64's derived tolerance, identical bits whatever the poison and the channel
    count, the crops of the boxes that show nothing exactly the normalised zero, the effective-box table equal to box_cs64 and to
    pam_box_cs_host bit for bit with its spare rows untouched."""
    from pam import _lib
    hw, res, names, boxes = CASES[k]
    n = len(boxes)
    view_of = U.case_view_of(n)
    val, tol = U.case_reference(k, bool(antialias))
    pf = PoisonedFrames(U.case_frames(hw), dev)
    want_eff = bits(A.box_cs64(boxes, res[1], res[0]))
    assert np.array_equal(bits(_lib.box_cs(boxes, res[1], res[0], A.BOX_SCALE)), want_eff)
    first = None
    for fill in G.FILLS[:2]:
        pf.refill(fill)
        for out_c in (3, 8):
            L = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n, 0, antialias)
            got = L.values()
            assert np.isfinite(got).all(), 'poison reached a result'
            worst, bad = crop_check(got, val, tol)
            if first is None:
                first = L.bits[..., :3].copy()
                parity('test_udp_crops_against_crop_udp64', '%s aa%d' % (IDS[k], antialias), crops=n, worst_over_tol=worst, out_of_tol=bad)
            assert bad == 0, (fill, out_c, worst, bad)
            assert np.array_equal(L.bits[..., :3], first), (fill, out_c)
            assert out_c == 3 or not L.bits[..., 3:].any()               # +0: all bits clear
            assert np.array_equal(L.eff_bits[:n], want_eff)
            assert (L.eff_bits[n:] == SENT32).all(), 'a row of the effective-box table beyond n was written'
    zero = bf16_rne(A.kernel_f32_identity(np.zeros(3, dtype=np.uint8)))
    got = bf16_bits_to_f64(first.view(np.uint16))
    for nm in U.ALL_ZERO:
        assert np.array_equal(got[names.index(nm)], np.broadcast_to(zero, got.shape[1:])), nm
    assert not np.array_equal(got[names.index('inside')], np.broadcast_to(zero, got.shape[1:]))


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('out_c', [3, 8])
def test_udp_rows_padding_and_mirrors(lib, dev, out_c, antialias):
    """3 crops: n_total = n + 3 repeats the last crop bit for bit; under flip rows [n, 2n) are the column reversal of the plain rows bit
    for bit and rows from 2n on (n_total = 2n + 2) repeat the last mirror; the plain rows and the table are those of the unpadded call."""
    k = [i for i, c in enumerate(CASES) if c[1] == (64, 48) and c[0] == U.FRAME_SIZES[0]][0]
    hw, res, names, all_boxes = CASES[k]
    pick = [names.index(nm) for nm in ('down-scaled 3 x', 'half outside, left', 'inside, taller')]
    n = len(pick)
    boxes, view_of = all_boxes[pick], U.case_view_of(len(all_boxes))[pick]
    pf = PoisonedFrames(U.case_frames(hw), dev)
    pf.refill(G.FILLS[0])
    plain = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n, 0, antialias)
    val, tol = U.case_reference(k, bool(antialias))
    assert crop_check(plain.values(), val[pick], tol[pick])[1] == 0
    assert not np.array_equal(plain.bits, plain.bits[:, :, ::-1])
    padded = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n + 3, 0, antialias)
    assert np.array_equal(padded.bits[:n], plain.bits)
    assert all(np.array_equal(padded.bits[r], plain.bits[n - 1]) for r in range(n, n + 3))
    for n_total in (2 * n, 2 * n + 2):
        f = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n_total, 1, antialias)
        assert np.array_equal(f.bits[:n], plain.bits)
        assert np.array_equal(f.bits[n:2 * n], plain.bits[:, :, ::-1])
        assert all(np.array_equal(f.bits[r], f.bits[2 * n - 1]) for r in range(2 * n, n_total))
        assert np.array_equal(f.eff_bits, plain.eff_bits)
    assert np.array_equal(padded.eff_bits, plain.eff_bits) and (plain.eff_bits[n:] == SENT32).all()
    parity('test_udp_rows_padding_and_mirrors', 'c%d aa%d' % (out_c, antialias), mismatches=0)


def test_udp_crop_ends_on_the_box_edges_bit_for_bit(lib, dev):
    """scale 1, a square output and a square box with We = out_w - 1 and integer corners (only a square has the pitch 1 along both axes:
    the effective box has the input's aspect, out_w / out_h): pixel 0 reads the box's left column and pixel
    out_w - 1 its right edge column xe + We, every sample falls on a pixel, and the output is bf16_rne of the float32 expression the
    kernel writes.  (The affine launch on the same box has the pitch (out_w - 1) / out_w and ends one pitch short of the edge.)"""
    hw = U.FRAME_SIZES[0]
    fr = U.case_frames(hw)
    H, W = 13, 13
    boxes = np.asarray([[5, 7, W - 1, H - 1], [hw[1] - W, hw[0] - H, W - 1, H - 1]], dtype=np.float32)
    view_of = np.asarray([0, 1], dtype=np.int32)
    pf = PoisonedFrames(fr, dev)
    pf.refill(G.FILLS[0])
    L = Launch(lib, dev, pf, hw, view_of, boxes, (H, W), 3, len(boxes), 0, 0, scale=1.0)
    got = bf16_bits_to_f64(L.bits.view(np.uint16))
    assert np.array_equal(L.eff_bits[:len(boxes)], bits(boxes))
    for i, b in enumerate(boxes):
        x, y = int(b[0]), int(b[1])
        want = bf16_rne(A.kernel_f32_identity(fr[view_of[i], y:y + H, x:x + W, ::-1]))
        assert np.array_equal(got[i], want), i


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
class UdpHead(FlipHead):
    """FlipHead (device copies of one case: rows [0, n) plain, [n, 2n) mirrored, one spare; guarded outputs) with the new entry point."""

    def udp(self, flags, k, heat=False):
        """-> det rows (n, 17, 3) float64, kp (n, 17, 3), heat (n, P, 17) or None."""
        n = self.n
        need = int(self.lib.pam_head_decode_udp_scratch_bytes(n, self.h, self.w))
        assert need == int(self.lib.pam_head_decode_scratch_bytes(n, self.h, self.w))
        scratch = Guarded(need, torch.uint8, self.dev)
        det = Guarded(3 * self.slots * J * 3, torch.float64, self.dev)
        kp = Guarded(self.rows * J * 3, torch.float32, self.dev)
        hm = Guarded(self.rows * self.P * J, torch.float32, self.dev) if heat else None
        rc = self.lib.pam_head_decode_udp(stream(self.dev), n, n, self.h, self.w, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J,
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


def check_udp(name, where, hd, flags, k, M, bd, boxes, cap=True):
    """One pam_head_decode_udp call (blur size k, or 0) against pam_head_decode_flip with the same merge flags and against udp64 on the
    float64 map:
    * arg-max cell and score exactly pam_head_decode_flip's (the cell through each entry's own mapping, the score's bits), the cell
      accepted by image_ref.argmax_check;
    * decided positions within their derived bound plus the float32 rounding of the UDP mapping, undecided ones within the widest answer
      the derivation allows (dark_ref.judge); at k = 0 every position is the cell itself; undecided cases (arg-max included) at most
      1 % (cap=False, the planted crops: their other joints' maps carry no blob; the caller asserts the planted joint's case instead);
    * kp = the det rows in float32 (x, y, score); nothing read from the spare feature row (1e30: a finite map's row is finite);
    * the heat output bit-equal to pam_head_decode_flip's M, and the keypoints the same with and without it.
    -> idx, result of udp64, (py, px), rows."""
    n, h, w = hd.n, hd.h, hd.w
    frows, fkp, fheat, _ = hd.decode(flags, heat=True)
    rows, kp, _ = hd.udp(flags, k)
    rows2, kp2, heat = hd.udp(flags, k, heat=True)
    assert rows.tobytes() == rows2.tobytes() and kp.tobytes() == kp2.tobytes(), (name, where, 'the heat-map pointer changed the keypoints')
    assert np.array_equal(bits(heat), bits(fheat)), (name, where, 'heat output differs from pam_head_decode_flip')
    idx, oy0, ox0 = rows_to_cells(frows, boxes[:n], h, w)
    assert not oy0.any() and not ox0.any()
    flatM, flatB = M.reshape(n, J, -1), bd.reshape(n, J, -1)
    am = R.argmax_check(flatM, flatB, idx)
    assert am['wrong'] == [], (name, where, am['wrong'][:5])
    assert np.array_equal(bits(rows[:, :, 2]), bits(frows[:, :, 2])), (name, where, 'score bits')
    res = U.udp64(M, bd, idx, k)
    py, px, sy, sx = U.cells_of(rows, boxes[:n], h, w)
    fin = np.isfinite(flatM.max(2))
    assert np.isfinite(rows[fin]).all(), (name, where, 'non-finite keypoint of a finite map')
    verdict = D.judge(py, px, idx, res, w, sy, sx)
    assert verdict['wrong'] == [], (name, where, verdict['wrong'][:5])
    undecided = ~(res['decided'] & D.argmax_decided(M, bd))
    assert not cap or undecided.sum() <= 0.01 * idx.size, (name, where, int(undecided.sum()), int(idx.size))
    assert np.array_equal(kp[:, :, 0].astype(np.float64), rows[:, :, 1]) and np.array_equal(kp[:, :, 1].astype(np.float64), rows[:, :, 0])
    assert np.array_equal(kp[:, :, 2].astype(np.float64), rows[:, :, 2])
    dec = res['decided']
    with np.errstate(invalid='ignore'):
        off = np.maximum(np.abs(py - idx // w), np.abs(px - idx % w))
        err = np.maximum(np.abs(py - (idx // w + res['oy'])), np.abs(px - (idx % w + res['ox'])))
    parity(name, where, flags=flags, k=k, cases=int(idx.size), undecided=int(undecided.sum()), worst_over_allowance=verdict['worst'],
           max_bound=float(res['bound'][dec].max(initial=0.0)), max_offset=float(off[dec].max(initial=0.0)), max_error=float(err[dec].max(initial=0.0)))
    return idx, res, (py, px), rows


RANDOM_CASES = [(c, hw, k, n) for c in U.UDP_CHANNELS for hw, k in U.UDP_MAPS for n in U.UDP_CROPS]


@pytest.mark.parametrize('C_,hw,k,n', RANDOM_CASES, ids=['C%d-%dx%d-k%d-n%d' % (c, hw[0], hw[1], k, n) for c, hw, k, n in RANDOM_CASES])
def test_udp_head_vs_fp64(lib, dev, C_, hw, k, n):
    """pam_head_decode_udp with flags 0, MERGE and MERGE | SHIFT, at the map's blur size and at 0, on the seeded random-blob features (a
    batch of 2n + 1 rows, the spare one at 1e30), with and without a heat-map pointer."""
    h, w = hw
    name = 'C%d %dx%d k%d n%d' % (C_, h, w, k, n)
    moved = 0
    for shift, flag_set in ((False, (0, 1)), (True, (3,))):
        feat, wt, b, boxes, _ = U.udp_inputs(C_, h, w, n, k, shift)
        hd = UdpHead(lib, dev, feat, wt, b, boxes)
        for flags in flag_set:
            M, bd = U.reference(feat, wt, b, n, flags)
            idx, res, (py, px), rows = check_udp('test_udp_head_vs_fp64', name, hd, flags, k, M, bd, boxes)
            moved += int((np.abs(py - idx // w) > 0.01).sum())
            _, _, _, rows0 = check_udp('test_udp_head_vs_fp64', name, hd, flags, 0, M, bd, boxes)
            want_y, want_x = U.map64(idx // w, idx % w, boxes[:n], h, w)
            assert np.array_equal(rows0[:, :, 0], want_y) and np.array_equal(rows0[:, :, 1], want_x), (name, flags, 'the mapping of a whole cell')
    assert moved > 0                                                   # the option does something: sub-cell offsets reached the rows


@pytest.mark.parametrize('hw,k', U.PLANTS, ids=['%dx%d-k%d' % (hw[0], hw[1], k) for hw, k in U.PLANTS])
def test_udp_head_planted_cases(lib, dev, hw, k):
    """The planted crops of udp_ref.planted_inputs (one crop per cell), flags 0, MERGE, MERGE | SHIFT, k = 11 and 17: the winner in each
    corner, on each edge and at the centre -- where DARK decodes nothing, every border winner takes a decided step here -- joint 7 with
    a bias of -inf (cell 0, score -inf, offset exactly 0), and the 2 x 2 map (the smallest the entry takes; its window of 2 R + 3 cells
    is reflections of four cells, the blurred map is flat and the step is whatever the bound allows)."""
    h, w = hw
    for flags in U.UDP_FLAGS:
        feat, wt, b, boxes, cases = U.planted_inputs(h, w, flags)
        n = len(cases)
        hd = UdpHead(lib, dev, feat, wt, b, boxes)
        M, bd = U.reference(feat, wt, b, n, flags)
        name = 'planted %dx%d k%d' % (h, w, k)
        idx, res, (py, px), rows = check_udp('test_udp_head_planted_cases', name, hd, flags, k, M, bd, boxes, cap=False)
        rows0 = hd.udp(flags, 0)[0]
        am = D.argmax_decided(M, bd)
        assert (idx[:, 7] == 0).all() and np.isneginf(rows[:, 7, 2]).all() and rows[:, 7].tobytes() == rows0[:, 7].tobytes()
        for i, (y, x) in cases:
            where = (name, (y, x), flags)
            assert idx[i, 5] == y * w + x and am[i, 5], where
            if hw == (2, 2):
                continue
            assert res['decided'][i, 5], where
            if y in (0, h - 1) or x in (0, w - 1):
                assert rows[i, 5].tobytes() != rows0[i, 5].tobytes(), where
                assert max(abs(py[i, 5] - y), abs(px[i, 5] - x)) > 0.4, where


def test_bad_arguments_are_refused(lib, dev):
    """Every documented PAM_E_ARG of the two entries comes back before a launch and touches nothing; n == 0 is PAM_OK."""
    feat, wt, b, boxes, _ = U.udp_inputs(32, 7, 5, 1, 11)
    hd = UdpHead(lib, dev, feat, wt, b, boxes)
    det = Guarded(3 * hd.slots * J * 3, torch.float64, dev)
    scratch = Guarded(int(lib.pam_head_decode_udp_scratch_bytes(1, 7, 5)), torch.uint8, dev)
    assert lib.pam_head_decode_udp_scratch_bytes(1, 1, 5) == -1 and lib.pam_head_decode_udp_scratch_bytes(1, 7, 1) == -1

    def call(n=1, row0=None, h=7, w=5, Cc=32, Jn=J, flags=0, k=11, f=hd.f.data_ptr(), d=det.ptr(), s=scratch.ptr()):
        return lib.pam_head_decode_udp(stream(dev), n, n if row0 is None else row0, h, w, f, Cc, hd.wt.data_ptr(), hd.b.data_ptr(), Jn, flags, k, None,
                                       hd.view_of.data_ptr(), hd.slot_of.data_ptr(), hd.boxes.data_ptr(), hd.slots, d, None, s)
    for kw in (dict(k=10), dict(k=12), dict(k=7), dict(k=19), dict(k=1), dict(k=-11), dict(flags=4), dict(flags=5), dict(flags=7), dict(flags=2),
               dict(flags=8), dict(flags=1, row0=0), dict(h=1, w=35), dict(h=35, w=1), dict(h=1, w=35, k=0), dict(Jn=16), dict(Cc=28), dict(n=-1),
               dict(f=None), dict(d=None), dict(s=None)):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(n=0, flags=3, k=17) == 0 and call(n=0, k=0) == 0
    torch.cuda.synchronize()
    assert det.intact() and scratch.intact() and det.untouched(det.t) and scratch.untouched(scratch.t)
    # the crop entry
    hw = U.FRAME_SIZES[1]
    pf = PoisonedFrames(U.case_frames(hw), dev)
    pf.refill(G.FILLS[0])
    n, H, W = 2, 16, 12
    out = torch.full((2 * n + 1, H, W, 8), -7.0, dtype=torch.bfloat16, device=dev)
    eff = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    v = up_frames(np.asarray([0, 1], dtype=np.int32), dev); bx = up_frames(np.asarray([[5, 7, 12, 16], [3, 3, 20, 9]], dtype=np.float32), dev)
    good = [stream(dev), n, n, 0, pf.ptrs.data_ptr(), hw[0], hw[1], v.data_ptr(), bx.data_ptr(), 1.25, H, W, 8, out.data_ptr(), 0, eff.data_ptr()]
    fn = lib.pam_preprocess_crops_udp
    bad = {1: -1, 4: None, 7: None, 8: None, 9: [0.0, -1.25, float('nan')], 10: [1, 0, -3], 11: [1, 0, -3], 12: [4, 0, 16], 13: None, 15: None}
    for at, values in bad.items():
        for val in (values if isinstance(values, list) else [values]):
            a = list(good); a[at] = val
            assert fn(*a) == -1, (at, val)
    a = list(good); a[2] = n - 1
    assert fn(*a) == -1                                                   # n_total < n
    a = list(good); a[3] = 1; a[2] = 2 * n - 1
    assert fn(*a) == -1                                                   # flip: n_total < 2 n
    a = list(good); a[1] = 0; a[2] = 0
    assert fn(*a) == 0                                                    # nothing to do
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((eff == -7.0).all())
    a = list(good); a[3] = 1; a[2] = 2 * n + 1
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not bool((eff == -7.0).any())
