"""GPU: the affine crop launch (pam_preprocess_crops_affine) and the table launch (pam_box_cs) through the C ABI against the float64
restatement of tests/affine_ref.py with its derived tolerance.  Every output is carved out of guarded_mem's sentinel arena, every frame
lies between bands of poison: no output element may stay unwritten, no band may change, rows of the effective-box table the call does
not own keep the sentinel, and nothing read outside a frame may reach a result.  The inputs and the tolerance are those
tests/test_affine_ref.py checks on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import affine_ref as A
import guarded_mem as G
from image_ref import bf16_bits_to_f64, bf16_rne, crop_check

pytestmark = pytest.mark.gpu

SENT32 = np.uint32(G.SENTINEL << 16 | G.SENTINEL)           # a float32 of the arena's sentinel halves: a NaN


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib.load()


def parity(test, where, **figures):
    print('PARITY ' + json.dumps(dict(test=test, family='affine', where=where, **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in figures.items()})))


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def up(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)           # (a copy: the shared case frames are read-only)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class PoisonedFrames(object):
    """Every view's (h, w, 3) uint8 frame in a buffer of its own between two bands of 2 * GUARD bytes of a 16-bit fill pattern
    (guarded_mem.FILLS: as bytes 0x7F / 0xE5, 0x7F / 0x00 and 0xFF / 0x00 -- a stray read is a pixel of 127, 229, 255 or 0 where the
    reference has the frame's own pixel or the zero border; the three patterns between them leave no value a stray byte could hide in)."""

    def __init__(self, frames, dev):
        self.nbytes = int(frames[0].size)
        self.bufs, self.views = [], []
        for f in frames:
            buf = torch.empty(2 * G.GUARD + (self.nbytes + 1) // 2, dtype=torch.int16, device=dev)
            v = buf.view(torch.uint8)[2 * G.GUARD:2 * G.GUARD + self.nbytes]
            self.bufs.append(buf); self.views.append(v)
        self.frames = [up(f, dev).reshape(-1) for f in frames]
        self.ptrs = torch.tensor([v.data_ptr() for v in self.views], dtype=torch.int64, device=dev)

    def refill(self, fill):
        for buf, v, f in zip(self.bufs, self.views, self.frames):
            buf.fill_(G.as_i16(fill))
            v.copy_(f)


class Launch(object):
    """One pam_preprocess_crops_affine call into a fresh arena: out (n_total, H, W, out_c) bf16 and an effective-box table of n + 2 rows."""

    def __init__(self, lib, dev, pf, frame_hw, view_of, boxes, res, out_c, n_total, flip, antialias, scale=A.BOX_SCALE):
        H, W = res
        n = len(boxes)
        self.arena = G.GuardArena(dev, 2 * n_total * H * W * out_c + 16 * (n + 2) + 16 * G.GUARD + 8 * G.ALIGN)
        out = self.arena.alloc(n_total, out_c, H, W)
        eff = self.arena.alloc(n + 2, 8, 1, 1)                       # 16 bytes a row: 4 float32
        v_dev, b_dev = up(np.asarray(view_of, dtype=np.int32), dev), up(np.asarray(boxes, dtype=np.float32), dev)
        rc = lib.pam_preprocess_crops_affine(stream(dev), n, n_total, flip, pf.ptrs.data_ptr(), frame_hw[0], frame_hw[1], v_dev.data_ptr(),
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


CASES = A.case_list()
IDS = ['%dx%d->%dx%d' % (c[0] + c[1]) for c in CASES]


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('k', range(len(CASES)), ids=IDS)
def test_affine_crops_against_warp64(lib, dev, k, antialias):
    """Every case box, plain and antialias, 3- and 8-channel outputs, under each poison: values within warp64's tolerance, identical
    bits whatever the poison and the channel count, the crops of the boxes outside the frame exactly the normalised zero, the
    effective-box table equal to box_cs64 and to pam_box_cs bit for bit with its spare rows untouched."""
    hw, res, names, boxes = CASES[k]
    n = len(boxes)
    frames = A.case_frames(hw)
    view_of = A.case_view_of(n)
    val, tol = A.case_reference(k, bool(antialias))
    pf = PoisonedFrames(frames, dev)
    want_eff = bits(A.box_cs64(boxes, res[1], res[0]))
    first = None
    for fill in G.FILLS:
        pf.refill(fill)
        for out_c in (3, 8):
            L = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n, 0, antialias)
            got = L.values()
            assert np.isfinite(got).all(), 'poison reached a result'
            worst, bad = crop_check(got, val, tol)
            if first is None:
                first = L.bits[..., :3].copy()
                parity('test_affine_crops_against_warp64', '%s aa%d' % (IDS[k], antialias), crops=n, worst_over_tol=worst, out_of_tol=bad)
            assert bad == 0, (fill, out_c, worst, bad)
            assert np.array_equal(L.bits[..., :3], first), (fill, out_c)
            assert out_c == 3 or not L.bits[..., 3:].any()               # +0: all bits clear
            assert np.array_equal(L.eff_bits[:n], want_eff)
            assert (L.eff_bits[n:] == SENT32).all(), 'a row of the effective-box table beyond n was written'
    zero = bf16_rne(A.kernel_f32_identity(np.zeros(3, dtype=np.uint8)))
    got = bf16_bits_to_f64(first.view(np.uint16))
    for nm in A.OUTSIDE:
        if nm in names:
            assert np.array_equal(got[names.index(nm)], np.broadcast_to(zero, got.shape[1:])), nm
    # the table launch
    b_dev = up(boxes, dev)
    tab = torch.empty((n + 2, 4), dtype=torch.float32, device=dev)
    tab.view(torch.int32).fill_(int(SENT32))
    assert lib.pam_box_cs(stream(dev), n, b_dev.data_ptr(), res[1], res[0], A.BOX_SCALE, tab.data_ptr()) == 0
    torch.cuda.synchronize()
    tb = tab.view(torch.int32).cpu().numpy().view(np.uint32)
    assert np.array_equal(tb[:n], want_eff) and (tb[n:] == SENT32).all()
    from pam import _lib
    assert np.array_equal(bits(_lib.box_cs(boxes, res[1], res[0], A.BOX_SCALE)), want_eff)


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('out_c', [3, 8])
@pytest.mark.parametrize('n', A.CROP_COUNTS)
def test_rows_padding_and_mirrors(lib, dev, n, out_c, antialias):
    """n = 1, 3, 5 crops: n_total = n + 3 repeats the last crop bit for bit; under flip rows [n, 2n) are the column reversal of the plain
    rows bit for bit and rows from 2n on (n_total = 2n + 2) repeat the last mirror; the plain rows and the table are those of the
    unpadded call."""
    k = [i for i, c in enumerate(CASES) if c[1] == (64, 48) and c[0] == A.FRAME_SIZES[1]][0]
    hw, res, names, all_boxes = CASES[k]
    pick = [names.index(nm) for nm in ('down-scaled 3 x', 'over the left edge', 'taller', 'over the bottom edge', 'up-scaled 9 x 7')][:n]
    boxes, view_of = all_boxes[pick], A.case_view_of(len(all_boxes))[pick]
    pf = PoisonedFrames(A.case_frames(hw), dev)
    pf.refill(G.FILLS[0])
    plain = Launch(lib, dev, pf, hw, view_of, boxes, res, out_c, n, 0, antialias)
    val, tol = A.case_reference(k, bool(antialias))
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
    parity('test_rows_padding_and_mirrors', 'n%d c%d aa%d' % (n, out_c, antialias), mismatches=0)


@pytest.mark.parametrize('antialias', [0, 1])
def test_identity_known_answer_bit_for_bit(lib, dev, antialias):
    """scale 1, a box at the aspect with We = out_w and integer corners: every sample falls on a pixel, and the output is bf16_rne of the
    float32 expression the kernel writes, (p * (1/255) - mean) * (1/std); one pixel past each edge the column / row outside is that of 0."""
    hw = A.FRAME_SIZES[0]
    fr = A.case_frames(hw)
    H, W = 16, 12
    boxes = np.asarray([[5, 7, W, H], [hw[1] - W, hw[0] - H, W, H], [-1, 7, W, H], [5, -1, W, H], [hw[1] - W + 1, 3, W, H], [4, hw[0] - H + 1, W, H]],
                       dtype=np.float32)
    view_of = np.asarray([0, 1, 0, 1, 0, 1], dtype=np.int32)
    pf = PoisonedFrames(fr, dev)
    padded = np.zeros((2, hw[0] + 2, hw[1] + 2, 3), dtype=np.uint8)          # the frames inside one pixel of zero border
    padded[:, 1:-1, 1:-1] = fr
    for fill in G.FILLS:
        pf.refill(fill)
        L = Launch(lib, dev, pf, hw, view_of, boxes, (H, W), 3, len(boxes), 0, antialias, scale=1.0)
        got = bf16_bits_to_f64(L.bits.view(np.uint16))
        assert np.array_equal(L.eff_bits[:len(boxes)], bits(boxes))
        for i, b in enumerate(boxes):
            x, y = int(b[0]) + 1, int(b[1]) + 1
            want = bf16_rne(A.kernel_f32_identity(padded[view_of[i], y:y + H, x:x + W, ::-1]))
            assert np.array_equal(got[i], want), (fill, i)


def test_argument_errors(lib, dev):
    """Every documented argument error of the two device entries returns PAM_E_ARG before any launch: the outputs keep their sentinel."""
    hw = A.FRAME_SIZES[0]
    pf = PoisonedFrames(A.case_frames(hw), dev)
    pf.refill(G.FILLS[0])
    n, H, W = 2, 16, 12
    out = torch.full((2 * n + 1, H, W, 8), -7.0, dtype=torch.bfloat16, device=dev)
    eff = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    v = up(np.asarray([0, 1], dtype=np.int32), dev); b = up(np.asarray([[5, 7, 12, 16], [3, 3, 20, 9]], dtype=np.float32), dev)
    good = [stream(dev), n, n, 0, pf.ptrs.data_ptr(), hw[0], hw[1], v.data_ptr(), b.data_ptr(), 1.25, H, W, 8, out.data_ptr(), 0, eff.data_ptr()]
    fn = lib.pam_preprocess_crops_affine
    bad = {1: -1, 4: None, 7: None, 8: None, 9: [0.0, -1.25, float('nan')], 10: [0, -3], 11: [0, -3], 12: [4, 0, 16], 13: None, 15: None}
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
    tab = lib.pam_box_cs
    g2 = [stream(dev), n, b.data_ptr(), W, H, 1.25, eff.data_ptr()]
    for at, values in {1: -1, 2: None, 3: [0, -1], 4: [0, -1], 5: [0.0, -2.0, float('nan')], 6: None}.items():
        for val in (values if isinstance(values, list) else [values]):
            a = list(g2); a[at] = val
            assert tab(*a) == -1, (at, val)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((eff == -7.0).all())
    a = list(good); a[3] = 1; a[2] = 2 * n + 1
    assert fn(*a) == 0 and tab(*g2) == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not bool((eff == -7.0).any())
