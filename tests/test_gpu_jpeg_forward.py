"""The device half of the JPEG encode path (csrc/pam_jpeg_fwd.hip) on a real MI355X: k_jpeg_fdct's coefficients against the
restatement (tests/jpeg_enc_ref.py, itself held to Pillow) with array_equal, frames and coefficient buffers in sentinel-filled, banded
memory under two complementary fills (a word that is never written differs between the two runs, so it cannot equal the reference in
both), 32 images of mixed sizes and samplings in one launch against one launch each, the device's coefficients through pam_jpeg_encode
against Pillow's file bytes, and forward + pam_jpeg_reconstruct against Pillow's decode of Pillow's file."""
import ctypes as C

import numpy as np
import pytest

from pam import _lib
import guarded_mem as GM
import jpeg_enc_ref as E
import jpeg_ref as J

pytestmark = pytest.mark.gpu
BAND = 2 * GM.GUARD              # bytes on each side
FILLS = (0xE5, 0x1A)             # complementary bytes
SIZES = [(1, 1), (8, 8), (17, 23), (33, 31), (40, 50), (9, 70), (24, 8), (200, 150)]      # (W, H)


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


class Banded(object):
    """nbytes of device memory at a 256-byte-aligned address plus `shift` between two bands of at least BAND bytes of `fill`; the band
    behind begins at the payload's last byte + 1.  The payload starts out as `fill` too."""

    def __init__(self, torch, nbytes, fill, shift=0):
        raw = torch.empty(nbytes + 2 * BAND + GM.ALIGN + shift, dtype=torch.uint8, device='cuda:0')
        self.start = BAND + (-(raw.data_ptr() + BAND)) % GM.ALIGN + shift
        self.raw, self.nbytes, self.fill = raw[:self.start + nbytes + BAND], nbytes, fill
        self.raw.fill_(fill)
        self.payload = self.raw[self.start:self.start + nbytes]

    def damaged(self):
        return int((self.raw[:self.start] != self.fill).sum() + (self.raw[self.start + self.nbytes:] != self.fill).sum())


def frames_of(w, h, seed):
    """The four contents of one size: all-0, all-255, the 0 / 255 checkerboard (the largest coefficients a frame can give), noise."""
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), board,
            np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)]


def run(torch, lib, items, fill):
    """One pam_jpeg_forward over items = [(BGR uint8 (H, W, 3), sampling, tables (2, 64))], every frame (at an odd address), table and
    coefficient buffer in banded memory of `fill` -> ([int16 coefficients], damaged band bytes, the device buffers)."""
    images = (_lib.PamJpegFwdImage * len(items))()
    bufs = []
    for k, (im, (bgr, sampling, tables)) in enumerate(zip(images, items)):
        h, w = bgr.shape[:2]
        hs, vs = E.SAMPLINGS[sampling]
        words = E.layout(w, h, hs, vs)['coef_words']
        src, quant, coef = Banded(torch, bgr.size, fill, shift=k % 4), Banded(torch, 3 * 64 * 2, fill), Banded(torch, 2 * words, fill)
        src.payload.copy_(torch.from_numpy(np.ascontiguousarray(bgr).reshape(-1)))
        quant.payload.copy_(torch.from_numpy(np.asarray(tables)[[0, 1, 1]].astype(np.uint16).view(np.uint8).reshape(-1)))
        im.dev_bgr, im.dev_quant, im.dev_coef = src.payload.data_ptr(), quant.payload.data_ptr(), coef.payload.data_ptr()
        im.width, im.height, im.h_samp, im.v_samp = w, h, hs, vs
        bufs.append((src, quant, coef))
    assert lib.pam_jpeg_forward(None, len(items), images) == 0
    torch.cuda.synchronize()
    coefs = [c.payload.cpu().numpy().view(np.int16) for _, _, c in bufs]
    for (bgr, _, _), (src, _, _) in zip(items, bufs):
        assert np.array_equal(src.payload.cpu().numpy(), bgr.reshape(-1))          # the frame is read, never written
    return coefs, sum(b.damaged() for trio in bufs for b in trio), bufs


def host_encode(lib, coef, w, h, sampling, quality):
    hs, vs = E.SAMPLINGS[sampling]
    p = _lib.PamJpegEncodeParams(width=w, height=h, h_samp=hs, v_samp=vs, quality=quality)
    cap = C.c_size_t(0)
    assert lib.pam_jpeg_encode_bound(w, h, hs, vs, C.byref(cap)) == 0
    out = np.zeros(cap.value, dtype=np.uint8)
    n = C.c_size_t(0)
    coef = np.ascontiguousarray(coef)
    assert lib.pam_jpeg_encode(coef.ctypes.data, coef.size, C.byref(p), out.ctypes.data, out.size, C.byref(n)) == 0
    return bytes(out[:n.value])


@pytest.fixture(scope='module')
def matrix():
    """[(BGR, sampling, tables, quality)]: 8 sizes x 3 samplings x 4 contents, the qualities cycling; the restatement's coefficients are
    computed once (``wants``)."""
    items = []
    for i, (w, h) in enumerate(SIZES):
        for j, s in enumerate(E.SAMPLINGS):
            for k, bgr in enumerate(frames_of(w, h, 100 + 10 * i + j)):
                q = E.QUALITIES[(i + 2 * j + 3 * k) % 7] if k == 3 else (100, 75, 100)[k]
                items.append((bgr, s, E.quality_tables(q), q))
    return items


@pytest.fixture(scope='module')
def wants(matrix):
    return [E.forward(bgr, s, t) for bgr, s, t, _ in matrix]


def test_coefficients_equal_the_restatement_between_bands_under_both_fills(torch, lib, matrix, wants):
    assert len(matrix) == 96
    bad = []
    for fill in FILLS:
        for lo in range(0, len(matrix), 32):
            coefs, damaged, _ = run(torch, lib, [m[:3] for m in matrix[lo:lo + 32]], fill)
            assert damaged == 0, (fill, lo)
            for k, got in enumerate(coefs):
                if not np.array_equal(got, wants[lo + k]):               # padding blocks included: zeros under either fill
                    bad.append((fill, lo + k, matrix[lo + k][0].shape, matrix[lo + k][1]))
    assert not bad, bad[:10]
    assert max(int(np.abs(w).max()) for w in wants) >= 1016              # an all-0 frame at the all-ones tables: DC -1024, the largest there is


def test_32_mixed_images_in_one_launch_equal_one_launch_each(torch, lib, matrix, wants):
    pick = list(range(3, 96, 3))[:32]                                    # every size, sampling and content
    assert len({(matrix[i][0].shape, matrix[i][1]) for i in pick}) >= 20
    together, damaged, _ = run(torch, lib, [matrix[i][:3] for i in pick], FILLS[0])
    assert damaged == 0
    for k, i in enumerate(pick):
        single, damaged, _ = run(torch, lib, [matrix[i][:3]], FILLS[1])
        assert damaged == 0
        assert np.array_equal(single[0], together[k]) and np.array_equal(single[0], wants[i]), i


def test_device_coefficients_through_the_host_encoder_equal_pillows_file(torch, lib, matrix):
    pick = list(range(1, 96, 3))
    coefs, damaged, _ = run(torch, lib, [matrix[i][:3] for i in pick], FILLS[0])
    assert damaged == 0
    for got, i in zip(coefs, pick):
        bgr, s, _, q = matrix[i]
        assert host_encode(lib, got, bgr.shape[1], bgr.shape[0], s, q) == E.pillow_bytes(bgr, s, q), (i, bgr.shape, s, q)


def test_a_1032x776_frame_at_the_defaults_is_pillows_file(torch, lib, tmp_path):
    """The Shelf frame size at quality 75 and 4:2:0: 776 rows are 48.5 MCU rows, 1032 columns 64.5 MCUs."""
    from PIL import Image
    rgb = J.content('smooth', 1032, 776, 3)
    rgb = np.clip(rgb.astype(np.int16) + np.random.default_rng(4).integers(-24, 25, rgb.shape), 0, 255).astype(np.uint8)
    bgr = np.ascontiguousarray(rgb[:, :, ::-1])
    p = str(tmp_path / 'shelf.jpg')
    Image.fromarray(rgb).save(p)
    coefs, damaged, _ = run(torch, lib, [(bgr, '420', E.quality_tables(75))], FILLS[1])
    assert damaged == 0 and coefs[0].size == 64 * (130 * 98 + 2 * 65 * 49)
    assert host_encode(lib, coefs[0], 1032, 776, '420', 75) == open(p, 'rb').read()


@pytest.mark.parametrize('sampling', list(E.SAMPLINGS))
def test_forward_then_reconstruct_equals_pillows_decode_of_pillows_file(torch, lib, tmp_path, sampling):
    """The coefficient buffer goes to pam_jpeg_reconstruct as it is: its padding blocks are zeros, which no output pixel depends on."""
    for i, (w, h) in enumerate(((17, 23), (33, 31), (40, 50), (24, 8))):
        bgr = np.ascontiguousarray(J.content('smooth' if i % 2 else 'noise', w, h, 60 + i)[:, :, ::-1])
        q = (92, 75, 50, 30)[i]
        tables = E.quality_tables(q)
        _, damaged, bufs = run(torch, lib, [(bgr, sampling, tables)], FILLS[i % 2])
        assert damaged == 0
        _, quant, coef = bufs[0]
        hs, vs = E.SAMPLINGS[sampling]
        planes = torch.empty(coef.nbytes // 2, dtype=torch.uint8, device='cuda:0')
        out = torch.empty((h, w, 3), dtype=torch.uint8, device='cuda:0')
        im = (_lib.PamJpegImage * 1)()
        im[0].dev_coef, im[0].dev_quant, im[0].dev_planes, im[0].dev_out = coef.payload.data_ptr(), quant.payload.data_ptr(), planes.data_ptr(), out.data_ptr()
        im[0].width, im[0].height, im[0].n_comp, im[0].h_samp, im[0].v_samp = w, h, 3, hs, vs
        assert lib.pam_jpeg_reconstruct(None, 1, im) == 0
        torch.cuda.synchronize()
        p = str(tmp_path / ('r_%d.jpg' % i))
        with open(p, 'wb') as f:
            f.write(E.pillow_bytes(bgr, sampling, q))
        assert np.array_equal(out.cpu().numpy(), J.pillow_bgr(p)), (w, h, sampling)


def test_forward_refuses_what_it_cannot_run_before_any_launch(torch, lib):
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda:0')
    base = buf.data_ptr()

    def call(n=1, **kw):
        im = (_lib.PamJpegFwdImage * 1)()
        v = dict(dev_bgr=base + 1, dev_quant=base + 1024, dev_coef=base + 2048, width=8, height=8, h_samp=1, v_samp=1)
        v.update(kw)
        for k, x in v.items():
            setattr(im[0], k, x)
        return lib.pam_jpeg_forward(None, n, im)

    assert call() == 0
    for kw in (dict(dev_bgr=None), dict(dev_quant=None), dict(dev_coef=None), dict(dev_quant=base + 1032), dict(dev_coef=base + 2050),
               dict(width=0), dict(height=65536), dict(h_samp=1, v_samp=2), dict(h_samp=4, v_samp=1), dict(h_samp=0, v_samp=0), dict(n=0), dict(n=33)):
        assert call(**kw) == -1, kw
    assert lib.pam_jpeg_forward(None, 1, None) == -1
    torch.cuda.synchronize()
