"""The device half of the JPEG path (csrc/pam_jpeg.hip) on a real MI355X: k_jpeg_idct alone against the restatement's idct, the whole
reconstruction against Pillow on the shared matrix of files, both into sentinel-filled, banded memory, one launch pair over images of
different sizes and samplings, and FrameLoader(device_decode=True) against LoadImages with files that fall back.

Memory: guarded_mem's arena hands out bf16 activations and counts unwritten int16 sentinels, which a uint8 frame can hold by chance,
so the bands here are local (``Banded``, with guarded_mem's band width and alignment) and "every byte is written" is shown by
running under two different fills: a byte that is never written holds a different value in the two runs, so it cannot equal the
reference in both."""
import ctypes as C
import os

import numpy as np
import pytest

import pam
from pam import _lib
import guarded_mem as GM
import jpeg_ref as J
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu
BAND = 2 * GM.GUARD              # bytes on each side
FILLS = (0xE5, 0x1A)             # complementary bytes


@pytest.fixture(scope='module')
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return J.matrix(tmp_path_factory.mktemp('jpeg_matrix'))


class Banded(object):
    """nbytes of device memory at a 256-byte-aligned address between two bands of at least BAND bytes of `fill`; the band behind begins
    at the payload's last byte + 1.  The payload starts out as `fill` too."""

    def __init__(self, torch, nbytes, fill):
        raw = torch.empty(nbytes + 2 * BAND + GM.ALIGN, dtype=torch.uint8, device='cuda:0')
        self.start = BAND + (-(raw.data_ptr() + BAND)) % GM.ALIGN
        self.raw, self.nbytes, self.fill = raw[:self.start + nbytes + BAND], nbytes, fill
        self.raw.fill_(fill)
        self.payload = self.raw[self.start:self.start + nbytes]
        assert self.payload.data_ptr() % GM.ALIGN == 0

    def damaged(self):
        """Bytes of the two bands that no longer hold the fill."""
        return int((self.raw[:self.start] != self.fill).sum() + (self.raw[self.start + self.nbytes:] != self.fill).sum())


def host_pass(lib, data):
    """File bytes -> (PamJpegInfo, int16 coefficients) through the library's host entropy pass."""
    info = _lib.PamJpegInfo()
    assert lib.pam_jpeg_probe(data, len(data), C.byref(info)) == 0 and not info.unsupported
    coef = np.empty(int(info.coef_words), dtype=np.int16)
    assert lib.pam_jpeg_entropy(data, len(data), C.byref(info), coef.ctypes.data_as(C.c_void_p), coef.size) == 0
    return info, coef


def item_of(info, coef):
    """What ``run`` takes per image: (W, H, n_comp, hs, vs, quant uint16 (3, 64), coef int16)."""
    return (info.width, info.height, info.n_comp, info.h_samp[0], info.v_samp[0], np.ctypeslib.as_array(info.quant).copy(), coef)


def run(torch, lib, items, fill):
    """One pam_jpeg_reconstruct over `items` with coefficients, planes and frames each in banded memory of `fill`.
    -> (frames [uint8 (H, W, 3)], planes [uint8 (words,)], damaged band bytes over all buffers)."""
    images = (_lib.PamJpegImage * len(items))()
    bufs = []
    for im, (W, H, n, hs, vs, quant, coef) in zip(images, items):
        src = Banded(torch, 512 + 2 * coef.size, fill)                   # [3 x 64 quantisation words | padding to 512 bytes | coefficients]
        head = np.zeros(256, dtype=np.uint16); head[:192] = quant.reshape(-1)
        src.payload.copy_(torch.from_numpy(np.concatenate([head.view(np.int16), coef]).view(np.uint8)))
        planes, out = Banded(torch, coef.size, fill), Banded(torch, H * W * 3, fill)
        im.dev_quant, im.dev_coef = src.payload.data_ptr(), src.payload.data_ptr() + 512
        im.dev_planes, im.dev_out = planes.payload.data_ptr(), out.payload.data_ptr()
        im.width, im.height, im.n_comp, im.h_samp, im.v_samp = W, H, n, hs, vs
        bufs.append((src, planes, out))
    assert lib.pam_jpeg_reconstruct(None, len(items), images) == 0
    torch.cuda.synchronize()
    frames = [out.payload.cpu().numpy().reshape(it[1], it[0], 3) for (_, _, out), it in zip(bufs, items)]
    plane_bytes = [planes.payload.cpu().numpy() for _, planes, _ in bufs]
    return frames, plane_bytes, sum(b.damaged() for trio in bufs for b in trio)


def idct_on_device(torch, lib, coef, quant, bw):
    """(N, 64) coefficients as a one-component image of bw blocks per row -> k_jpeg_idct's plane as (N, 8, 8), read from the scratch."""
    n = coef.shape[0]
    assert n % bw == 0
    bh = n // bw
    q3 = np.zeros((3, 64), dtype=np.uint16); q3[0] = quant
    got = None
    for fill in FILLS:
        _, planes, damaged = run(torch, lib, [(8 * bw, 8 * bh, 1, 1, 1, q3, coef.astype(np.int16).reshape(-1))], fill)
        assert damaged == 0
        blocks = planes[0].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(n, 8, 8)
        assert got is None or np.array_equal(got, blocks)                # whatever the scratch held before
        got = blocks
    return got


STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])


def test_idct_dc_only_blocks_are_exact(torch, lib):
    dc = np.arange(-1024, 1024, 13)                                      # 158 blocks: five workgroups, the last one partly empty
    dc = dc[:154]                                                        # 154 = 7 x 22
    coef = np.zeros((dc.size, 64), dtype=np.int64); coef[:, 0] = dc
    for quant in (np.ones(64, dtype=np.int64), STD_LUMA):
        coef_q = coef.copy(); coef_q[:, 0] = dc // quant[0]
        got = idct_on_device(torch, lib, coef_q, quant, 7)
        assert np.array_equal(got, J.idct(coef_q, quant))
        assert (got == got[:, :1, :1]).all() and len(np.unique(got)) > 50      # flat blocks, many levels


def test_idct_one_ac_term_at_each_position_and_sign_is_exact(torch, lib):
    blocks = []
    for k in range(1, 64):
        for sign in (1, -1):
            for mag, dcv in ((1, 0), (9, 3), (40, -20)):
                b = np.zeros(64, dtype=np.int64); b[k] = sign * mag; b[0] = dcv
                blocks.append(b)
    coef = np.stack(blocks)                                              # 378 = 14 x 27
    for quant in (np.ones(64, dtype=np.int64), STD_LUMA):
        got = idct_on_device(torch, lib, coef, quant, 14)
        want = J.idct(coef, quant)
        assert np.array_equal(got, want), np.argwhere((got != want).any(axis=(1, 2)))[:5]
    assert len(np.unique(want)) > 50


def test_idct_dense_random_blocks_and_a_table_of_255_are_exact(torch, lib):
    rng = np.random.default_rng(5)
    # what an encoder can write for this table (|coef * quant| <= 1024 or so), then the same blocks under a table of all 255 with
    # coefficients an encoder could write for THAT, then values no encoder writes: int32 arithmetic that wraps, equally on both sides
    scale = np.maximum(1024 // STD_LUMA, 1)
    enc = rng.integers(-scale, scale + 1, (165, 64))
    got = idct_on_device(torch, lib, enc, STD_LUMA, 11)
    assert np.array_equal(got, J.idct(enc, STD_LUMA)) and 0 in got and 255 in got
    q255 = np.full(64, 255, dtype=np.int64)
    small = rng.integers(-4, 5, (165, 64))
    got = idct_on_device(torch, lib, small, q255, 11)
    assert np.array_equal(got, J.idct(small, q255)) and len(np.unique(got)) > 200
    wild = rng.integers(-32768, 32768, (165, 64))
    got = idct_on_device(torch, lib, wild, q255, 11)
    assert np.array_equal(got, J.idct(wild, q255))


def test_whole_reconstruction_equals_pillow_on_the_matrix(torch, lib, files):
    """Every file of the matrix, 32 images to a launch pair (sizes and samplings mixed as the matrix orders them)."""
    bad = []
    for lo in range(0, len(files), 32):
        part = files[lo:lo + 32]
        items = [item_of(*host_pass(lib, open(p, 'rb').read())) for p, _ in part]
        frames, _, damaged = run(torch, lib, items, FILLS[(lo // 32) % 2])
        assert damaged == 0
        for (p, tag), got in zip(part, frames):
            want = J.pillow_bgr(p)
            if got.shape != want.shape or not np.array_equal(got, want):
                bad.append((tag, int((got != want).sum())))
    assert not bad, bad[:10]


def test_a_1032x776_420_frame_equals_pillow(torch, lib, tmp_path):
    """The Shelf frame size: 776 rows are 48.5 MCU rows, 1032 columns 64.5 MCUs; 19 110 blocks, 783 workgroups of the colour pass."""
    rgb = J.content('smooth', 1032, 776, 3)
    rgb = np.clip(rgb.astype(np.int16) + np.random.default_rng(4).integers(-24, 25, rgb.shape), 0, 255).astype(np.uint8)
    p = str(tmp_path / 'shelf.jpg')
    J.write_jpeg(p, rgb, '420', 92)
    info, coef = host_pass(lib, open(p, 'rb').read())
    assert (info.mcu_w, info.mcu_h, info.blocks_h[0]) == (65, 49, 98)
    want = J.pillow_bgr(p)
    for fill in FILLS:
        frames, _, damaged = run(torch, lib, [item_of(info, coef)], fill)
        assert damaged == 0 and np.array_equal(frames[0], want)


@pytest.mark.parametrize('sampling', J.SAMPLINGS)
def test_every_byte_is_written_nothing_outside_and_the_scratch_does_not_matter(torch, lib, tmp_path, sampling):
    """1x1; exactly one block / one MCU; partial MCUs in both directions with odd subsampled extents; one block row."""
    for i, (w, h) in enumerate(((1, 1), (8, 8), (16, 16), (17, 23), (33, 31), (9, 70))):
        p = str(tmp_path / ('m_%d.jpg' % i))
        J.write_jpeg(p, J.content('noise' if i % 2 else 'smooth', w, h, 20 + i), sampling, 88)
        data = open(p, 'rb').read()
        info, coef = host_pass(lib, data)
        want = J.pillow_bgr(p)
        hdr = J.parse(data)
        want_planes = np.concatenate([pl.reshape(-1) for pl in J.planes(J.entropy(data, hdr), hdr)])
        for fill in FILLS:
            frames, planes, damaged = run(torch, lib, [item_of(info, coef)], fill)
            assert damaged == 0, (w, h, fill)
            assert np.array_equal(frames[0], want), (w, h, fill)          # under both fills: no byte of the frame is left as it was
            assert np.array_equal(planes[0], want_planes), (w, h, fill)   # the padding blocks too: the scratch is written in full


def test_one_launch_pair_over_three_different_images_equals_three_calls(torch, lib, tmp_path):
    specs = [(33, 31, 'grey', 90), (40, 50, '444', 85), (17, 100, '420', 50)]
    items, wants = [], []
    for i, (w, h, s, q) in enumerate(specs):
        p = str(tmp_path / ('t_%d.jpg' % i))
        J.write_jpeg(p, J.content('smooth', w, h, 40 + i), s, q)
        items.append(item_of(*host_pass(lib, open(p, 'rb').read())))
        wants.append(J.pillow_bgr(p))
    assert [(it[2], it[3], it[4]) for it in items] == [(1, 1, 1), (3, 1, 1), (3, 2, 2)]
    together, planes_t, damaged = run(torch, lib, items, FILLS[0])
    assert damaged == 0
    for k, it in enumerate(items):
        single, planes_s, damaged = run(torch, lib, [it], FILLS[1])
        assert damaged == 0
        assert np.array_equal(together[k], single[0]) and np.array_equal(planes_t[k], planes_s[0])
        assert np.array_equal(together[k], wants[k])


def test_reconstruct_refuses_what_it_cannot_run_before_any_launch(torch, lib):
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda:0')
    base = buf.data_ptr()

    def call(n=1, **kw):
        im = (_lib.PamJpegImage * 1)()
        v = dict(dev_coef=base, dev_quant=base + 1024, dev_planes=base + 2048, dev_out=base + 3072, width=8, height=8, n_comp=1, h_samp=1, v_samp=1)
        v.update(kw)
        for k, x in v.items():
            setattr(im[0], k, x)
        return lib.pam_jpeg_reconstruct(None, n, im)

    assert call() == 0
    for kw in (dict(dev_coef=None), dict(dev_out=None), dict(dev_coef=base + 8), dict(dev_planes=base + 2052), dict(dev_out=base + 3073),
               dict(width=0), dict(height=65536), dict(n_comp=2), dict(n_comp=4), dict(h_samp=2), dict(n_comp=3, h_samp=1, v_samp=2),
               dict(n_comp=3, h_samp=4, v_samp=1), dict(n=0), dict(n=33)):
        assert call(**kw) == -1, kw
    assert lib.pam_jpeg_reconstruct(None, 1, None) == -1
    torch.cuda.synchronize()


N_FRAMES = 23


def _dataset(tmp_path, mixed):
    """Four cameras of different sizes and samplings, 23 frames.  mixed: Camera3 serves a progressive JPEG on frames 0, 3, 6, ... and a
    PNG (under the same extension) on frames 1, 4, 7, ...; else baseline files only.  -> (file names, files that fall back)."""
    from PIL import Image
    from pam.dataset import LoadFilenames
    rng = np.random.default_rng(1)
    cams = {'Camera0': (32, 24, '420'), 'Camera1': (20, 30, '444'), 'Camera2': (17, 23, 'grey'), 'Camera3': (40, 26, '422')}
    fallbacks = 0
    for cam, (w, h, s) in cams.items():
        os.makedirs(tmp_path / cam)
        for i in range(N_FRAMES):
            rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            p = str(tmp_path / cam / ('%03d.jpg' % i))
            if mixed and cam == 'Camera3' and i % 3 == 0:
                Image.fromarray(rgb).save(p, format='JPEG', quality=90, progressive=True); fallbacks += 1
            elif mixed and cam == 'Camera3' and i % 3 == 1:
                Image.fromarray(rgb).save(p, format='PNG'); fallbacks += 1
            else:
                J.write_jpeg(p, rgb, s, 90)
    ds = pam.dataset.AttrDict(dict(ROOT=str(tmp_path), FOLDERS_ORDER=list(cams), DATA_FORMAT='*.jpg'))
    return LoadFilenames(ds), fallbacks


@pytest.mark.parametrize('mixed', [False, True])
def test_frame_loader_device_decode_matches_loadimages_and_counts_its_fallbacks(torch, tmp_path, mixed):
    """A run longer than the ring (depth + 1 = 4 slots, 23 frames), every tensor kept until the end.  With baseline files only nothing
    may fall back, so a loader that quietly takes the Pillow path everywhere fails."""
    from pam.dataset import LoadImages
    from pam.ingest import FrameLoader
    files, n_fallback = _dataset(tmp_path, mixed)
    assert n_fallback == (16 if mixed else 0)
    loader = FrameLoader('Shelf', files, workers=4, depth=3, device=torch.device('cuda:0'), device_decode=True)
    kept, seen = [], []
    with recorded_calls() as calls:
        for idx, imgs, ts in loader:
            kept.append(imgs)
            seen.append(idx)
    loader.close()
    torch.cuda.synchronize()
    assert seen == list(range(N_FRAMES))
    for idx, imgs in zip(seen, kept):
        ref, _ = LoadImages('Shelf', files[idx])
        assert len(imgs) == 4
        for a, b in zip(imgs, ref):
            assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b), idx
    assert (loader.fallbacks, loader.device_decoded) == (n_fallback, 4 * N_FRAMES - n_fallback)
    assert calls.count('pam_jpeg_probe') == 4 * N_FRAMES and calls.count('pam_jpeg_entropy') == 4 * N_FRAMES - n_fallback
    assert calls.count('pam_jpeg_reconstruct') == N_FRAMES               # one launch pair per frame set


def test_the_default_loader_makes_none_of_the_new_calls(torch, tmp_path):
    from pam.dataset import LoadImages
    from pam.ingest import FrameLoader
    files, _ = _dataset(tmp_path, False)
    dev = torch.device('cuda:0')
    with recorded_calls() as calls:
        for kw in (dict(device=dev), dict(device=dev, device_decode=False), dict(), dict(device_decode=True)):     # no device: nothing to decode on
            loader = FrameLoader('Shelf', files, workers=2, depth=2, **kw)
            for idx, imgs, ts in loader:
                if idx == 5:
                    ref, _ = LoadImages('Shelf', files[idx])
                    assert all(np.array_equal(a.cpu().numpy() if kw.get('device') else a, b) for a, b in zip(imgs, ref))
            loader.close()
            assert loader.device_decoded == 0 and loader.fallbacks == 0 and not loader.device_decode
    torch.cuda.synchronize()
    assert calls == []                                                   # the Pillow path calls nothing in the library at all
