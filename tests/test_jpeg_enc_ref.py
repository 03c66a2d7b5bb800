"""tests/jpeg_enc_ref.py, the NumPy restatement of the device JPEG encode path, held to Pillow (libjpeg-turbo) with ``==`` on the whole
file: sizes from one pixel to several MCUs with partial MCUs and odd subsampled extents in both directions, the three samplings, seven
qualities from the clamped tables of quality 1 to the all-ones tables of quality 100, noise and smooth content."""
import numpy as np
import pytest

import jpeg_enc_ref as E
import jpeg_ref as J


@pytest.fixture(scope='module')
def cases():
    return E.matrix()


def test_the_matrix_covers_what_it_says(cases):
    assert len(cases) == 13 * 3 * 2 + 3 * 3 * 7
    assert {(c[1].shape[1], c[1].shape[0]) for c in cases} == set(J.SIZES) | {(24, 8), (8, 24)}
    assert {c[2] for c in cases} == {'444', '422', '420'} and {c[3] for c in cases} == {1, 5, 30, 50, 75, 92, 100}


def test_whole_files_equal_pillow_on_the_matrix(cases):
    bad = []
    for tag, bgr, sampling, quality in cases:
        if E.encode_bgr(bgr, sampling, quality) != E.pillow_bytes(bgr, sampling, quality):
            bad.append(tag)
    assert not bad, bad[:10]


def test_the_default_is_what_pillow_writes_without_arguments(tmp_path):
    from PIL import Image
    bgr = np.ascontiguousarray(J.content('smooth', 40, 50, 7)[:, :, ::-1])
    p = str(tmp_path / 'd.jpg')
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(p)
    assert open(p, 'rb').read() == E.encode_bgr(bgr)


def test_coefficients_equal_what_the_decode_side_reads_from_pillow_files(cases):
    """The forward half alone: every real block's coefficients are those in Pillow's file, read by jpeg_ref's parser and Huffman pass;
    the padding blocks are zeros in the restatement (the decode side finds the encoder's dummy blocks there)."""
    for tag, bgr, sampling, quality in cases[::7]:
        data = E.pillow_bytes(bgr, sampling, quality)
        hdr = J.parse(data)
        want = J.entropy(data, hdr)
        tables = E.quality_tables(quality)
        assert np.array_equal(hdr['quant'], tables[[0, 1, 1]]), tag
        got = E.forward(bgr, sampling, tables)
        hs, vs = E.SAMPLINGS[sampling]
        lay = E.layout(bgr.shape[1], bgr.shape[0], hs, vs)
        assert lay['coef_words'] == hdr['coef_words'] and lay['coef_offset'] == hdr['coef_offset']
        for c in range(3):
            n = 64 * lay['blocks_w'][c] * lay['blocks_h'][c]
            a = got[lay['coef_offset'][c]:lay['coef_offset'][c] + n].reshape(lay['blocks_h'][c], lay['blocks_w'][c], 64)
            b = want[lay['coef_offset'][c]:lay['coef_offset'][c] + n].reshape(lay['blocks_h'][c], lay['blocks_w'][c], 64)
            rh, rw = lay['real_h'][c], lay['real_w'][c]
            assert np.array_equal(a[:rh, :rw], b[:rh, :rw]), (tag, c)
            assert not a[rh:].any() and not a[:, rw:].any(), (tag, c)


def test_extreme_frames_stay_inside_the_standard_tables():
    """All-0, all-255 and the 0 / 255 checkerboard, the largest coefficients a frame can give, at the all-ones tables of quality 100."""
    for w, h in ((17, 23), (16, 16)):
        yy, xx = np.mgrid[0:h, 0:w]
        for frame in (np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8),
                      np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)):
            for sampling in E.SAMPLINGS:
                assert E.encode_bgr(frame, sampling, 100) == E.pillow_bytes(frame, sampling, 100)


def test_a_coefficient_without_a_code_is_refused():
    tables = E.quality_tables(75)
    coef = np.zeros(E.layout(8, 8, 1, 1)['coef_words'], dtype=np.int16)
    coef[0] = 2047
    E.encode(coef, 8, 8, '444', tables)
    coef[0] = 2048
    with pytest.raises(E.NoCode):
        E.encode(coef, 8, 8, '444', tables)
    coef[0] = 0; coef[5] = -1023
    E.encode(coef, 8, 8, '444', tables)
    coef[5] = -1024
    with pytest.raises(E.NoCode):
        E.encode(coef, 8, 8, '444', tables)
