"""The NumPy restatement of the device JPEG path (tests/jpeg_ref.py) against Pillow, byte for byte, on the shared matrix of files; and
the files it must refuse.  No GPU, no library."""
import io

import numpy as np
import pytest

import jpeg_ref as J


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return J.matrix(tmp_path_factory.mktemp('jpeg_matrix'))


def test_the_matrix_covers_what_it_says(files):
    tags = [t for _, t in files]
    assert len(files) >= 200 and len(set(tags)) == len(tags)
    for w, h in J.SIZES:
        for s in J.SAMPLINGS:
            assert any('_%dx%d_%s_' % (w, h, s) in t for t in tags), (w, h, s)
    for q in J.QUALITIES:
        assert any('_q%d_' % q in t for t in tags)
    assert any('optimize' in t for t in tags) and any('rst_blocks' in t for t in tags) and any('rst_rows' in t for t in tags)
    hdrs = [J.parse(open(p, 'rb').read()) for p, _ in files]
    assert {(h['n_comp'], h['h'][0], h['v'][0]) for h in hdrs} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert {h['restart_interval'] for h in hdrs} >= {0, 1, 3, 5}
    assert not any(h['unsupported'] for h in hdrs)


def test_restatement_equals_pillow_in_every_byte(files):
    bad = []
    for path, tag in files:
        got = J.decode_bgr(open(path, 'rb').read())
        want = J.pillow_bgr(path)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((tag, got.shape, want.shape, int((got.astype(int) - want).__abs__().max()) if got.shape == want.shape else -1))
    assert not bad, bad[:10]


def _jpeg_bytes(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format='JPEG', **kw)
    return buf.getvalue()


def test_progressive_cmyk_and_411_are_refused_with_a_reason():
    from PIL import Image
    rgb = Image.fromarray(J.content('smooth', 40, 24, 1))
    assert J.parse(_jpeg_bytes(rgb, quality=80, progressive=True))['unsupported'] == J.U_PROGRESSIVE
    assert J.parse(_jpeg_bytes(rgb.convert('CMYK'), quality=80))['unsupported'] == J.U_COMPONENTS
    d = bytearray(_jpeg_bytes(rgb, quality=80, subsampling=2))
    sof = d.index(b'\xff\xc0')
    assert d[sof + 11] == 0x22                       # the luma sampling byte of a 4:2:0 frame header
    d[sof + 11] = 0x41                               # ... declared 4:1:1 (Pillow cannot write one)
    assert J.parse(bytes(d))['unsupported'] == J.U_SAMPLING
    d[sof + 11] = 0x12                               # 4:4:0
    assert J.parse(bytes(d))['unsupported'] == J.U_SAMPLING
    assert J.parse(b'\x89PNG\r\n\x1a\n' + bytes(40))['unsupported'] == J.U_NOT_JPEG
    with pytest.raises(ValueError):
        J.decode_bgr(_jpeg_bytes(rgb, quality=80, progressive=True))
