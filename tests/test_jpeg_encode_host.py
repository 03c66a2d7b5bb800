"""The host half of the JPEG encode path (csrc/pam_jpeg_encode.hpp through libpam_hip.so; no GPU): pam_jpeg_encode on the restatement's
coefficients against Pillow's bytes on the shared matrix, its stores against the capacity between sentinel bands, and what it refuses."""
import ctypes as C

import numpy as np
import pytest

from pam import _lib
import jpeg_enc_ref as E

BAND = 256
FILL = 0xA7


@pytest.fixture(scope='module')
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ('pam_jpeg_encode', 'pam_jpeg_encode_bound', 'pam_jpeg_quality_tables'):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    return lib


@pytest.fixture(scope='module')
def cases():
    """(tag, w, h, sampling, quality, restatement coefficients, Pillow's bytes)"""
    return [(tag, bgr.shape[1], bgr.shape[0], s, q, E.forward(bgr, s, E.quality_tables(q)), E.pillow_bytes(bgr, s, q))
            for tag, bgr, s, q in E.matrix()]


def bound_of(lib, w, h, sampling):
    hs, vs = E.SAMPLINGS[sampling]
    n = C.c_size_t(0)
    assert lib.pam_jpeg_encode_bound(w, h, hs, vs, C.byref(n)) == 0
    return n.value


def encode(lib, coef, w, h, sampling, quality, capacity, tables=None, coef_words=None):
    """-> (return code, bytes written or None, the two bands still intact)"""
    hs, vs = E.SAMPLINGS.get(sampling, sampling)
    p = _lib.PamJpegEncodeParams(width=w, height=h, h_samp=hs, v_samp=vs, quality=quality)
    if tables is not None:
        for t in range(2):
            for i in range(64):
                p.quant[t][i] = int(tables[t][i])
    buf = np.full(BAND + capacity + BAND, FILL, dtype=np.uint8)
    n = C.c_size_t(0)
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    rc = lib.pam_jpeg_encode(coef.ctypes.data, coef.size if coef_words is None else coef_words, C.byref(p),
                             buf[BAND:].ctypes.data, capacity, C.byref(n))
    intact = bool((buf[:BAND] == FILL).all() and (buf[BAND + capacity:] == FILL).all())
    return rc, (bytes(buf[BAND:BAND + n.value]) if rc == 0 else None), intact


def test_quality_tables_are_the_restatements(lib):
    for q in (1, 5, 30, 49, 50, 75, 92, 100):
        t = np.zeros((2, 64), dtype=np.uint16)
        assert lib.pam_jpeg_quality_tables(q, t.ctypes.data) == 0
        assert np.array_equal(t, E.quality_tables(q)), q
    t = np.zeros((2, 64), dtype=np.uint16)
    assert lib.pam_jpeg_quality_tables(0, t.ctypes.data) == -1 and lib.pam_jpeg_quality_tables(101, t.ctypes.data) == -1
    assert lib.pam_jpeg_quality_tables(75, None) == -1 and not t.any()


def test_files_equal_pillow_at_exactly_the_bound(lib, cases):
    bad = []
    for tag, w, h, s, q, coef, want in cases:
        rc, got, intact = encode(lib, coef, w, h, s, q, bound_of(lib, w, h, s))
        assert intact, tag
        if rc != 0 or got != want:
            bad.append((tag, rc))
    assert not bad, bad[:10]


def test_given_tables_write_the_same_file_as_their_quality(lib, cases):
    for tag, w, h, s, q, coef, want in cases[::5]:
        rc, got, intact = encode(lib, coef, w, h, s, 0, bound_of(lib, w, h, s), tables=E.quality_tables(q))
        assert (rc, intact) == (0, True) and got == want, tag


def test_one_byte_short_of_each_file_is_refused_with_the_bands_intact(lib, cases):
    for tag, w, h, s, q, coef, want in cases:
        rc, got, intact = encode(lib, coef, w, h, s, q, len(want))
        assert (rc, intact) == (0, True) and got == want, tag           # exactly the file's size: taken
        rc, _, intact = encode(lib, coef, w, h, s, q, len(want) - 1)
        assert (rc, intact) == (-1, True), tag
    tag, w, h, s, q, coef, want = cases[40]
    for cap in (0, 1, 2, 100, 622, 623, 624, 625):                       # inside the headers
        rc, _, intact = encode(lib, coef, w, h, s, q, cap)
        assert (rc, intact) == (-1, True), cap


def test_the_bound_holds_for_the_longest_codes(lib):
    """Every AC coefficient +-1023 with alternating sign and a DC that swings by 2047 from block to block: 26 bits per coefficient."""
    for (w, h, s) in ((17, 23, '420'), (24, 8, '444'), (9, 70, '422')):
        hs, vs = E.SAMPLINGS[s]
        lay = E.layout(w, h, hs, vs)
        coef = np.tile(np.where(np.arange(64) % 2, 1023, -1023).astype(np.int16), lay['coef_words'] // 64)
        coef[0::128] = 1023; coef[64::128] = -1023
        tables = E.quality_tables(100)
        want = E.encode(coef, w, h, s, tables)
        rc, got, intact = encode(lib, coef, w, h, s, 100, bound_of(lib, w, h, s))
        assert (rc, intact) == (0, True) and got == want and len(got) <= bound_of(lib, w, h, s)
        assert len(got) > 625 + 190 * (lay['mcu_w'] * lay['mcu_h'] * (hs * vs + 2)) // 2


def test_categories_beyond_the_tables_are_refused(lib):
    w, h, s = 16, 16, '420'
    words = E.layout(w, h, 2, 2)['coef_words']
    cap = bound_of(lib, w, h, s)
    base = np.zeros(words, dtype=np.int16)
    for at, v, ok in ((0, 2047, True), (0, 2048, False), (0, -2047, True), (0, -2048, False), (5, 1023, True), (5, 1024, False),
                      (64 * 4 + 63, -1023, True), (64 * 4 + 63, -1024, False), (64 * 5 + 1, 32767, False), (64 * 5, -32768, False)):
        coef = base.copy(); coef[at] = v
        rc, got, intact = encode(lib, coef, w, h, s, 75, cap)
        assert intact and (rc == 0) == ok, (at, v)
        if ok:
            assert got == E.encode(coef, w, h, s, E.quality_tables(75))
    coef = base.copy(); coef[0] = 1024; coef[64] = -1024                 # each fits, their difference does not
    assert encode(lib, coef, w, h, s, 75, cap)[0] == -1


def test_bad_sizes_samplings_and_arguments_are_refused(lib):
    coef = np.zeros(64 * 6 * 4, dtype=np.int16)
    cap = 1 << 16
    assert encode(lib, coef, 16, 16, '420', 75, cap)[0] == 0
    for kw in (dict(w=0), dict(w=65536), dict(h=0), dict(h=65536), dict(w=-1), dict(s=(1, 2)), dict(s=(2, 4)), dict(s=(4, 1)),
               dict(s=(0, 0)), dict(s=(3, 1)), dict(q=101), dict(q=-1)):
        rc, _, intact = encode(lib, coef, kw.get('w', 16), kw.get('h', 16), kw.get('s', '420'), kw.get('q', 75), cap)
        assert (rc, intact) == (-1, True), kw
        n = C.c_size_t(7)
        if 'q' not in kw:
            hs, vs = E.SAMPLINGS.get(kw.get('s', '420'), kw.get('s'))
            assert lib.pam_jpeg_encode_bound(kw.get('w', 16), kw.get('h', 16), hs, vs, C.byref(n)) == -1 and n.value == 7
    assert lib.pam_jpeg_encode_bound(16, 16, 2, 2, None) == -1
    assert encode(lib, coef, 16, 16, '420', 75, cap, coef_words=64 * 6 - 1)[0] == -1        # fewer words than the layout's
    tables = E.quality_tables(75).copy()
    assert encode(lib, coef, 16, 16, '420', 0, cap, tables=tables)[0] == 0
    for bad in (0, 256):
        t = tables.copy(); t[1, 63] = bad
        assert encode(lib, coef, 16, 16, '420', 0, cap, tables=t)[0] == -1
    p = _lib.PamJpegEncodeParams(width=16, height=16, h_samp=2, v_samp=2, quality=75)
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    for args in ((None, coef.size, C.byref(p), out.ctypes.data, cap, C.byref(n)), (coef.ctypes.data, coef.size, None, out.ctypes.data, cap, C.byref(n)),
                 (coef.ctypes.data, coef.size, C.byref(p), None, cap, C.byref(n)), (coef.ctypes.data, coef.size, C.byref(p), out.ctypes.data, cap, None)):
        assert lib.pam_jpeg_encode(*args) == -1
    assert not out.any()
