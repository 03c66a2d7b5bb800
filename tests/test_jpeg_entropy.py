"""The host entropy pass of the device JPEG path (pam_jpeg_probe / pam_jpeg_entropy in libpam_hip.so; the library loads without a GPU)
against the NumPy restatement (tests/jpeg_ref.py): header fields, every coefficient word of every file of the shared matrix, the struct
size, hostile input (every truncation, seeded corruptions) into a buffer with sentinel bands, and eight threads at once."""
import ctypes as C
import io
import os
import re
import threading

import numpy as np
import pytest

import pam  # noqa: F401
from pam import _lib
import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, SENT = 4096, 0x5A5A


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    return J.matrix(tmp_path_factory.mktemp('jpeg_matrix'))


def _probe(lib, data):
    info = _lib.PamJpegInfo()
    rc = lib.pam_jpeg_probe(data, len(data), C.byref(info))
    return rc, info


def _entropy(lib, data, info, words=None, into=None):
    words = int(info.coef_words) if words is None else words
    coef = np.empty(words, dtype=np.int16) if into is None else into
    rc = lib.pam_jpeg_entropy(data, len(data), C.byref(info), coef.ctypes.data_as(C.c_void_p), words)
    return rc, coef


def test_struct_sizes_match_the_header():
    assert C.sizeof(_lib.PamJpegInfo) == J.INFO_BYTES == 496
    assert C.sizeof(_lib.PamJpegImage) == 4 * 8 + 6 * 4
    hdr = open(os.path.join(ROOT, 'include', 'pam.h')).read()
    body = hdr[hdr.index('typedef struct PamJpegInfo {'):hdr.index('} PamJpegInfo;')]
    names = re.findall(r'\b([a-z_0-9]+)(?:\[[0-9]+\])*[,;]', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert names == [n for n, _ in _lib.PamJpegInfo._fields_]
    for code, name in ((1, 'NOT_JPEG'), (2, 'PROGRESSIVE'), (7, 'COMPONENTS'), (9, 'SAMPLING'), (11, 'DNL')):
        assert re.search(r'#define PAM_JPEG_U_%s %d\b' % (name, code), hdr) and code in _lib.JPEG_UNSUPPORTED
    assert sorted(_lib.JPEG_UNSUPPORTED) == list(range(1, 12))


def test_probe_fields_and_every_coefficient_word_equal_the_restatement(lib, files):
    for path, tag in files:
        data = open(path, 'rb').read()
        ref = J.parse(data)
        rc, info = _probe(lib, data)
        assert rc == 0 and info.unsupported == 0, tag
        n = ref['n_comp']
        assert (info.width, info.height, info.n_comp, info.restart_interval) == (ref['width'], ref['height'], n, ref['restart_interval']), tag
        assert (info.mcu_w, info.mcu_h, info.coef_words) == (ref['mcu_w'], ref['mcu_h'], ref['coef_words']), tag
        for key in ('h_samp', 'v_samp', 'blocks_w', 'blocks_h', 'coef_offset'):
            assert list(getattr(info, key))[:n] == ref[{'h_samp': 'h', 'v_samp': 'v'}.get(key, key)], (tag, key)
        assert np.array_equal(np.ctypeslib.as_array(info.quant)[:n], ref['quant']), tag
        rc, coef = _entropy(lib, data, info)
        assert rc == 0, tag
        want = J.entropy(data, ref)
        assert coef.dtype == want.dtype and np.array_equal(coef, want), (tag, int((coef != want).sum()))


def _bytes(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format='JPEG', **kw)
    return buf.getvalue()


def test_unsupported_files_get_the_restatements_reason_and_are_no_error(lib):
    from PIL import Image
    rgb = Image.fromarray(J.content('smooth', 40, 24, 1))
    base = bytearray(_bytes(rgb, quality=80, subsampling=2))
    sof = base.index(b'\xff\xc0')
    v411, v440, zero_h, p12 = bytearray(base), bytearray(base), bytearray(base), bytearray(base)
    v411[sof + 11] = 0x41; v440[sof + 11] = 0x12; zero_h[sof + 5] = zero_h[sof + 6] = 0; p12[sof + 4] = 12
    png = io.BytesIO(); rgb.save(png, format='PNG')
    cases = [(_bytes(rgb, quality=80, progressive=True), J.U_PROGRESSIVE), (_bytes(rgb.convert('CMYK'), quality=80), J.U_COMPONENTS),
             (bytes(v411), J.U_SAMPLING), (bytes(v440), J.U_SAMPLING), (bytes(zero_h), J.U_DNL), (bytes(p12), J.U_PRECISION),
             (png.getvalue(), J.U_NOT_JPEG), (b'', J.U_NOT_JPEG)]
    for data, why in cases:
        rc, info = _probe(lib, data)
        assert rc == 0 and info.unsupported == why == J.parse(data)['unsupported'], why
        assert _entropy(lib, data, info, words=64)[0] == -1              # and the entropy pass does not take an info that says so


def _hostile_targets(tmp_path):
    """16x16 and 17x23, each as 4:2:0 and as 4:2:0 with a restart marker after every MCU."""
    out = []
    for (w, h) in ((16, 16), (17, 23)):
        for kw in ({}, dict(restart_marker_blocks=1)):
            p = os.path.join(str(tmp_path), 'h_%d_%d_%d.jpg' % (w, h, len(kw)))
            J.write_jpeg(p, J.content('noise', w, h, 7), '420', 90, **kw)
            out.append(open(p, 'rb').read())
    return out


def _guarded(words):
    buf = np.full(words + 2 * BAND, SENT, dtype=np.uint16).view(np.int16)
    return buf, buf[BAND:BAND + words]


def _bands_intact(buf, words):
    u = buf.view(np.uint16)
    return bool((u[:BAND] == SENT).all() and (u[BAND + words:] == SENT).all())


def test_truncation_at_every_byte_and_seeded_corruptions_stay_in_bounds(lib, tmp_path):
    outcomes = {0: 0, -1: 0}
    rng = np.random.default_rng(11)
    targets = _hostile_targets(tmp_path)
    for data in targets:
        rc, info = _probe(lib, data)
        assert rc == 0 and not info.unsupported
        words = int(info.coef_words)
        buf, coef = _guarded(words)
        for cut in range(len(data)):
            piece = data[:cut]
            rc, i2 = _probe(lib, piece)
            assert rc in (0, -1)
            if rc == 0 and not i2.unsupported:
                rc = lib.pam_jpeg_entropy(piece, len(piece), C.byref(i2), coef.ctypes.data_as(C.c_void_p), words)
                assert rc in (0, -1), cut
                outcomes[rc] += 1
                assert rc == -1 or cut >= len(data) - 2, cut             # only the end-of-image marker may be missing
        assert _bands_intact(buf, words)
    for k in range(2000):
        data = bytearray(targets[k % len(targets)])
        data[int(rng.integers(0, len(data)))] = int(rng.integers(0, 256))
        data = bytes(data)
        rc, info = _probe(lib, data)
        assert rc in (0, -1)
        if rc == 0 and not info.unsupported and 0 < info.coef_words <= 1 << 20:
            words = int(info.coef_words)
            buf, coef = _guarded(words)
            rc = lib.pam_jpeg_entropy(data, len(data), C.byref(info), coef.ctypes.data_as(C.c_void_p), words)
            assert rc in (0, -1), k
            outcomes[rc] += 1
            assert _bands_intact(buf, words), k
            # a buffer one word short is refused before anything is written
            buf, coef = _guarded(words - 1)
            assert lib.pam_jpeg_entropy(data, len(data), C.byref(info), coef.ctypes.data_as(C.c_void_p), words - 1) == -1
            assert _bands_intact(buf, words - 1) and (coef.view(np.uint16) == SENT).all()
    assert outcomes[0] > 100 and outcomes[-1] > 100, outcomes             # both outcomes occur: the corpus is not one-sided


def test_an_info_of_another_file_is_refused(lib, files):
    a = open(files[10][0], 'rb').read()
    b = open(files[40][0], 'rb').read()
    _, ia = _probe(lib, a)
    _, ib = _probe(lib, b)
    assert (ia.width, ia.height) != (ib.width, ib.height)
    assert _entropy(lib, a, ib, words=int(max(ia.coef_words, ib.coef_words)))[0] == -1


def test_eight_threads_decode_different_files_at_once(lib, files):
    picks = [files[i] for i in np.linspace(0, len(files) - 1, 8).astype(int)]
    datas = [open(p, 'rb').read() for p, _ in picks]
    single = []
    for d in datas:
        _, info = _probe(lib, d)
        single.append(_entropy(lib, d, info)[1])
    got, errs = [None] * 8, []
    gate = threading.Barrier(8)

    def work(i):
        try:
            gate.wait()
            for _ in range(40):
                rc, info = _probe(lib, datas[i])
                rc2, coef = _entropy(lib, datas[i], info)
                if rc or rc2 or not np.array_equal(coef, single[i]):
                    errs.append(i)
            got[i] = coef
        except Exception as e:                                           # noqa: BLE001
            errs.append((i, repr(e)))

    ts = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for a, b in zip(got, single):
        assert np.array_equal(a, b)
