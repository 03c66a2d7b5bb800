"""NumPy restatement of the device JPEG ENCODE path (a plain helper, imported like jpeg_ref.py; no GPU, no library): libjpeg's default
encoder as include/pam.h states it -- colour conversion, edge replication, chroma downsampling, slow-integer forward DCT, quantisation
into the coefficient layout of the decode -- and the file around them: Pillow's header, the standard Huffman tables, the MCU-interleaved
scan.  It shares no code with csrc/pam_jpeg_fwd.hip or csrc/pam_jpeg_encode.hpp; tests/test_jpeg_enc_ref.py holds it to Pillow with
``==`` on the whole file, and the library and the kernel are then held to it."""
import numpy as np

from jpeg_ref import NATURAL_OF

SAMPLINGS = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}
PILLOW_SUB = {'444': 0, '422': 1, '420': 2}

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                      80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                      95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.full(64, 99)
BASE_CHROMA.reshape(8, 8)[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# Annex K.3 - K.6 as (counts per code length 1 .. 16, symbols in code order)
_DC = [bytes.fromhex('00010501010101010100000000000000'), bytes.fromhex('00030101010101010101010000000000')]
_AC = [bytes.fromhex('0002010303020403050504040000017d'), bytes.fromhex('00020102040403040705040400010277')]
_DC_VALS = bytes(range(12))
_AC_VALS = [bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
    'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'), bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849'
    '4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5'
    'c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')]
assert [len(v) for v in _AC_VALS] == [162, 162] and [sum(b) for b in _AC] == [162, 162]


def quality_tables(quality):
    """-> int (2, 64), natural order: luma, chroma"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (BASE_LUMA, BASE_CHROMA)])


def layout(w, h, hs, vs):
    """The decode's buffer layout for three components: dict(mcu_w, mcu_h, blocks_w, blocks_h, real_w, real_h, coef_offset, coef_words)."""
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    bw, bh = [mw * hs, mw, mw], [mh * vs, mh, mh]
    cw, chh = -(-w // hs), -(-h // vs)
    sizes = [64 * a * b for a, b in zip(bw, bh)]
    return dict(mcu_w=mw, mcu_h=mh, blocks_w=bw, blocks_h=bh, real_w=[-(-w // 8), -(-cw // 8), -(-cw // 8)],
                real_h=[-(-h // 8), -(-chh // 8), -(-chh // 8)], coef_offset=[0, sizes[0], sizes[0] + sizes[1]], coef_words=sum(sizes))


def ycc(bgr):
    b, g, r = [bgr[..., k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _extend(p, rows, cols):
    """Replicates the last row / column of p out to (rows, cols)."""
    return np.pad(p, ((0, max(0, rows - p.shape[0])), (0, max(0, cols - p.shape[1]))), mode='edge')


def component_planes(bgr, hs, vs):
    """BGR uint8 (H, W, 3) -> [Y, Cb, Cr] int64 planes of 8 real_h x 8 real_w samples, edges as libjpeg builds them: input rows out to a
    multiple of vs and columns to the downsampled plane's width first, then the downsampling, then the downsampled rows repeated."""
    h, w = bgr.shape[:2]
    lay = layout(w, h, hs, vs)
    y, cb, cr = ycc(bgr)
    out = [_extend(y, 8 * lay['real_h'][0], 8 * lay['real_w'][0])]
    for p in (cb, cr):
        cols, rows = 8 * lay['real_w'][1], 8 * lay['real_h'][1]
        p = _extend(p, -(-h // vs) * vs, cols * hs)
        if hs == 2:
            bias = np.tile([0, 1] if vs == 1 else [1, 2], cols // 2)[None, :]
            if vs == 1:
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
            else:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_extend(p, rows, cols))
    return out


def _fdct_pass(d, first):
    """One 1-D pass on the LAST axis of an int64 array (..., 8): the row pass (first) or the column pass."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., k] for k in range(8)]
    t0, t1, t2, t3 = d0 + d7, d1 + d6, d2 + d5, d3 + d4
    t7, t6, t5, t4 = d0 - d7, d1 - d6, d2 - d5, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    s = 11 if first else 15
    rnd = lambda v: (v + (1 << (s - 1))) >> s
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else (t10 + t11 + 2) >> 2
    o[4] = (t10 - t11) << 2 if first else (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o[2] = rnd(z1 + t13 * 6270)
    o[6] = rnd(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = rnd(t4 + z1 + z3), rnd(t5 + z2 + z4), rnd(t6 + z2 + z3), rnd(t7 + z1 + z4)
    return np.stack(o, axis=-1)


def fdct_quant(blocks, quant):
    """(N, 8, 8) samples 0 .. 255, quant (64,) -> int64 (N, 64) quantised coefficients, natural order."""
    x = _fdct_pass(blocks.astype(np.int64) - 128, True)
    x = _fdct_pass(x.transpose(0, 2, 1), False).transpose(0, 2, 1).reshape(-1, 64)
    qv = 8 * np.asarray(quant, dtype=np.int64)[None, :]
    return np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)


def forward(bgr, sampling, tables):
    """BGR uint8 (H, W, 3), '444' / '422' / '420', tables int (2, 64) -> int16 (coef_words,) in the decode's layout, padding blocks 0."""
    hs, vs = SAMPLINGS[sampling]
    h, w = bgr.shape[:2]
    lay = layout(w, h, hs, vs)
    coef = np.zeros(lay['coef_words'], dtype=np.int16)
    for c, plane in enumerate(component_planes(bgr, hs, vs)):
        rh, rw = lay['real_h'][c], lay['real_w'][c]
        blocks = plane.reshape(rh, 8, rw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        q = fdct_quant(blocks, tables[min(c, 1)]).reshape(rh, rw, 64)
        view = coef[lay['coef_offset'][c]:lay['coef_offset'][c] + 64 * lay['blocks_w'][c] * lay['blocks_h'][c]]
        view.reshape(lay['blocks_h'][c], lay['blocks_w'][c], 64)[:rh, :rw] = q
    return coef


def _codes(counts, vals):
    """-> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for length, n in enumerate(counts, 1):
        for _ in range(n):
            out[vals[k]] = (code, length)
            code += 1; k += 1
        code <<= 1
    return out


def header(w, h, hs, vs, tables):
    seg = lambda marker, body: bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + body
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2):
        zz = np.asarray(tables[t]).reshape(-1)[NATURAL_OF]
        out += seg(0xDB, bytes([t]) + bytes(int(v) for v in zz))
    out += seg(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        out += seg(0xC4, bytes([t]) + _DC[t] + _DC_VALS)
        out += seg(0xC4, bytes([0x10 | t]) + _AC[t] + _AC_VALS[t])
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class NoCode(ValueError):
    pass


def _value_bits(v, n):
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


def scan(coef, w, h, hs, vs):
    """The entropy-coded bytes of the one interleaved scan, stuffed and padded with one-bits."""
    lay = layout(w, h, hs, vs)
    dc = [_codes(_DC[t], _DC_VALS) for t in range(2)]
    ac = [_codes(_AC[t], _AC_VALS[t]) for t in range(2)]
    bits = []

    def put(code, length):
        bits.append(format(code, '0%db' % length) if length else '')

    pred = [0, 0, 0]
    fac = [(hs, vs), (1, 1), (1, 1)]
    for my in range(lay['mcu_h']):
        for mx in range(lay['mcu_w']):
            for c in range(3):
                t = min(c, 1)
                for v in range(fac[c][1]):
                    for hh in range(fac[c][0]):
                        by, bx = my * fac[c][1] + v, mx * fac[c][0] + hh
                        if bx >= lay['real_w'][c] or by >= lay['real_h'][c]:
                            put(*dc[t][0]); put(*ac[t][0])               # a dummy block: DC difference 0, end of block
                            continue
                        at = lay['coef_offset'][c] + 64 * (by * lay['blocks_w'][c] + bx)
                        zz = [int(x) for x in coef[at:at + 64][NATURAL_OF]]
                        diff = zz[0] - pred[c]
                        pred[c] = zz[0]
                        n = abs(diff).bit_length()
                        if n > 11:
                            raise NoCode('DC difference %d' % diff)
                        put(*dc[t][n]); put(_value_bits(diff, n), n)
                        run = 0
                        for a in zz[1:]:
                            if a == 0:
                                run += 1
                                continue
                            while run > 15:
                                put(*ac[t][0xF0]); run -= 16
                            n = abs(a).bit_length()
                            if n > 10:
                                raise NoCode('AC value %d' % a)
                            put(*ac[t][(run << 4) | n]); put(_value_bits(a, n), n)
                            run = 0
                        if run:
                            put(*ac[t][0])
    s = ''.join(bits)
    s += '1' * (-len(s) % 8)
    raw = int(s, 2).to_bytes(len(s) // 8, 'big') if s else b''
    return raw.replace(b'\xff', b'\xff\x00')


def encode(coef, w, h, sampling, tables):
    hs, vs = SAMPLINGS[sampling]
    return header(w, h, hs, vs, tables) + scan(coef, w, h, hs, vs) + b'\xff\xd9'


def encode_bgr(bgr, sampling='420', quality=75):
    """What Image.fromarray(rgb).save(path, quality=quality, subsampling=...) writes from the same pixels."""
    tables = quality_tables(quality)
    return encode(forward(bgr, sampling, tables), bgr.shape[1], bgr.shape[0], sampling, tables)


def pillow_bytes(bgr, sampling='420', quality=75):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, format='JPEG', quality=quality, subsampling=PILLOW_SUB[sampling])
    return buf.getvalue()


# ---- the shared matrix
SIZES_EXTRA = [(24, 8), (8, 24)]
QUALITIES = [1, 5, 30, 50, 75, 92, 100]


def matrix():
    """[(tag, BGR uint8, sampling, quality)]: every size x sampling with both contents (qualities cycling through the seven), and three
    sizes with partial MCUs x sampling x all seven qualities."""
    import jpeg_ref as J
    cases, seed = [], 0
    sizes = list(J.SIZES) + SIZES_EXTRA
    for i, (w, h) in enumerate(sizes):
        for j, s in enumerate(SAMPLINGS):
            for k, kind in enumerate(('noise', 'smooth')):
                cases.append((w, h, s, QUALITIES[(i + 3 * j + 5 * k) % 7], kind))
    for (w, h) in ((17, 23), (33, 31), (9, 70)):
        for s in SAMPLINGS:
            for q in QUALITIES:
                cases.append((w, h, s, q, 'noise' if q % 2 else 'smooth'))
    out = []
    for (w, h, s, q, kind) in cases:
        rgb = J.content(kind, w, h, 1000 + seed)
        out.append(('%03d_%dx%d_%s_q%d_%s' % (seed, w, h, s, q, kind), np.ascontiguousarray(rgb[:, :, ::-1]), s, q))
        seed += 1
    return out


def write_coef_files(directory):
    """The matrix for tools/jpeg_enc_hostcheck.cpp: per case TAG.coef (five int32 -- width, height, h_samp, v_samp, quality -- then the
    restatement's int16 coefficients) and TAG.jpg (Pillow's bytes from the same pixels) -> number of cases."""
    import os
    n = 0
    for tag, bgr, s, q in matrix():
        hs, vs = SAMPLINGS[s]
        with open(os.path.join(directory, tag + '.coef'), 'wb') as f:
            f.write(np.array([bgr.shape[1], bgr.shape[0], hs, vs, q], dtype='<i4').tobytes())
            f.write(forward(bgr, s, quality_tables(q)).astype('<i2').tobytes())
        with open(os.path.join(directory, tag + '.jpg'), 'wb') as f:
            f.write(pillow_bytes(bgr, s, q))
        n += 1
    return n
