"""NumPy restatement of the device JPEG path (a plain helper, imported like image_ref.py; no GPU, no library): a header parser, a
bit-at-a-time Huffman decoder and the reconstruction formulas of include/pam.h -- slow-integer inverse DCT, triangle ("fancy") chroma
upsampling over the true subsampled extents, YCbCr -> BGR.  It shares no code with csrc/pam_jpeg_entropy.hpp or csrc/pam_jpeg.hip;
tests/test_jpeg_ref.py holds it to Pillow byte for byte, and the library and the kernels are then held to it.

The arithmetic is int32 and wraps, as the kernels' does (NumPy's array arithmetic wraps silently), so ``idct`` is defined for any
coefficients, not only those an encoder writes.

``matrix(dir)`` writes the files the tests share, with seeded content: sizes from one pixel to several MCUs in both directions with
partial MCUs and odd subsampled extents, the four samplings, eight qualities, noise and smooth content, optimised Huffman tables and
restart intervals of 1, 3 and 5 MCUs and of one MCU row."""
import os

import numpy as np

# PamJpegInfo.unsupported (include/pam.h)
U_NOT_JPEG, U_PROGRESSIVE, U_ARITHMETIC, U_SOF, U_PRECISION, U_QUANT16, U_COMPONENTS, U_COLORSPACE, U_SAMPLING, U_SCAN, U_DNL = range(1, 12)
INFO_BYTES = 4 * 4 + 6 * 4 + 2 * 4 + 6 * 4 + 2 * 4 + 4 * 8 + 3 * 64 * 2      # sizeof(PamJpegInfo) as the header lays it out

ZIGZAG = np.array([[0, 1, 5, 6, 14, 15, 27, 28], [2, 4, 7, 13, 16, 26, 29, 42], [3, 8, 12, 17, 25, 30, 41, 43],
                   [9, 11, 18, 24, 31, 40, 44, 53], [10, 19, 23, 32, 39, 45, 52, 54], [20, 22, 33, 38, 46, 51, 55, 60],
                   [21, 34, 37, 47, 50, 56, 59, 61], [35, 36, 48, 49, 57, 58, 62, 63]])
NATURAL_OF = np.argsort(ZIGZAG.reshape(-1))          # zigzag position k -> natural (row-major) index


class Corrupt(ValueError):
    pass


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """bytes -> dict: width, height, n_comp, h, v (lists), quant (n_comp, 64) natural order, restart_interval, mcu_w, mcu_h, blocks_w,
    blocks_h, coef_offset, coef_words, unsupported (0 or a U_* code), scan (offset of the entropy-coded bytes), dc / ac (per component:
    dict (length, code) -> symbol).  Corrupt for a broken header."""
    d = bytes(data)
    out = dict(unsupported=0, width=0, height=0, n_comp=0, restart_interval=0)
    if d[:2] != b'\xff\xd8':
        return dict(out, unsupported=U_NOT_JPEG)
    qt, hts, comps, jfif, adobe = {}, {}, None, False, None
    p = 2
    while True:
        if p >= len(d) or d[p] != 0xFF:
            raise Corrupt('marker expected at %d' % p)
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt('cut short')
        m = d[p]; p += 1
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m in (0x00, 0xD9) or p + 2 > len(d):
            raise Corrupt('marker %02x' % m)
        n = _u16(d, p)
        if n < 2 or p + n > len(d):
            raise Corrupt('segment length')
        seg = d[p + 2:p + n]; p += n
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if comps is not None:
                raise Corrupt('two frames')
            if len(seg) >= 5:
                out['height'], out['width'] = _u16(seg, 1), _u16(seg, 3)
            if m != 0xC0:
                return dict(out, unsupported=U_PROGRESSIVE if m == 0xC2 else U_ARITHMETIC if m >= 0xC9 else U_SOF)
            if len(seg) < 6:
                raise Corrupt('frame header')
            if seg[0] != 8:
                return dict(out, unsupported=U_PRECISION)
            nf = seg[5]
            if nf not in (1, 3):
                return dict(out, unsupported=U_COMPONENTS)
            if len(seg) != 6 + 3 * nf or out['width'] == 0:
                raise Corrupt('frame header')
            if out['height'] == 0:
                return dict(out, unsupported=U_DNL)
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)]
            if any(not (1 <= h <= 4 and 1 <= v <= 4 and t <= 3) for _, h, v, t in comps):
                raise Corrupt('sampling factors')
            out['n_comp'] = nf
        elif m == 0xCC:
            return dict(out, unsupported=U_ARITHMETIC)
        elif m == 0xDB:
            o = 0
            while o < len(seg):
                pq, tq = seg[o] >> 4, seg[o] & 15
                if tq > 3 or pq > 1:
                    raise Corrupt('DQT')
                if pq:
                    return dict(out, unsupported=U_QUANT16)
                if len(seg) - o < 65:
                    raise Corrupt('DQT length')
                t = np.zeros(64, dtype=np.int32)
                t[NATURAL_OF] = np.frombuffer(seg[o + 1:o + 65], dtype=np.uint8)
                qt[tq] = t
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                if len(seg) - o < 17:
                    raise Corrupt('DHT length')
                tc, th = seg[o] >> 4, seg[o] & 15
                counts = list(seg[o + 1:o + 17])
                if tc > 1 or th > 3 or sum(counts) > 256 or len(seg) - o - 17 < sum(counts):
                    raise Corrupt('DHT')
                table, code, k = {}, 0, o + 17
                for length, cnt in enumerate(counts, 1):
                    for _ in range(cnt):
                        if code >= 1 << length:
                            raise Corrupt('DHT: not a prefix code')
                        table[(length, code)] = seg[k]
                        code += 1; k += 1
                    code <<= 1
                hts[(tc, th)] = table
                o = k
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt('DRI')
            out['restart_interval'] = _u16(seg, 0)
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b'JFIF\0'
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b'Adobe':
                adobe = seg[11]
        elif m == 0xDC:
            return dict(out, unsupported=U_DNL)
        elif m == 0xDA:
            if comps is None or len(seg) < 1 or not 1 <= seg[0] <= 4 or len(seg) != 4 + 2 * seg[0]:
                raise Corrupt('SOS')
            ns = seg[0]
            if ns != len(comps) or any(seg[1 + 2 * c] != comps[c][0] for c in range(ns)):
                return dict(out, unsupported=U_SCAN)
            tabs = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(ns)]
            if any(a > 3 or b > 3 for a, b in tabs):
                raise Corrupt('SOS tables')
            if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0):
                return dict(out, unsupported=U_SCAN)
            hv = [(h, v) for _, h, v, _ in comps]
            if ns == 1:
                if hv[0] != (1, 1):
                    return dict(out, unsupported=U_SAMPLING)
            else:
                if hv[0] not in ((1, 1), (2, 1), (2, 2)) or hv[1] != (1, 1) or hv[2] != (1, 1):
                    return dict(out, unsupported=U_SAMPLING)
                ids = bytes(c[0] for c in comps)
                if (adobe != 1) if adobe is not None else (not jfif and ids == b'RGB'):
                    return dict(out, unsupported=U_COLORSPACE)
            for c in range(ns):
                if comps[c][3] not in qt or (0, tabs[c][0]) not in hts or (1, tabs[c][1]) not in hts:
                    raise Corrupt('missing table')
            H, V = hv[0]
            mw, mh = -(-out['width'] // (8 * H)), -(-out['height'] // (8 * V))
            bw, bh = [mw * h for h, _ in hv], [mh * v for _, v in hv]
            sizes = [64 * a * b for a, b in zip(bw, bh)]
            out.update(h=[h for h, _ in hv], v=[v for _, v in hv], quant=np.stack([qt[c[3]] for c in comps]), mcu_w=mw, mcu_h=mh,
                       blocks_w=bw, blocks_h=bh, coef_offset=[int(x) for x in np.cumsum([0] + sizes[:-1])], coef_words=int(sum(sizes)),
                       scan=p, dc=[hts[(0, a)] for a, _ in tabs], ac=[hts[(1, b)] for _, b in tabs])
            return out


def _segments(d, p):
    """The entropy-coded bytes from offset p, stuffing removed, split at the restart markers: [(bits as a list of 0 / 1, RSTn index
    that FOLLOWS the segment or None)]."""
    segs, cur = [], bytearray()
    n = len(d)
    while p < n:
        b = d[p]
        if b != 0xFF:
            cur.append(b); p += 1
            continue
        q = p
        while q < n and d[q] == 0xFF:
            q += 1
        if q >= n:
            break
        if d[q] == 0x00 and q == p + 1:
            cur.append(0xFF); p = q + 1
            continue
        if 0xD0 <= d[q] <= 0xD7:
            segs.append((cur, d[q] - 0xD0)); cur = bytearray(); p = q + 1
            continue
        break                                          # any other marker ends the scan
    segs.append((cur, None))
    return [(np.unpackbits(np.frombuffer(bytes(s), dtype=np.uint8)).tolist(), r) for s, r in segs]


class _Bits(object):
    def __init__(self, bits):
        self.bits, self.p = bits, 0

    def bit(self):
        if self.p >= len(self.bits):
            raise Corrupt('entropy-coded data cut short')
        b = self.bits[self.p]; self.p += 1
        return b

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                return s
        raise Corrupt('undefined code')

    def value(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy(data, hdr):
    """The scan -> int16 (coef_words,): quantised coefficients, natural order, 64 per block, block-row-major per component with the
    padding blocks of partial MCUs."""
    d = bytes(data)
    coef = np.zeros(hdr['coef_words'], dtype=np.int16)
    segs = _segments(d, hdr['scan'])
    si, rd = 0, _Bits(segs[0][0])
    pred = [0] * hdr['n_comp']
    ri, done = hdr['restart_interval'], 0
    for my in range(hdr['mcu_h']):
        for mx in range(hdr['mcu_w']):
            if ri and done and done % ri == 0:
                if segs[si][1] != (done // ri - 1) % 8 or si + 1 >= len(segs):
                    raise Corrupt('restart marker')
                si += 1; rd = _Bits(segs[si][0]); pred = [0] * hdr['n_comp']
            done += 1
            for c in range(hdr['n_comp']):
                for v in range(hdr['v'][c]):
                    for h in range(hdr['h'][c]):
                        at = hdr['coef_offset'][c] + 64 * ((my * hdr['v'][c] + v) * hdr['blocks_w'][c] + mx * hdr['h'][c] + h)
                        s = rd.symbol(hdr['dc'][c])
                        if s > 15:
                            raise Corrupt('DC size')
                        if s:
                            pred[c] += rd.value(s)
                        coef[at] = np.int16(((pred[c] + 32768) % 65536) - 32768)
                        k = 1
                        while k < 64:
                            rs = rd.symbol(hdr['ac'][c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 64:
                                    raise Corrupt('run')
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt('run')
                            coef[at + NATURAL_OF[k]] = rd.value(s)
                            k += 1
    return coef


def _pass(x, s):
    """One 1-D pass on the LAST axis of an int32 array (..., 8)."""
    i = np.int32
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., k] for k in range(8)]
    z1 = (x2 + x6) * i(4433)
    t2 = z1 - x6 * i(15137)
    t3 = z1 + x2 * i(6270)
    t0 = (x0 + x4) << i(13)
    t1 = (x0 - x4) << i(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * i(9633)
    a0 = a0 * i(2446); a1 = a1 * i(16819); a2 = a2 * i(25172); a3 = a3 * i(12299)
    z1 = z1 * i(-7373); z2 = z2 * i(-20995)
    z3 = z3 * i(-16069) + z5
    z4 = z4 * i(-3196) + z5
    a0 = a0 + z1 + z3; a1 = a1 + z2 + z4; a2 = a2 + z2 + z3; a3 = a3 + z1 + z4
    outs = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([(o + i(1 << (s - 1))) >> i(s) for o in outs], axis=-1)


def idct(coef, quant):
    """coef (N, 64) integers, quant (64,) -> uint8 (N, 8, 8): dequantise, columns with s = 11, rows with s = 18, + 128, clamp."""
    with np.errstate(over='ignore'):
        x = (np.asarray(coef).astype(np.int32) * np.asarray(quant).astype(np.int32)[None, :]).reshape(-1, 8, 8)
        x = _pass(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # down the columns
        x = _pass(x, 18)                                                # along the rows
        return np.clip(x + np.int32(128), 0, 255).astype(np.uint8)


def planes(coef, hdr):
    """-> per component the uint8 plane at component resolution, padded to whole blocks: (blocks_h * 8, blocks_w * 8)."""
    out = []
    for c in range(hdr['n_comp']):
        bw, bh = hdr['blocks_w'][c], hdr['blocks_h'][c]
        blk = idct(coef[hdr['coef_offset'][c]:hdr['coef_offset'][c] + 64 * bw * bh].reshape(-1, 64), hdr['quant'][c])
        out.append(blk.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def upsample_h2v1(p):
    """(h, w) -> (h, 2 w)"""
    p = p.astype(np.int32)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int32)
    out[:, 2::2] = (3 * p[:, 1:] + p[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * p[:, :-1] + p[:, 1:] + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def upsample_h2v2(p):
    """(h, w) -> (2 h, 2 w)"""
    p = p.astype(np.int32)
    h, w = p.shape
    out = np.empty((2 * h, 2 * w), dtype=np.int32)
    for y in range(2 * h):
        r = y >> 1
        r2 = min(max(r - 1 if y % 2 == 0 else r + 1, 0), h - 1)
        s = 3 * p[r] + p[r2]
        out[y, 2::2] = (3 * s[1:] + s[:-1] + 8) >> 4
        out[y, 1:-1:2] = (3 * s[:-1] + s[1:] + 7) >> 4
        out[y, 0] = (4 * s[0] + 8) >> 4
        out[y, -1] = (4 * s[-1] + 7) >> 4
    return out


def to_bgr(y, cb=None, cr=None):
    y = y.astype(np.int32)
    if cb is None:
        return np.stack([y, y, y], axis=-1).astype(np.uint8)
    cb, cr = cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def reconstruct(coef, hdr):
    """coefficients -> BGR uint8 (H, W, 3)"""
    W, H = hdr['width'], hdr['height']
    pl = planes(coef, hdr)
    if hdr['n_comp'] == 1:
        return to_bgr(pl[0][:H, :W])
    hs, vs = hdr['h'][0], hdr['v'][0]
    w, h = -(-W // hs), -(-H // vs)
    up = {(1, 1): lambda p: p, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(hs, vs)]
    cb, cr = [up(p[:h, :w])[:H, :W] for p in pl[1:]]
    return to_bgr(pl[0][:H, :W], cb, cr)


def decode_bgr(data):
    hdr = parse(data)
    if hdr['unsupported']:
        raise ValueError('unsupported: %d' % hdr['unsupported'])
    return reconstruct(entropy(data, hdr), hdr)


# ---- the shared files

SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (24, 32), (33, 31), (40, 50), (9, 70), (33, 47), (17, 100), (200, 150)]      # (W, H)
SAMPLINGS = ['444', '422', '420', 'grey']
QUALITIES = [1, 5, 50, 85, 88, 90, 92, 100]
_SUB = {'444': 0, '422': 1, '420': 2}


def content(kind, w, h, seed):
    """RGB uint8 (h, w, 3): 'noise', or 'smooth' (gradients and a soft blob, with a little noise)."""
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = rng.uniform(0.5, 3.0, 3)
    img = np.stack([127 + 120 * np.sin(f[0] * xx / max(w, 2) * 3 + yy / max(h, 2)), 255 * xx / max(w - 1, 1) * 0.5 + 255 * yy / max(h - 1, 1) * 0.5,
                    255 * np.exp(-(((xx - w / 2) / (0.3 * w + 1)) ** 2 + ((yy - h / 2) / (0.3 * h + 1)) ** 2) * f[2])], axis=-1)
    return np.clip(img + rng.normal(0, 2, img.shape), 0, 255).astype(np.uint8)


def write_jpeg(path, rgb, sampling, quality, **kw):
    from PIL import Image
    if sampling == 'grey':
        Image.fromarray(rgb[:, :, 1]).save(path, format='JPEG', quality=quality, **kw)
    else:
        Image.fromarray(rgb).save(path, format='JPEG', quality=quality, subsampling=_SUB[sampling], **kw)


def matrix(directory):
    """Writes the shared files into ``directory`` -> [(path, tag)].  Every size x sampling with both contents (qualities cycling through
    the eight), three sizes with partial MCUs x sampling x all eight qualities, optimised tables, restart intervals."""
    directory = str(directory)
    cases, seed = [], 0
    for i, (w, h) in enumerate(SIZES):
        for j, s in enumerate(SAMPLINGS):
            for k, kind in enumerate(('noise', 'smooth')):
                cases.append((w, h, s, QUALITIES[(i + 3 * j + 5 * k) % 8], kind, {}))
    for (w, h) in ((17, 23), (33, 47), (40, 50)):
        for s in SAMPLINGS:
            for q in QUALITIES:
                cases.append((w, h, s, q, 'noise' if q % 2 else 'smooth', {}))
    for (w, h) in ((16, 16), (17, 23), (33, 31), (200, 150)):
        for s in SAMPLINGS:
            cases.append((w, h, s, 85, 'smooth', dict(optimize=True)))
    for (w, h) in ((16, 16), (17, 23), (33, 47)):
        for s in ('420', '444', 'grey'):
            for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=3), dict(restart_marker_blocks=5), dict(restart_marker_rows=1)):
                cases.append((w, h, s, 90, 'noise', kw))
    out = []
    for (w, h, s, q, kind, kw) in cases:
        tag = '%03d_%dx%d_%s_q%d_%s%s' % (seed, w, h, s, q, kind, ''.join('_%s%s' % (k.replace('restart_marker_', 'rst_'), v) for k, v in sorted(kw.items())))
        path = os.path.join(directory, tag + '.jpg')
        write_jpeg(path, content(kind, w, h, seed), s, q, **kw)
        out.append((path, tag))
        seed += 1
    return out


def pillow_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
