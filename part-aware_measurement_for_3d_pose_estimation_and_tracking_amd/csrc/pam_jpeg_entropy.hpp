// Host half of the device JPEG path: header parse (SOI .. SOS) and the Huffman pass of a baseline file into quantised coefficients.
// Plain C++ with no HIP, no globals and no allocation, so any number of threads may run it at once; pam_jpeg.hip exports it from
// libpam_hip.so and tools/jpeg_hostcheck.cpp compiles it alone under the host sanitizers.  Written from the public definition of
// the format (ITU-T T.81): every read is checked against data + n, every store against coef_words, every table index against its table.
#ifndef PAM_JPEG_ENTROPY_HPP
#define PAM_JPEG_ENTROPY_HPP

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/pam.h"

namespace pamjpeg {

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { LOOK = 9 };        // bits of look-ahead of the fast table

struct Huff {
    uint16_t fast[1 << LOOK];     // (length << 8) | symbol for codes of up to LOOK bits, 0 = longer or undefined
    int32_t maxcode[17];          // largest code of each length, -1 = none
    int32_t valoff[17];           // index of a length's first symbol minus its first code
    uint8_t vals[256];
    int32_t n_vals;
    bool present;
};

// counts[16] + symbols -> tables; false when the counts describe no prefix code
static inline bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* syms, int total) {
    memset(h.fast, 0, sizeof(h.fast));
    memcpy(h.vals, syms, (size_t)total);
    h.n_vals = total;
    int32_t code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        h.valoff[l] = k - code;
        const int cnt = counts[l - 1];
        if (code + cnt > (1 << l)) return false;
        for (int i = 0; i < cnt; ++i, ++code, ++k) {
            if (l <= LOOK) {
                const int lo = code << (LOOK - l), hi = lo + (1 << (LOOK - l));
                for (int e = lo; e < hi; ++e) h.fast[e] = (uint16_t)((l << 8) | syms[k]);
            }
        }
        h.maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[0] = -1;
    h.valoff[0] = 0;
    h.present = true;
    return true;
}

struct Header {
    PamJpegInfo info;
    Huff dc[4], ac[4];
    int td[3], ta[3];
    size_t scan;          // offset of the first entropy-coded byte
};

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// SOI .. SOS.  PAM_OK with info.unsupported = 0 (take the file) or a reason (leave it to another decoder); PAM_E_ARG for a header that
// is cut short or contradicts itself.  With want_tables the Huffman tables are built as well (the entropy pass), else only checked.
static inline int parse(const uint8_t* d, size_t n, Header& H) {
    PamJpegInfo& I = H.info;
    memset(&I, 0, sizeof(I));
    for (int t = 0; t < 4; ++t) H.dc[t].present = H.ac[t].present = false;
    if (!d || n < 2 || d[0] != 0xFF || d[1] != 0xD8) { I.unsupported = PAM_JPEG_U_NOT_JPEG; return PAM_OK; }
    uint16_t q[4][64];
    bool have_q[4] = {false, false, false, false};
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    size_t p = 2;
    for (;;) {
        if (p >= n || d[p] != 0xFF) return PAM_E_ARG;
        while (p < n && d[p] == 0xFF) ++p;          // fill bytes in front of a marker
        if (p >= n) return PAM_E_ARG;
        const int m = d[p++];
        if (m == 0x00) return PAM_E_ARG;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;      // stand-alone markers
        if (m == 0xD9) return PAM_E_ARG;                          // EOI in front of a scan
        if (n - p < 2) return PAM_E_ARG;
        const size_t L = ((size_t)d[p] << 8) | d[p + 1];
        if (L < 2 || L > n - p) return PAM_E_ARG;
        const uint8_t* s = d + p + 2;
        const size_t len = L - 2;
        p += L;
        if (m == 0xC0 || m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) ||
            (m >= 0xCD && m <= 0xCF)) {
            if (sof) return PAM_E_ARG;
            if (len >= 5) { I.height = (s[1] << 8) | s[2]; I.width = (s[3] << 8) | s[4]; }
            if (m != 0xC0) {
                I.unsupported = m == 0xC2 ? PAM_JPEG_U_PROGRESSIVE : m >= 0xC9 ? PAM_JPEG_U_ARITHMETIC : PAM_JPEG_U_SOF;
                return PAM_OK;
            }
            if (len < 6) return PAM_E_ARG;
            const int nf = s[5];
            if (s[0] != 8) { I.unsupported = PAM_JPEG_U_PRECISION; return PAM_OK; }
            if (nf != 1 && nf != 3) { I.unsupported = PAM_JPEG_U_COMPONENTS; return PAM_OK; }
            if (len != (size_t)(6 + 3 * nf) || I.width == 0) return PAM_E_ARG;
            if (I.height == 0) { I.unsupported = PAM_JPEG_U_DNL; return PAM_OK; }
            I.n_comp = nf;
            for (int c = 0; c < nf; ++c) {
                comp_id[c] = s[6 + 3 * c];
                I.h_samp[c] = s[7 + 3 * c] >> 4;
                I.v_samp[c] = s[7 + 3 * c] & 15;
                comp_tq[c] = s[8 + 3 * c];
                if (I.h_samp[c] < 1 || I.h_samp[c] > 4 || I.v_samp[c] < 1 || I.v_samp[c] > 4 || comp_tq[c] > 3) return PAM_E_ARG;
            }
            sof = true;
        } else if (m == 0xCC) {
            I.unsupported = PAM_JPEG_U_ARITHMETIC;
            return PAM_OK;
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < len) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3 || pq > 1) return PAM_E_ARG;
                if (pq == 1) { I.unsupported = PAM_JPEG_U_QUANT16; return PAM_OK; }
                if (len - o < 65) return PAM_E_ARG;
                for (int k = 0; k < 64; ++k) q[tq][kNatural[k]] = s[o + 1 + k];
                have_q[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < len) {
                if (len - o < 17) return PAM_E_ARG;
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return PAM_E_ARG;
                int total = 0;
                for (int k = 0; k < 16; ++k) total += s[o + 1 + k];
                if (total > 256 || len - o - 17 < (size_t)total) return PAM_E_ARG;
                if (!build_huff(tc ? H.ac[th] : H.dc[th], s + o + 1, s + o + 17, total)) return PAM_E_ARG;
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (len != 2) return PAM_E_ARG;
            I.restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (len >= 5 && !memcmp(s, "JFIF", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (len >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDC) {
            I.unsupported = PAM_JPEG_U_DNL;
            return PAM_OK;
        } else if (m == 0xDA) {
            if (!sof || len < 1) return PAM_E_ARG;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || len != (size_t)(4 + 2 * ns)) return PAM_E_ARG;
            if (ns != I.n_comp) { I.unsupported = PAM_JPEG_U_SCAN; return PAM_OK; }
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) { I.unsupported = PAM_JPEG_U_SCAN; return PAM_OK; }
                H.td[c] = s[2 + 2 * c] >> 4;
                H.ta[c] = s[2 + 2 * c] & 15;
                if (H.td[c] > 3 || H.ta[c] > 3) return PAM_E_ARG;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) { I.unsupported = PAM_JPEG_U_SCAN; return PAM_OK; }
            if (I.n_comp == 1) {
                if (I.h_samp[0] != 1 || I.v_samp[0] != 1) { I.unsupported = PAM_JPEG_U_SAMPLING; return PAM_OK; }
            } else {
                const int h = I.h_samp[0], v = I.v_samp[0];
                const bool luma = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
                if (!luma || I.h_samp[1] != 1 || I.v_samp[1] != 1 || I.h_samp[2] != 1 || I.v_samp[2] != 1) {
                    I.unsupported = PAM_JPEG_U_SAMPLING;
                    return PAM_OK;
                }
                // what the three components mean: an Adobe marker says so; without one and without JFIF, ids 'R','G','B' mean RGB
                const bool rgb_ids = comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B';
                if (adobe ? adobe_transform != 1 : (!jfif && rgb_ids)) { I.unsupported = PAM_JPEG_U_COLORSPACE; return PAM_OK; }
            }
            for (int c = 0; c < I.n_comp; ++c) {
                if (!have_q[comp_tq[c]] || !H.dc[H.td[c]].present || !H.ac[H.ta[c]].present) return PAM_E_ARG;
                for (int k = 0; k < 64; ++k) I.quant[c][k] = q[comp_tq[c]][k];
            }
            I.mcu_w = ceil_div(I.width, 8 * I.h_samp[0]);
            I.mcu_h = ceil_div(I.height, 8 * I.v_samp[0]);
            int64_t off = 0;
            for (int c = 0; c < I.n_comp; ++c) {
                I.blocks_w[c] = I.mcu_w * I.h_samp[c];
                I.blocks_h[c] = I.mcu_h * I.v_samp[c];
                I.coef_offset[c] = off;
                off += (int64_t)64 * I.blocks_w[c] * I.blocks_h[c];
            }
            I.coef_words = off;
            H.scan = p;
            return PAM_OK;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

// MSB-first bit reader over the entropy-coded segment: removes the stuffed zero after FF, stops at a marker and feeds zeros from
// there on (pad counts them, so a caller can tell whether any were used).
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;       // the top `n` bits are valid
    int n;
    int pad;            // how many of the lowest valid bits are made-up zeros

    inline void fill() {
        if (n <= 32 && end - p >= 4) {
            const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            if (!((~w - 0x01010101u) & w & 0x80808080u) && !pad) {        // no FF among the four (may say yes wrongly: then bytewise)
                buf |= (uint64_t)w << (32 - n);
                n += 32;
                p += 4;
                return;
            }
        }
        while (n <= 56) {
            uint32_t b = 0;
            if (pad || p >= end) {
                pad += 8;
            } else if (*p != 0xFF) {
                b = *p++;
            } else if (end - p >= 2 && p[1] == 0x00) {
                b = 0xFF;
                p += 2;
            } else {
                pad += 8;                                                // a marker (or FF as the last byte): stay in front of it
            }
            buf |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(buf >> (64 - k)); }
    inline void drop(int k) { buf <<= k; n -= k; }
    inline bool used_padding() const { return n < pad; }
};

static inline int decode_symbol(Bits& b, const Huff& h) {
    const uint16_t e = h.fast[b.peek(LOOK)];
    if (e) {
        b.drop(e >> 8);
        return e & 255;
    }
    const uint32_t c16 = b.peek(16);
    for (int l = LOOK + 1; l <= 16; ++l) {
        const int32_t c = (int32_t)(c16 >> (16 - l));
        if (c <= h.maxcode[l]) {
            const int32_t idx = h.valoff[l] + c;
            if (idx < 0 || idx >= h.n_vals) return -1;
            b.drop(l);
            return h.vals[idx];
        }
    }
    return -1;                                                           // no code starts like this
}

static inline int32_t receive_extend(Bits& b, int s) {
    const int32_t v = (int32_t)b.peek(s);                                // 1 <= s <= 15
    b.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline bool same_layout(const PamJpegInfo& a, const PamJpegInfo& b) {
    if (a.width != b.width || a.height != b.height || a.n_comp != b.n_comp || a.coef_words != b.coef_words ||
        a.restart_interval != b.restart_interval || a.mcu_w != b.mcu_w || a.mcu_h != b.mcu_h)
        return false;
    for (int c = 0; c < a.n_comp; ++c)
        if (a.h_samp[c] != b.h_samp[c] || a.v_samp[c] != b.v_samp[c] || a.coef_offset[c] != b.coef_offset[c]) return false;
    return true;
}

static inline int probe(const uint8_t* d, size_t n, PamJpegInfo* info) {
    if (!info) return PAM_E_ARG;
    Header H;
    const int rc = parse(d, n, H);
    *info = H.info;
    return rc;
}

// The scan of a file `probe` took -> coef[0 .. info->coef_words).  Everything is zeroed first, so a stream that ends early leaves
// zeros (and PAM_E_ARG).
static inline int entropy(const uint8_t* d, size_t n, const PamJpegInfo* info, int16_t* coef, size_t coef_words) {
    if (!d || !info || !coef) return PAM_E_ARG;
    Header H;
    const int rc = parse(d, n, H);
    if (rc != PAM_OK) return rc;
    const PamJpegInfo& I = H.info;
    if (I.unsupported || info->unsupported || !same_layout(I, *info)) return PAM_E_ARG;
    if (I.coef_words < 0 || (uint64_t)I.coef_words > (uint64_t)coef_words) return PAM_E_ARG;
    memset(coef, 0, (size_t)I.coef_words * sizeof(int16_t));
    Bits b;
    b.p = d + H.scan;
    b.end = d + n;
    b.buf = 0;
    b.n = 0;
    b.pad = 0;
    int32_t pred[3] = {0, 0, 0};
    const int64_t n_mcu = (int64_t)I.mcu_w * I.mcu_h;
    int64_t until_restart = I.restart_interval ? I.restart_interval : n_mcu + 1;
    int next_rst = 0;
    int64_t mcu = 0;
    for (int my = 0; my < I.mcu_h; ++my) {
        for (int mx = 0; mx < I.mcu_w; ++mx, ++mcu) {
            if (until_restart == 0) {
                // the interval is over: whatever is left of the last byte is padding, then FF.. RSTn
                if (b.used_padding()) return PAM_E_ARG;
                if (b.n - b.pad >= 8) return PAM_E_ARG;                   // whole unread bytes in front of the marker
                const uint8_t* q = b.p;
                if (q >= b.end || *q != 0xFF) return PAM_E_ARG;
                while (q < b.end && *q == 0xFF) ++q;
                if (q >= b.end || *q != 0xD0 + next_rst) return PAM_E_ARG;
                b.p = q + 1;
                b.buf = 0;
                b.n = 0;
                b.pad = 0;
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                until_restart = I.restart_interval;
            }
            --until_restart;
            for (int c = 0; c < I.n_comp; ++c) {
                const Huff& hd = H.dc[H.td[c]];
                const Huff& ha = H.ac[H.ta[c]];
                for (int v = 0; v < I.v_samp[c]; ++v) {
                    for (int h = 0; h < I.h_samp[c]; ++h) {
                        const int64_t by = (int64_t)my * I.v_samp[c] + v, bx = (int64_t)mx * I.h_samp[c] + h;
                        const int64_t at = I.coef_offset[c] + (by * I.blocks_w[c] + bx) * 64;
                        if (at < 0 || at + 64 > I.coef_words) return PAM_E_ARG;
                        int16_t* blk = coef + at;
                        b.fill();
                        int s = decode_symbol(b, hd);
                        if (s < 0 || s > 15) return PAM_E_ARG;
                        if (s) pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)receive_extend(b, s));
                        blk[0] = (int16_t)(uint16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            b.fill();
                            const int rs = decode_symbol(b, ha);
                            if (rs < 0) return PAM_E_ARG;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (!s) {
                                if (r != 15) break;                      // end of block
                                k += 16;
                                if (k > 64) return PAM_E_ARG;
                                continue;
                            }
                            k += r;
                            if (k > 63) return PAM_E_ARG;                 // the run leaves the block
                            blk[kNatural[k]] = (int16_t)receive_extend(b, s);
                            ++k;
                        }
                    }
                }
            }
        }
    }
    return b.used_padding() ? PAM_E_ARG : PAM_OK;
}

}  // namespace pamjpeg
#endif
