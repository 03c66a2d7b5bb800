// Host half of the device JPEG ENCODE: quantised coefficients (PamJpegInfo's layout, as pam_jpeg_forward writes them) -> a complete
// baseline JFIF file with the standard Huffman tables, the file libjpeg's default encoder writes.  Plain C++ with no HIP, no globals
// and no allocation, so any number of threads may run it at once; pam_jpeg_fwd.hip exports it from libpam_hip.so and
// tools/jpeg_enc_hostcheck.cpp compiles it alone under the host sanitizers.  Written from the public definition of the format
// (ITU-T T.81, Annex K for the tables): every store is checked against the capacity, every coefficient against the code tables.
#ifndef PAM_JPEG_ENCODE_HPP
#define PAM_JPEG_ENCODE_HPP

#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/pam.h"

namespace pamjpegenc {

static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2, natural order
static const uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 - K.6: code counts per length 1 .. 16, then the symbols in code order
static const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

enum { HEADER_BYTES = 623, BLOCK_BYTES = 420 };       // SOI .. SOS; 20 + 63 * 26 bits of a block, every byte stuffed, rounded up

static inline bool sampling_ok(int hs, int vs) { return (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2); }

static inline int quality_tables(int quality, uint16_t* tables) {
    if (!tables || quality < 1 || quality > 100) return PAM_E_ARG;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (kBaseQuant[t][i] * scale + 50) / 100;
            tables[t * 64 + i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return PAM_OK;
}

static inline int encode_bound(int width, int height, int hs, int vs, size_t* bytes) {
    if (!bytes || width < 1 || width > 65535 || height < 1 || height > 65535 || !sampling_ok(hs, vs)) return PAM_E_ARG;
    const size_t mw = ((size_t)width + 8 * hs - 1) / (8 * hs), mh = ((size_t)height + 8 * vs - 1) / (8 * vs);
    *bytes = (size_t)HEADER_BYTES + 2 + mw * mh * (size_t)(hs * vs + 2) * BLOCK_BYTES;
    return PAM_OK;
}

// the code of every symbol of one table: counts per length + symbols in code order -> (code, length), length 0 = no code
struct Codes {
    uint16_t code[256];
    uint8_t len[256];
};
static inline void build_codes(Codes& c, const uint8_t* bits, const uint8_t* vals, int n_vals) {
    memset(&c, 0, sizeof(c));
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1] && k < n_vals; ++i, ++k, ++code) {
            c.code[vals[k]] = (uint16_t)code;
            c.len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}

// bytes into out[0 .. cap): a store past the capacity is dropped and remembered.  Entropy-coded bits gather in `acc` and leave four
// bytes at a time: as one unchecked store when the capacity has room and none of the four is FF, else byte by byte with stuffing.
struct Sink {
    uint8_t* out;
    size_t cap, n;
    bool full;
    uint64_t acc;                // the low `bits` bits are pending
    int bits;
    inline void byte(unsigned b) {
        if (n < cap) out[n++] = (uint8_t)b;
        else full = true;
    }
    inline void bytes(const uint8_t* p, size_t k) {
        for (size_t i = 0; i < k; ++i) byte(p[i]);
    }
    inline void u16(unsigned v) { byte(v >> 8); byte(v & 255); }
    inline void entropy_byte(unsigned b) {
        byte(b);
        if (b == 0xFF) byte(0);
    }
    inline void put(uint32_t v, int len) {                               // v < 2^len, len <= 26
        acc = (acc << len) | v;
        bits += len;
        if (bits < 32) return;
        bits -= 32;
        const uint32_t w = (uint32_t)(acc >> bits);
        if (cap - n >= 4 && !(((w & 0x7F7F7F7Fu) + 0x01010101u) & w & 0x80808080u)) {      // room, and no byte of w is FF
            out[n] = (uint8_t)(w >> 24); out[n + 1] = (uint8_t)(w >> 16); out[n + 2] = (uint8_t)(w >> 8); out[n + 3] = (uint8_t)w;
            n += 4;
        } else {
            entropy_byte(w >> 24); entropy_byte((w >> 16) & 255u); entropy_byte((w >> 8) & 255u); entropy_byte(w & 255u);
        }
    }
    inline void flush_ones() {                                           // pads the last byte with one-bits and writes what is pending
        const int pad = (8 - (bits & 7)) & 7;
        acc = (acc << pad) | ((1u << pad) - 1u);
        bits += pad;
        while (bits > 0) {
            bits -= 8;
            entropy_byte((unsigned)(acc >> bits) & 255u);
        }
    }
};

static inline int category(int v) {                                      // bits of |v|
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

static inline int encode(const int16_t* coef, size_t coef_words, const PamJpegEncodeParams* p, uint8_t* out, size_t capacity, size_t* out_bytes) {
    if (!coef || !p || !out || !out_bytes) return PAM_E_ARG;
    size_t bound;
    if (encode_bound(p->width, p->height, p->h_samp, p->v_samp, &bound) != PAM_OK) return PAM_E_ARG;
    const int W = p->width, H = p->height, hs = p->h_samp, vs = p->v_samp;
    const size_t mw = ((size_t)W + 8 * hs - 1) / (8 * hs), mh = ((size_t)H + 8 * vs - 1) / (8 * vs);
    const size_t luma = mw * hs * mh * vs, chroma = mw * mh;
    if (coef_words < 64 * (luma + 2 * chroma)) return PAM_E_ARG;
    uint16_t quant[2][64];
    if (p->quality == 0) {
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < 64; ++i) {
                if (p->quant[t][i] < 1 || p->quant[t][i] > 255) return PAM_E_ARG;
                quant[t][i] = p->quant[t][i];
            }
    } else if (quality_tables(p->quality, &quant[0][0]) != PAM_OK) {
        return PAM_E_ARG;
    }
    Sink s = {out, capacity, 0, false, 0, 0};
    s.u16(0xFFD8);
    static const uint8_t app0[16] = {0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    s.u16(0xFFE0); s.bytes(app0, sizeof(app0));
    for (int t = 0; t < 2; ++t) {
        s.u16(0xFFDB); s.u16(67); s.byte(t);
        for (int k = 0; k < 64; ++k) s.byte(quant[t][kNatural[k]]);
    }
    s.u16(0xFFC0); s.u16(17); s.byte(8); s.u16(H); s.u16(W); s.byte(3);
    s.byte(1); s.byte((hs << 4) | vs); s.byte(0);
    s.byte(2); s.byte(0x11); s.byte(1);
    s.byte(3); s.byte(0x11); s.byte(1);
    Codes dc[2], ac[2];
    for (int t = 0; t < 2; ++t) {
        build_codes(dc[t], kDcBits[t], kDcVals, 12);
        build_codes(ac[t], kAcBits[t], kAcVals[t], 162);
        s.u16(0xFFC4); s.u16(2 + 1 + 16 + 12); s.byte(t); s.bytes(kDcBits[t], 16); s.bytes(kDcVals, 12);
        s.u16(0xFFC4); s.u16(2 + 1 + 16 + 162); s.byte(0x10 | t); s.bytes(kAcBits[t], 16); s.bytes(kAcVals[t], 162);
    }
    static const uint8_t sos[12] = {0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    s.u16(0xFFDA); s.bytes(sos, sizeof(sos));

    // real blocks per row and rows of blocks of each component; the layout's rows are bw[c] blocks long
    const size_t wb[3] = {((size_t)W + 7) / 8, ((size_t)(W + hs - 1) / hs + 7) / 8, ((size_t)(W + hs - 1) / hs + 7) / 8};
    const size_t hb[3] = {((size_t)H + 7) / 8, ((size_t)(H + vs - 1) / vs + 7) / 8, ((size_t)(H + vs - 1) / vs + 7) / 8};
    const size_t bw[3] = {mw * hs, mw, mw}, first[3] = {0, luma, luma + chroma};
    const int ch[3] = {hs, 1, 1}, cv[3] = {vs, 1, 1};
    int pred[3] = {0, 0, 0};
    for (size_t my = 0; my < mh && !s.full; ++my)
        for (size_t mx = 0; mx < mw && !s.full; ++mx)
            for (int c = 0; c < 3; ++c) {
                const int t = c ? 1 : 0;
                for (int v = 0; v < cv[c]; ++v)
                    for (int h = 0; h < ch[c]; ++h) {
                        const size_t by = my * cv[c] + v, bx = mx * ch[c] + h;
                        if (bx >= wb[c] || by >= hb[c]) {                  // a dummy block: the DC of the block before it, no AC
                            s.put(dc[t].code[0], dc[t].len[0]);
                            s.put(ac[t].code[0], ac[t].len[0]);
                            continue;
                        }
                        const int16_t* b = coef + 64 * (first[c] + by * bw[c] + bx);
                        const int diff = (int)b[0] - pred[c];
                        pred[c] = b[0];
                        int n = category(diff);
                        if (n > 11) return PAM_E_ARG;
                        s.put(dc[t].code[n], dc[t].len[n]);
                        if (n) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
                        int run = 0;
                        for (int k = 1; k < 64; ++k) {
                            const int a = b[kNatural[k]];
                            if (a == 0) { ++run; continue; }
                            while (run > 15) { s.put(ac[t].code[0xF0], ac[t].len[0xF0]); run -= 16; }
                            n = category(a);
                            if (n > 10) return PAM_E_ARG;
                            const int sym = (run << 4) | n;
                            s.put(((unsigned)ac[t].code[sym] << n) | ((unsigned)(a < 0 ? a - 1 : a) & ((1u << n) - 1u)), ac[t].len[sym] + n);
                            run = 0;
                        }
                        if (run) s.put(ac[t].code[0], ac[t].len[0]);
                    }
            }
    s.flush_ones();
    s.u16(0xFFD9);
    if (s.full) return PAM_E_ARG;
    *out_bytes = s.n;
    return PAM_OK;
}

}  // namespace pamjpegenc
#endif
