// libpam_hip.so, BGR frames turned into quantised JPEG coefficients on the device: the mirror image of pam_jpeg.hip.  k_jpeg_fdct reads
// the frame's pixels directly -- colour conversion, edge replication and chroma downsampling happen in the load, no component planes
// exist in memory -- runs libjpeg's slow-integer forward DCT and quantises into the layout PamJpegInfo describes; the host then runs
// the serial Huffman pass alone (pam_jpeg_encode.hpp, exported here).  All images of a frame set go through ONE launch; the
// arithmetic is int32 as include/pam.h states it, done in uint32 so that nothing a caller passes can overflow a signed type.
// gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_jpeg_encode.hpp"

#define JF_BLOCK 256
#define JF_BLOCKS_PER_WG 32           /* 8 lanes per 8x8 block, as k_jpeg_idct */
#define JF_LDS_STRIDE 72              /* dwords per block in LDS: 64 + 8, so the four blocks of a 32-lane group fall on 32 different banks */

struct JfImg {
    const uint8_t* bgr;
    const uint16_t* quant;
    int16_t* coef;
    uint32_t blk_first[3];            // first block of each component
    uint32_t n_blk;
    uint16_t bw[3];                   // blocks per row of each component in the layout
    uint16_t wb[3], hb[3];            // real blocks per row / block rows of each component
    uint16_t W, H, hs, vs;
    uint32_t wg_first;                // first workgroup of this image
};
struct JfArgs {
    JfImg img[PAM_MAX_VIEWS];
    int n_img;
};
static_assert(sizeof(JfArgs) <= 4096, "descriptors travel in the kernel arguments");

typedef uint32_t u32;

__device__ __forceinline__ u32 jf_round(u32 v, int s) { return (u32)((int32_t)(v + (1u << (s - 1))) >> s); }

// one 1-D pass of the slow-integer forward DCT (include/pam.h) on d[0..7] in place; rows: first pass (s = 11, DC terms << 2), else the
// second (s = 15, DC terms rounded >> 2)
__device__ __forceinline__ void jf_fdct8(u32* d, bool rows) {
    const u32 t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    u32 t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int s = rows ? 11 : 15;
    d[0] = rows ? (t10 + t11) << 2 : jf_round(t10 + t11, 2);
    d[4] = rows ? (t10 - t11) << 2 : jf_round(t10 - t11, 2);
    u32 z1 = (t12 + t13) * 4433u;
    d[2] = jf_round(z1 + t13 * 6270u, s);
    d[6] = jf_round(z1 - t12 * 15137u, s);
    z1 = t4 + t7;
    u32 z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const u32 z5 = (z3 + z4) * 9633u;
    t4 *= 2446u; t5 *= 16819u; t6 *= 25172u; t7 *= 12299u;
    z1 *= (u32)-7373; z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    d[7] = jf_round(t4 + z1 + z3, s);
    d[5] = jf_round(t5 + z2 + z4, s);
    d[3] = jf_round(t6 + z2 + z3, s);
    d[1] = jf_round(t7 + z1 + z4, s);
}

// component c (0 = Y, 1 = Cb, 2 = Cr) of one B, G, R pixel
__device__ __forceinline__ int jf_comp(const uint8_t* px, int c) {
    const int B = px[0], G = px[1], R = px[2];
    if (c == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (c == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// 8 lanes per 8x8 block: lane r builds row r of the block's samples from the pixels and runs the row pass, the results are transposed
// through LDS, lane j runs column j, the results go back through LDS, and lane r quantises row r and stores its 16 bytes.  A padding
// block of the layout (beyond the component's real blocks) is stored as zeros; groups beyond the image's last block store nothing.
__global__ __launch_bounds__(JF_BLOCK) void k_jpeg_fdct(const JfArgs a) {
    __shared__ u32 lds[2][JF_BLOCKS_PER_WG * JF_LDS_STRIDE];
    int ii = 0;                                                           // workgroup-uniform: a workgroup never spans two images
    for (int k = 1; k < a.n_img; ++k)
        if (blockIdx.x >= a.img[k].wg_first) ii = k;
    const JfImg& im = a.img[ii];
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const u32 b = (blockIdx.x - im.wg_first) * JF_BLOCKS_PER_WG + g;     // block of the image, components one after the other
    const bool live = b < im.n_blk;
    const int c = b >= im.blk_first[2] ? 2 : b >= im.blk_first[1] ? 1 : 0;
    const u32 bc = b - im.blk_first[c], bw = im.bw[c];
    const u32 by = bc / bw, bx = bc - by * bw;
    const bool real = live && bx < im.wb[c] && by < im.hb[c];
    u32 x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = 0;
    if (real) {
        const int W = im.W, H = im.H;
        const int hs = c ? im.hs : 1, vs = c ? im.vs : 1;               // pixels per sample of this component
        const int rows = (H + vs - 1) / vs;                              // the component's true height: rows below it repeat its last row
        const int y = min((int)(by * 8 + r), rows - 1);
        const uint8_t* const r0 = im.bgr + (size_t)min(vs * y, H - 1) * W * 3;
        const uint8_t* const r1 = im.bgr + (size_t)min(vs * y + vs - 1, H - 1) * W * 3;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int xs = bx * 8 + k;
            int v;
            if (hs == 1) {
                v = jf_comp(r0 + (size_t)min(xs, W - 1) * 3, c);
            } else {
                const int x0 = min(2 * xs, W - 1) * 3, x1 = min(2 * xs + 1, W - 1) * 3;
                if (vs == 1) v = (jf_comp(r0 + x0, c) + jf_comp(r0 + x1, c) + (k & 1)) >> 1;
                else v = (jf_comp(r0 + x0, c) + jf_comp(r0 + x1, c) + jf_comp(r1 + x0, c) + jf_comp(r1 + x1, c) + 1 + (k & 1)) >> 2;
            }
            x[k] = (u32)(v - 128);
        }
    }
    jf_fdct8(x, true);
    u32* const t0 = lds[0] + g * JF_LDS_STRIDE;
    u32* const t1 = lds[1] + g * JF_LDS_STRIDE;
#pragma unroll
    for (int k = 0; k < 8; ++k) t0[r * 8 + k] = x[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t0[k * 8 + r];                    // column r
    jf_fdct8(x, false);
#pragma unroll
    for (int k = 0; k < 8; ++k) t1[k * 8 + r] = x[k];
    __syncthreads();
    if (!live) return;
    u32 o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = 0;
    if (real) {
        const uint4 qw = *reinterpret_cast<const uint4*>(im.quant + c * 64 + r * 8);
        const u32 qp[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int32_t v = (int32_t)t1[r * 8 + k];                    // row r
            const u32 q = (k & 1) ? qp[k >> 1] >> 16 : qp[k >> 1] & 0xFFFFu;
            const u32 qv = max(q, 1u) << 3;
            const u32 m = ((u32)abs(v) + (qv >> 1)) / qv;                // |v| < 2^15: the quotient fits int16
            o[k] = (u32)(v < 0 ? -(int32_t)m : (int32_t)m) & 0xFFFFu;
        }
    }
    uint4 w;
    w.x = o[0] | (o[1] << 16); w.y = o[2] | (o[3] << 16); w.z = o[4] | (o[5] << 16); w.w = o[6] | (o[7] << 16);
    *reinterpret_cast<uint4*>(im.coef + (size_t)b * 64 + r * 8) = w;
}

extern "C" int pam_jpeg_quality_tables(int quality, uint16_t* tables) { return pamjpegenc::quality_tables(quality, tables); }

extern "C" int pam_jpeg_encode_bound(int width, int height, int h_samp, int v_samp, size_t* bytes) {
    return pamjpegenc::encode_bound(width, height, h_samp, v_samp, bytes);
}

extern "C" int pam_jpeg_encode(const int16_t* coef, size_t coef_words, const PamJpegEncodeParams* params, uint8_t* out, size_t capacity,
                               size_t* out_bytes) {
    return pamjpegenc::encode(coef, coef_words, params, out, capacity, out_bytes);
}

extern "C" int pam_jpeg_forward(void* stream, int n_img, const PamJpegFwdImage* images) {
    if (!images || n_img < 1 || n_img > PAM_MAX_VIEWS) return PAM_E_ARG;
    JfArgs a;
    memset(&a, 0, sizeof(a));
    a.n_img = n_img;
    uint64_t wg = 0;
    for (int i = 0; i < n_img; ++i) {
        const PamJpegFwdImage& s = images[i];
        JfImg& d = a.img[i];
        if (!s.dev_bgr || !s.dev_quant || !s.dev_coef) return PAM_E_ARG;
        if (((uintptr_t)s.dev_quant | (uintptr_t)s.dev_coef) & 15) return PAM_E_ARG;
        if (s.width < 1 || s.width > 65535 || s.height < 1 || s.height > 65535) return PAM_E_ARG;
        const int hs = s.h_samp, vs = s.v_samp;
        if (!pamjpegenc::sampling_ok(hs, vs)) return PAM_E_ARG;
        const uint64_t mw = (s.width + 8 * hs - 1) / (8 * hs), mh = (s.height + 8 * vs - 1) / (8 * vs);
        const uint64_t luma = mw * hs * mh * vs, chroma = mw * mh, n_blk = luma + 2 * chroma;
        if (n_blk * 64 >= (1ull << 31)) return PAM_E_ARG;                  // coefficient offsets stay far inside 32 bits
        d.bgr = s.dev_bgr; d.quant = s.dev_quant; d.coef = s.dev_coef;
        d.blk_first[0] = 0; d.blk_first[1] = (uint32_t)luma; d.blk_first[2] = (uint32_t)(luma + chroma);
        d.n_blk = (uint32_t)n_blk;
        d.bw[0] = (uint16_t)(mw * hs); d.bw[1] = d.bw[2] = (uint16_t)mw;
        d.wb[0] = (uint16_t)((s.width + 7) / 8); d.hb[0] = (uint16_t)((s.height + 7) / 8);
        d.wb[1] = d.wb[2] = (uint16_t)(((s.width + hs - 1) / hs + 7) / 8);
        d.hb[1] = d.hb[2] = (uint16_t)(((s.height + vs - 1) / vs + 7) / 8);
        d.W = (uint16_t)s.width; d.H = (uint16_t)s.height; d.hs = (uint16_t)hs; d.vs = (uint16_t)vs;
        d.wg_first = (uint32_t)wg;
        wg += (n_blk + JF_BLOCKS_PER_WG - 1) / JF_BLOCKS_PER_WG;
        if (wg >= (1ull << 31)) return PAM_E_ARG;
    }
    hipLaunchKernelGGL(k_jpeg_fdct, dim3((unsigned)wg), dim3(JF_BLOCK), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
