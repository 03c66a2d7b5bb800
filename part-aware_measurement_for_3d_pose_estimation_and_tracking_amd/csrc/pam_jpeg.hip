// libpam_hip.so, baseline JPEG frames rebuilt on the device: the host runs the serial Huffman pass alone (pam_jpeg_entropy.hpp) and
// uploads quantised coefficients; k_jpeg_idct dequantises and runs libjpeg's slow-integer inverse DCT into component planes, k_jpeg_color
// upsamples the chroma ("fancy" triangle filter), converts to BGR and writes the H x W x 3 frame the crop and resize kernels read.  All
// images of a frame set go through ONE launch pair; the arithmetic is int32 as include/pam.h states it, done in uint32 wherever a hostile
// coefficient could make it wrap.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_jpeg_entropy.hpp"

#define JP_BLOCK 256
#define JP_BLOCKS_PER_WG 32           /* 8 lanes per 8x8 block */
#define JP_LDS_STRIDE 72              /* dwords per block in LDS: 64 + 8, so the four blocks of a 32-lane group fall on 32 different banks */
#define JP_RUN 4                      /* output pixels per lane of k_jpeg_color: 12 bytes, three aligned dwords */

struct JpImg {
    const int16_t* coef;
    const uint16_t* quant;
    uint8_t* planes;
    uint8_t* out;
    uint32_t blk_first[3];            // first block of each component (also its plane's byte offset / 64)
    uint32_t n_blk;
    uint16_t bw[3];                   // blocks per row of each component's plane
    uint16_t W, H, n_comp, hs, vs;
    uint32_t wg_idct, wg_color;       // first workgroup of this image in either grid
};
struct JpArgs {
    JpImg img[PAM_MAX_VIEWS];
    int n_img;
};
static_assert(sizeof(JpArgs) <= 4096, "descriptors travel in the kernel arguments");

typedef uint32_t u32;

// one 1-D pass of the slow-integer inverse DCT (include/pam.h) on x[0..7] in place; s = 11 for the columns, 18 for the rows
__device__ __forceinline__ void jp_idct8(u32* x, int s) {
    u32 z1 = (x[2] + x[6]) * 4433u;
    const u32 t2 = z1 - x[6] * 15137u, t3 = z1 + x[2] * 6270u;
    const u32 t0 = (x[0] + x[4]) << 13, t1 = (x[0] - x[4]) << 13;
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u32 a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    u32 z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u32 z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (u32)-7373; z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const u32 r = 1u << (s - 1);
    x[0] = (u32)((int32_t)(t10 + a3 + r) >> s);
    x[7] = (u32)((int32_t)(t10 - a3 + r) >> s);
    x[1] = (u32)((int32_t)(t11 + a2 + r) >> s);
    x[6] = (u32)((int32_t)(t11 - a2 + r) >> s);
    x[2] = (u32)((int32_t)(t12 + a1 + r) >> s);
    x[5] = (u32)((int32_t)(t12 - a1 + r) >> s);
    x[3] = (u32)((int32_t)(t13 + a0 + r) >> s);
    x[4] = (u32)((int32_t)(t13 - a0 + r) >> s);
}

__device__ __forceinline__ int jp_image_of(const JpArgs& a, u32 wg, bool color) {
    int i = 0;                                                            // workgroup-uniform: a workgroup never spans two images
    for (int k = 1; k < a.n_img; ++k)
        if (wg >= (color ? a.img[k].wg_color : a.img[k].wg_idct)) i = k;
    return i;
}

// 8 lanes per 8x8 block: lane r loads row r of the coefficients and of the quantisation table (16 bytes each), the products are
// transposed through LDS, lane j runs column j (pass 1), the results go back through LDS, lane r runs row r (pass 2) and stores the
// 8 bytes of its row of the plane.  Groups beyond the image's last block do the arithmetic on zeros and store nothing.
__global__ __launch_bounds__(JP_BLOCK) void k_jpeg_idct(const JpArgs a) {
    __shared__ u32 lds[2][JP_BLOCKS_PER_WG * JP_LDS_STRIDE];
    const JpImg& im = a.img[jp_image_of(a, blockIdx.x, false)];
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const u32 b = (blockIdx.x - im.wg_idct) * JP_BLOCKS_PER_WG + g;      // block of the image, components one after the other
    const bool live = b < im.n_blk;
    int c = 0;
    if (im.n_comp == 3) c = b >= im.blk_first[2] ? 2 : b >= im.blk_first[1] ? 1 : 0;
    u32 x[8];
    if (live) {
        const uint4 cw = *reinterpret_cast<const uint4*>(im.coef + (size_t)b * 64 + r * 8);
        const uint4 qw = *reinterpret_cast<const uint4*>(im.quant + c * 64 + r * 8);
        const u32 cv[4] = {cw.x, cw.y, cw.z, cw.w}, qv[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[2 * k] = (u32)(int32_t)(int16_t)(cv[k] & 0xFFFFu) * (qv[k] & 0xFFFFu);
            x[2 * k + 1] = (u32)(int32_t)(int16_t)(cv[k] >> 16) * (qv[k] >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = 0;
    }
    u32* const t0 = lds[0] + g * JP_LDS_STRIDE;
    u32* const t1 = lds[1] + g * JP_LDS_STRIDE;
#pragma unroll
    for (int k = 0; k < 8; ++k) t0[r * 8 + k] = x[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t0[k * 8 + r];                    // column r
    jp_idct8(x, 11);
#pragma unroll
    for (int k = 0; k < 8; ++k) t1[k * 8 + r] = x[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t1[r * 8 + k];                    // row r
    jp_idct8(x, 18);
    if (!live) return;
    u32 px[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) px[k] = (u32)min(max((int32_t)x[k] + 128, 0), 255);
    const u32 bc = b - (c ? im.blk_first[c] : 0u), bw = im.bw[c];
    const u32 by = bc / bw, bx = bc - by * bw;
    uint2 o;
    o.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    o.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    uint8_t* const plane = im.planes + (size_t)(c ? im.blk_first[c] : 0u) * 64;
    *reinterpret_cast<uint2*>(plane + ((size_t)by * 8 + r) * (bw * 8) + bx * 8) = o;
}

__device__ __forceinline__ int jp_clamp255(int v) { return min(max(v, 0), 255); }

// one chroma sample of output pixel (y, x): the triangle filter over the true subsampled extents (w, h), neighbours clamped -- at an edge
// (3 p + p + 1) >> 2 = p and (3 s + s + 8) >> 4 = (4 s + 8) >> 4, which are the first / last column's rules
__device__ __forceinline__ int jp_chroma(const uint8_t* p, int stride, int hs, int vs, int w, int h, int y, int x) {
    if (hs == 1) return p[(size_t)y * stride + x];
    const int i = x >> 1, odd = x & 1;
    const int i2 = odd ? min(i + 1, w - 1) : max(i - 1, 0);
    if (vs == 1) {
        const uint8_t* row = p + (size_t)y * stride;
        return (3 * row[i] + row[i2] + 1 + odd) >> 2;
    }
    const int rr = y >> 1;
    const int r2 = (y & 1) ? min(rr + 1, h - 1) : max(rr - 1, 0);
    const uint8_t* near = p + (size_t)rr * stride;
    const uint8_t* far = p + (size_t)r2 * stride;
    const int s = 3 * near[i] + far[i], s2 = 3 * near[i2] + far[i2];
    return (3 * s + s2 + 8 - odd) >> 4;
}

// One lane = JP_RUN consecutive pixels of the frame taken as one row-major list (a run may wrap into the next image row), so a lane's 12
// output bytes are three aligned dwords whatever W is; the image's last lane stores what is left byte by byte.
__global__ __launch_bounds__(JP_BLOCK) void k_jpeg_color(const JpArgs a) {
    const JpImg& im = a.img[jp_image_of(a, blockIdx.x, true)];
    const int W = im.W, H = im.H;
    const u32 n_px = (u32)W * (u32)H;
    const u32 p0 = ((blockIdx.x - im.wg_color) * JP_BLOCK + threadIdx.x) * JP_RUN;
    if (p0 >= n_px) return;
    const int hs = im.hs, vs = im.vs, w = (W + hs - 1) / hs, h = (H + vs - 1) / vs;
    const uint8_t* const py = im.planes;
    const int sy = im.bw[0] * 8;
    const bool colour = im.n_comp == 3;
    const uint8_t* const pcb = im.planes + (size_t)im.blk_first[1] * 64;
    const uint8_t* const pcr = im.planes + (size_t)im.blk_first[2] * 64;
    const int sc = im.bw[1] * 8;
    int y = p0 / (u32)W, x = p0 - (u32)y * (u32)W;
    const int n = min((u32)JP_RUN, n_px - p0);
    u32 bytes[3 * JP_RUN];
#pragma unroll
    for (int k = 0; k < JP_RUN; ++k) {
        int B = 0, G = 0, R = 0;
        if (k < n) {
            const int Y = py[(size_t)y * sy + x];
            B = G = R = Y;
            if (colour) {
                const int cb = jp_chroma(pcb, sc, hs, vs, w, h, y, x) - 128, cr = jp_chroma(pcr, sc, hs, vs, w, h, y, x) - 128;
                R = jp_clamp255(Y + ((91881 * cr + 32768) >> 16));
                G = jp_clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                B = jp_clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
            if (++x == W) { x = 0; ++y; }
        }
        bytes[3 * k] = B; bytes[3 * k + 1] = G; bytes[3 * k + 2] = R;
    }
    uint8_t* const o = im.out + (size_t)p0 * 3;
    if (n == JP_RUN) {
        u32* const o4 = reinterpret_cast<u32*>(o);                        // out is 4-byte aligned (entry point) and p0 * 3 a multiple of 12
#pragma unroll
        for (int k = 0; k < 3; ++k) o4[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) o[k] = (uint8_t)bytes[k];
    }
}

extern "C" int pam_jpeg_probe(const uint8_t* data, size_t n, PamJpegInfo* info) { return pamjpeg::probe(data, n, info); }

extern "C" int pam_jpeg_entropy(const uint8_t* data, size_t n, const PamJpegInfo* info, int16_t* coef, size_t coef_words) {
    return pamjpeg::entropy(data, n, info, coef, coef_words);
}

extern "C" int pam_jpeg_reconstruct(void* stream, int n_img, const PamJpegImage* images) {
    if (!images || n_img < 1 || n_img > PAM_MAX_VIEWS) return PAM_E_ARG;
    JpArgs a;
    memset(&a, 0, sizeof(a));
    a.n_img = n_img;
    uint64_t wg_i = 0, wg_c = 0;
    for (int i = 0; i < n_img; ++i) {
        const PamJpegImage& s = images[i];
        JpImg& d = a.img[i];
        if (!s.dev_coef || !s.dev_quant || !s.dev_planes || !s.dev_out) return PAM_E_ARG;
        if (((uintptr_t)s.dev_coef | (uintptr_t)s.dev_quant | (uintptr_t)s.dev_planes) & 15 || ((uintptr_t)s.dev_out & 3)) return PAM_E_ARG;
        if (s.width < 1 || s.width > 65535 || s.height < 1 || s.height > 65535) return PAM_E_ARG;
        const int hs = s.h_samp, vs = s.v_samp;
        if (s.n_comp == 1 ? (hs != 1 || vs != 1) : s.n_comp == 3 ? !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) : true)
            return PAM_E_ARG;
        const uint64_t mw = (s.width + 8 * hs - 1) / (8 * hs), mh = (s.height + 8 * vs - 1) / (8 * vs);
        const uint64_t luma = mw * hs * mh * vs, chroma = s.n_comp == 3 ? mw * mh : 0, n_blk = luma + 2 * chroma;
        if (n_blk * 64 >= (1ull << 31)) return PAM_E_ARG;                  // plane and coefficient offsets stay far inside 32 bits
        d.coef = s.dev_coef; d.quant = s.dev_quant; d.planes = s.dev_planes; d.out = s.dev_out;
        d.blk_first[0] = 0; d.blk_first[1] = (uint32_t)luma; d.blk_first[2] = (uint32_t)(luma + chroma);
        d.n_blk = (uint32_t)n_blk;
        d.bw[0] = (uint16_t)(mw * hs); d.bw[1] = d.bw[2] = (uint16_t)mw;
        d.W = (uint16_t)s.width; d.H = (uint16_t)s.height; d.n_comp = (uint16_t)s.n_comp; d.hs = (uint16_t)hs; d.vs = (uint16_t)vs;
        d.wg_idct = (uint32_t)wg_i; d.wg_color = (uint32_t)wg_c;
        wg_i += (n_blk + JP_BLOCKS_PER_WG - 1) / JP_BLOCKS_PER_WG;
        wg_c += ((uint64_t)s.width * s.height + JP_BLOCK * JP_RUN - 1) / (JP_BLOCK * JP_RUN);
        if (wg_i >= (1ull << 31) || wg_c >= (1ull << 31)) return PAM_E_ARG;
    }
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)wg_i), dim3(JP_BLOCK), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_jpeg_color, dim3((unsigned)wg_c), dim3(JP_BLOCK), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
