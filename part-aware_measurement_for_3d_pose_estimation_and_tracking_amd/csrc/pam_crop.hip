// libpam_hip.so, crop part of a1 (HRNetPose.predict pre-processing; call site: the reference's src/ivclabpose.py:210).
// Crop / resize / normalise in front of the conv stack (csrc/pam_conv.hip and its pam_conv_*.hip kernel families): person boxes of the
// BGR uint8 frames -> RGB, /255, ImageNet mean/std, bf16 NHWC.  HBM-bound streaming kernels, one thread per output pixel.
// Two geometries, two kernels each (plain / with the mirrored rows of a flip test).  stretch: the box itself, border replicate -- one
// template over FLIP behind two plain kernels, on the functions below.  affine: the effective box of pam_box_cs.hpp, zero border -- one
// text included twice.  The float operations and their order are the contract (-ffp-contract=off; the tests pin bits).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"
#include "pam_box_cs.hpp"

constexpr int AA_MAXT = 24;             // antialias taps per axis at most (down-scaling by up to 11.5)
__host__ __device__ inline void store_box(float* row, const PamBoxCs e) { row[0] = e.x; row[1] = e.y; row[2] = e.w; row[3] = e.h; }

// Row layout of the output buffer.  FLIP false: rows n_src .. (grid) repeat row n_src - 1 -- a replay bucket larger than the call
// (HRNetPose pads a batch to a multiple of graph_bucket) needs no padded box table.  FLIP true: the crops of one flip-test forward in one
// buffer -- rows [0, n_src) plain, rows [n_src, 2 n_src) the column reversal of row r - n_src, rows from 2 n_src on repeat row
// 2 n_src - 1.  A mirrored row is the SAME sample stored at column ow - 1 - ox (the official input.flip(3)): bit-equal to the reversal of
// the plain row on both resize paths, never a resample of a mirrored box.
struct CropRow { int crop, src; bool mirror; };
template <bool FLIP>
__device__ __forceinline__ CropRow crop_row(int n_src) {
    CropRow r;
    r.crop = blockIdx.y;
    r.mirror = FLIP && r.crop >= n_src;
    r.src = min(r.mirror ? r.crop - n_src : r.crop, n_src - 1);
    return r;
}
// Two neighbouring pixels of a frame row are 6 consecutive bytes: ONE unaligned 8-byte load instead of six byte loads (the kernels were
// bound by the texture-address unit: 12 one-byte gathers per output pixel).  The caller checks that the 8 bytes at p lie inside the row
// and falls back to byte loads of the pixels its border rule needs where they do not.
__device__ __forceinline__ void load_two_pixels(const uint8_t* p, uint8_t (&t)[6]) {
    struct __attribute__((packed)) U8 { uint32_t x, y; };              // alignment 1: the backend emits one dwordx2 load (unaligned access is on)
    const U8 q = *(const U8*)p;
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = (uint8_t)((k < 4 ? q.x >> (8 * k) : q.y >> (8 * (k - 4))) & 0xff);
}
// bilinear blend of the 2 x 2 taps t0 (upper row) / t1 of RGB channel c (the source is BGR), 0 .. 255
__device__ __forceinline__ float blend(const uint8_t (&t0)[6], const uint8_t (&t1)[6], int c, float fx, float fy) {
    const int sc = 2 - c;
    const float a = (float)t0[sc], b = (float)t0[3 + sc];
    const float cc = (float)t1[sc], d = (float)t1[3 + sc];
    const float top = a + (b - a) * fx, bot = cc + (d - cc) * fx;
    return top + (bot - top) * fy;
}
// RGB channel c of a 0 .. 1 value -> ImageNet-normalised bf16
__device__ __forceinline__ uint16_t normalise(float v, int c) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, istd[3] = {1.0f / 0.229f, 1.0f / 0.224f, 1.0f / 0.225f};
    return f32_to_bf16((v - mean[c]) * istd[c]);
}
__device__ __forceinline__ void store_pixel(uint16_t* __restrict__ out, CropRow r, int oh, int ow, int oc, int oy, int ox, const uint16_t (&o)[3]) {
    const int st = r.mirror ? ow - 1 - ox : ox;      // the store column
    if (oc == 3) {
        uint16_t* dst = out + (((size_t)r.crop * oh + oy) * ow + st) * 3;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    } else {            // 8-channel form for the MFMA conv kernel (Cin % 8 == 0): RGB + 5 zero channels, one 16-B store
        uint4 v;
        v.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16); v.y = (uint32_t)o[2]; v.z = 0; v.w = 0;
        *(uint4*)(out + (((size_t)r.crop * oh + oy) * ow + st) * 8) = v;
    }
}

// ---- stretch: the box's own extent onto the output, half-pixel centres, border replicate ---------------------------------------------
// Plain bilinear interpolation (the default, = cv2.resize INTER_LINEAR / F.interpolate(bilinear)) only ever reads 2 x 2 pixels.
// antialias: the resize of upstream simple-HRNet (a PIL image through torchvision's Resize) filters with a triangle whose support grows
// with the down-scaling factor.  The two agree for boxes no larger than the network input; HD boxes taller than 384 pixels are
// down-scaled.  With antialias the taps are the frame pixels i whose centres lie within max(scale, 1) of the output pixel's centre, inside
// the box rounded outwards (the crop upstream cuts), weights 1 - |i + 0.5 - centre| / max(scale, 1), normalised (PIL's ImagingResample
// formula, in float32: PIL's own uint8 rounding between its two passes is not reproduced).
template <bool FLIP>
__device__ __forceinline__ void crop_stretch(int n_src, const uint8_t* const* __restrict__ frames, int H, int W,
                                             const int* __restrict__ view_of, const float* __restrict__ boxes,
                                             int oh, int ow, int oc, uint16_t* __restrict__ out, int antialias) {
    const CropRow row = crop_row<FLIP>(n_src);
    const int src = row.src;
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= oh * ow) return;
    const int oy = px / ow, ox = px % ow;
    const uint8_t* __restrict__ img = frames[view_of[src]];
    const float bx = boxes[src * 4 + 0], by = boxes[src * 4 + 1], bw = boxes[src * 4 + 2], bh = boxes[src * 4 + 3];
    uint16_t o[3];
    if (!antialias) {
        float sx = bx + (ox + 0.5f) * (bw / (float)ow) - 0.5f;
        float sy = by + (oy + 0.5f) * (bh / (float)oh) - 0.5f;
        sx = fminf(fmaxf(sx, 0.0f), (float)(W - 1));
        sy = fminf(fmaxf(sy, 0.0f), (float)(H - 1));
        const int x0 = (int)sx, y0 = (int)sy;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float fx = sx - (float)x0, fy = sy - (float)y0;
        const uint8_t* r0 = img + ((size_t)y0 * W) * 3;
        const uint8_t* r1 = img + ((size_t)y1 * W) * 3;
        uint8_t t0[6], t1[6];
        if (x0 + 2 < W) {                      // not for the last two columns (x1 is clamped there / the load would leave the row)
            load_two_pixels(r0 + x0 * 3, t0);
            load_two_pixels(r1 + x0 * 3, t1);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { t0[k] = r0[x0 * 3 + k]; t0[3 + k] = r0[x1 * 3 + k]; t1[k] = r1[x0 * 3 + k]; t1[3 + k] = r1[x1 * 3 + k]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = normalise(blend(t0, t1, c, fx, fy) * (1.0f / 255.0f), c);
    } else {
        const float scx = bw / (float)ow, scy = bh / (float)oh, supx = fmaxf(scx, 1.0f), supy = fmaxf(scy, 1.0f);
        const float cx = bx + (ox + 0.5f) * scx, cy = by + (oy + 0.5f) * scy;
        // (a box wholly right of / below the frame: the window is the last column / row, whose weight is 0 there -- a black pixel, never a read past the frame)
        const int xlo = min(max(0, (int)floorf(bx)), W - 1), xhi = max(xlo + 1, min(W, (int)ceilf(bx + bw)));
        const int ylo = min(max(0, (int)floorf(by)), H - 1), yhi = max(ylo + 1, min(H, (int)ceilf(by + bh)));
        int x0 = max(xlo, (int)(cx - supx + 0.5f)), x1 = min(xhi, (int)(cx + supx + 0.5f));
        int y0 = max(ylo, (int)(cy - supy + 0.5f)), y1 = min(yhi, (int)(cy + supy + 0.5f));
        if (x1 <= x0) { x0 = min(max((int)cx, xlo), xhi - 1); x1 = x0 + 1; }
        if (y1 <= y0) { y0 = min(max((int)cy, ylo), yhi - 1); y1 = y0 + 1; }
        // beyond the limit the window is cut to the AA_MAXT taps nearest the centre (symmetric: no shift of the sampled position)
        if (x1 - x0 > AA_MAXT) { x0 = min(max((int)floorf(cx - 0.5f * AA_MAXT + 0.5f), x0), x1 - AA_MAXT); x1 = x0 + AA_MAXT; }
        if (y1 - y0 > AA_MAXT) { y0 = min(max((int)floorf(cy - 0.5f * AA_MAXT + 0.5f), y0), y1 - AA_MAXT); y1 = y0 + AA_MAXT; }
        const float isx = 1.0f / supx, isy = 1.0f / supy;
        float acc[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
        for (int y = y0; y < y1; ++y) {
            const float wy = fmaxf(0.0f, 1.0f - fabsf(((float)y + 0.5f - cy) * isy));
            const uint8_t* r = img + ((size_t)y * W) * 3;
            float rs[3] = {0.f, 0.f, 0.f}, wr = 0.f;
            for (int x = x0; x < x1; ++x) {
                const float wx = fmaxf(0.0f, 1.0f - fabsf(((float)x + 0.5f - cx) * isx));
                rs[0] += wx * (float)r[x * 3 + 2]; rs[1] += wx * (float)r[x * 3 + 1]; rs[2] += wx * (float)r[x * 3 + 0];
                wr += wx;
            }
            acc[0] += wy * rs[0]; acc[1] += wy * rs[1]; acc[2] += wy * rs[2];
            wsum += wy * wr;
        }
        const float inv = wsum > 0.f ? 1.0f / (wsum * 255.0f) : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = normalise(acc[c] * inv, c);
    }
    store_pixel(out, row, oh, ow, oc, oy, ox, o);
}

// ---- affine: the pose checkpoints' own crop geometry (pam_box_cs.hpp), sampled with ONE scale and a zero border ----------------------------
// The two kernels' text is pam_crop_affine_kernel.inc, included once per form (see there why it is no template).
#define CROP_UDP 0
#define CROP_KERNEL k_preprocess_crops_affine
#define CROP_FLIP 0
#include "pam_crop_affine_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
#define CROP_KERNEL k_preprocess_crops_affine_flip
#define CROP_FLIP 1
#include "pam_crop_affine_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
#undef CROP_UDP
// udp: the same text on the align-corners grid, pitch We / (ow - 1) (CROP_UDP in the .inc)
#define CROP_UDP 1
#define CROP_KERNEL k_preprocess_crops_udp
#define CROP_FLIP 0
#include "pam_crop_affine_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
#define CROP_KERNEL k_preprocess_crops_udp_flip
#define CROP_FLIP 1
#include "pam_crop_affine_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
#undef CROP_UDP

// the stretch kernels' symbols: plain functions, so that a device-code comparison pairs them with any earlier build's
__global__ __launch_bounds__(256) void k_preprocess_crops(int n_src, const uint8_t* const* __restrict__ frames, int H, int W, const int* __restrict__ view_of,
        const float* __restrict__ boxes, int oh, int ow, int oc, uint16_t* __restrict__ out, int antialias) {
    crop_stretch<false>(n_src, frames, H, W, view_of, boxes, oh, ow, oc, out, antialias);
}
__global__ __launch_bounds__(256) void k_preprocess_crops_flip(int n_src, const uint8_t* const* __restrict__ frames, int H, int W, const int* __restrict__ view_of,
        const float* __restrict__ boxes, int oh, int ow, int oc, uint16_t* __restrict__ out, int antialias) {
    crop_stretch<true>(n_src, frames, H, W, view_of, boxes, oh, ow, oc, out, antialias);
}
// the whole effective-box table without a crop (a rank of the crop-sharded predict() crops its share but filters every row)
__global__ __launch_bounds__(256) void k_box_cs(int n, const float* __restrict__ boxes, int ow, int oh, float box_scale, float* __restrict__ eff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PamBoxCs e = pam_box_cs_fn(boxes[i * 4 + 0], boxes[i * 4 + 1], boxes[i * 4 + 2], boxes[i * 4 + 3], ow, oh, box_scale);
    store_box(eff + i * 4, e);
}

// n crops fill n_total >= rows * n output rows (rows = 2 with the mirrored copies)
static bool crop_args_ok(int n, int n_total, int rows, const void* frames, const void* view_of, const void* boxes, const void* out,
                         int out_h, int out_w, int out_c) {
    return n >= 0 && n_total >= rows * (long long)n && frames && view_of && boxes && out && out_h > 0 && out_w > 0 && (out_c == 3 || out_c == 8);
}
static dim3 crop_grid(int out_h, int out_w, int n_total) { return dim3((out_h * out_w + 255) / 256, n_total); }

// stretch geometry; mirrored: n_total >= 2 n rows, the second n the column reversals
static int crops_stretch(bool mirrored, void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w,
                         const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16, int antialias) {
    if (!crop_args_ok(n, n_total, mirrored ? 2 : 1, dev_frames, dev_view_of, dev_boxes, dev_out_bf16, out_h, out_w, out_c)) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    hipLaunchKernelGGL(mirrored ? k_preprocess_crops_flip : k_preprocess_crops, crop_grid(out_h, out_w, n_total), dim3(256), 0, (hipStream_t)stream, n,
                       (const uint8_t* const*)dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, (uint16_t*)dev_out_bf16,
                       antialias ? 1 : 0);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
extern "C" int pam_preprocess_crops_ex(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w, const int32_t* dev_view_of,
        const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16, int antialias) {
    return crops_stretch(false, stream, n, n_total, dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, dev_out_bf16, antialias);
}
extern "C" int pam_preprocess_crops(void* stream, int n, const void* const* dev_frames, int frame_h, int frame_w, const int32_t* dev_view_of,
        const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16) {
    return crops_stretch(false, stream, n, n, dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, dev_out_bf16, 0);
}
extern "C" int pam_preprocess_crops_flip(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w, const int32_t* dev_view_of,
        const float* dev_boxes, int out_h, int out_w, int out_c, void* dev_out_bf16, int antialias) {
    return crops_stretch(true, stream, n, n_total, dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, dev_out_bf16, antialias);
}

extern "C" int pam_preprocess_crops_affine(void* stream, int n, int n_total, int flip, const void* const* dev_frames, int frame_h, int frame_w,
                                           const int32_t* dev_view_of, const float* dev_boxes, float box_scale, int out_h, int out_w,
                                           int out_c, void* dev_out_bf16, int antialias, float* dev_eff_xywh) {
    if (!crop_args_ok(n, n_total, flip ? 2 : 1, dev_frames, dev_view_of, dev_boxes, dev_out_bf16, out_h, out_w, out_c) || !dev_eff_xywh ||
        !(box_scale > 0.0f))
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    hipLaunchKernelGGL(flip ? k_preprocess_crops_affine_flip : k_preprocess_crops_affine, crop_grid(out_h, out_w, n_total), dim3(256), 0,
                       (hipStream_t)stream, n, (const uint8_t* const*)dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, box_scale, out_h,
                       out_w, out_c, (uint16_t*)dev_out_bf16, antialias ? 1 : 0, dev_eff_xywh);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_preprocess_crops_udp(void* stream, int n, int n_total, int flip, const void* const* dev_frames, int frame_h, int frame_w,
                                        const int32_t* dev_view_of, const float* dev_boxes, float box_scale, int out_h, int out_w,
                                        int out_c, void* dev_out_bf16, int antialias, float* dev_eff_xywh) {
    if (!crop_args_ok(n, n_total, flip ? 2 : 1, dev_frames, dev_view_of, dev_boxes, dev_out_bf16, out_h, out_w, out_c) || !dev_eff_xywh ||
        !(box_scale > 0.0f) || out_w < 2 || out_h < 2)                 // the pitch divides by out_w - 1, out_h - 1
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    hipLaunchKernelGGL(flip ? k_preprocess_crops_udp_flip : k_preprocess_crops_udp, crop_grid(out_h, out_w, n_total), dim3(256), 0,
                       (hipStream_t)stream, n, (const uint8_t* const*)dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, box_scale, out_h,
                       out_w, out_c, (uint16_t*)dev_out_bf16, antialias ? 1 : 0, dev_eff_xywh);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_box_cs(void* stream, int n, const float* dev_boxes, int out_w, int out_h, float box_scale, float* dev_eff_xywh) {
    if (n < 0 || !dev_boxes || !dev_eff_xywh || out_w <= 0 || out_h <= 0 || !(box_scale > 0.0f)) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    hipLaunchKernelGGL(k_box_cs, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, dev_boxes, out_w, out_h, box_scale, dev_eff_xywh);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_box_cs_host(int n, const float* boxes, int out_w, int out_h, float box_scale, float* eff) {
    if (n < 0 || (n > 0 && (!boxes || !eff)) || out_w <= 0 || out_h <= 0 || !(box_scale > 0.0f)) return PAM_E_ARG;
    for (int i = 0; i < n; ++i) {
        const PamBoxCs e = pam_box_cs_fn(boxes[i * 4 + 0], boxes[i * 4 + 1], boxes[i * 4 + 2], boxes[i * 4 + 3], out_w, out_h, box_scale);
        store_box(eff + i * 4, e);
    }
    return PAM_OK;
}
