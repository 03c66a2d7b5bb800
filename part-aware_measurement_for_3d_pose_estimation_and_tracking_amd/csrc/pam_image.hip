// libpam_hip.so, image part of a1 (HRNetPose.predict pre/post-processing; call site /root/reference/src/ivclabpose.py:210).
// Crop / resize / normalise in front of the conv stack (csrc/pam_conv.hip and its pam_conv_*.hip kernel families, csrc/pam_block.hip), the network's final 1x1
// convolution and the arg-max decode behind it.  All HBM-bound streaming kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"
#include "pam_box_cs.hpp"

#define J PAM_J

// One thread per output pixel: bilinear sample (half-pixel centres, border replicate) of the person box from the BGR
// uint8 frame, BGR->RGB, /255, ImageNet mean/std, bf16 NHWC store (6 B per thread, contiguous across the wave).
// antialias: the resize of upstream simple-HRNet (a PIL image through torchvision's Resize) filters with a triangle whose support grows
// with the down-scaling factor; plain bilinear interpolation (the default here, = cv2.resize INTER_LINEAR / F.interpolate(bilinear)) only
// ever reads 2 x 2 pixels.  The two agree for boxes no larger than the network input; HD boxes taller than 384 pixels are down-scaled.
// With antialias the taps are the frame pixels i whose centres lie within max(scale, 1) of the output pixel's centre, inside the box
// rounded outwards (the crop upstream cuts), weights 1 - |i + 0.5 - centre| / max(scale, 1), normalised (PIL's ImagingResample formula,
// in float32: PIL's own uint8 rounding between its two passes is not reproduced).  Crops n_src .. (grid) repeat crop n_src - 1: a replay
// bucket larger than the call (HRNetPose pads a batch to a multiple of graph_bucket) needs no padded box table.
constexpr int AA_MAXT = 24;             // taps per axis at most (down-scaling by up to 11.5)
#define CROP_KERNEL k_preprocess_crops
#define CROP_FLIP 0
#include "pam_crop_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
#define CROP_KERNEL k_preprocess_crops_flip             // plain + mirrored rows of a flip-test forward (see pam_crop_kernel.inc)
#define CROP_FLIP 1
#include "pam_crop_kernel.inc"
#undef CROP_KERNEL
#undef CROP_FLIP
// The pose checkpoints' own crop geometry (pam_box_cs.hpp, pam_crop_affine_kernel.inc): the box widened to the input's aspect about its
// centre and enlarged, sampled with ONE scale and a zero border -- forms NEXT to the two above, whose instructions stay what they were.
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
// the whole effective-box table without a crop (a rank of the crop-sharded predict() crops its share but filters every row)
__global__ __launch_bounds__(256) void k_box_cs(int n, const float* __restrict__ boxes, int ow, int oh, float box_scale, float* __restrict__ eff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PamBoxCs e = pam_box_cs_fn(boxes[i * 4 + 0], boxes[i * 4 + 1], boxes[i * 4 + 2], boxes[i * 4 + 3], ow, oh, box_scale);
    eff[i * 4 + 0] = e.x; eff[i * 4 + 1] = e.y; eff[i * 4 + 2] = e.w; eff[i * 4 + 3] = e.h;
}

struct Best { float v; int i; };
__device__ __forceinline__ Best better(Best a, Best b) {    // larger value wins; ties -> smaller flat index (np.argmax)
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ Best wave_argmax(Best x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Best o; o.v = __shfl_xor(x.v, off, 64); o.i = __shfl_xor(x.i, off, 64);
        x = better(x, o);
    }
    return x;
}
__device__ __forceinline__ void write_keypoint_at(int j, double py, double pxx, float score, int hm_h, int hm_w, const float* box,
                                                  double* det_row, float* kp_row) {
    // upstream SimpleHRNet.predict: pt / (res // 4) * box extent + box origin, stored float32
    const float y = (float)(py / (double)hm_h * (double)box[3] + (double)box[1]);
    const float x = (float)(pxx / (double)hm_w * (double)box[2] + (double)box[0]);
    det_row[j * 3 + 0] = (double)y; det_row[j * 3 + 1] = (double)x; det_row[j * 3 + 2] = (double)score;
    if (kp_row) { kp_row[j * 3 + 0] = x; kp_row[j * 3 + 1] = y; kp_row[j * 3 + 2] = score; }
}
__device__ __forceinline__ void write_keypoint(int j, Best b, int hm_h, int hm_w, const float* box, double* det_row, float* kp_row) {
    if (b.i == 0x7fffffff) b.i = 0;        // no value was greater than -inf (a map of -inf or NaN): cell 0, as np.argmax
    write_keypoint_at(j, (double)(b.i / hm_w), (double)(b.i % hm_w), b.v, hm_h, hm_w, box, det_row, kp_row);
}
// soft-arg-max partial of one joint over a set of pixels: m = max, s = sum exp(beta (v - m)), sx / sy = the same sum weighted with the
// pixel's column / row.  Two partials merge by rescaling both to the larger maximum (the usual streaming softmax).
struct Soft { float m, s, sx, sy; };
__device__ __forceinline__ Soft soft_merge(Soft a, Soft b, float beta) {
    if (b.s == 0.0f) return a;
    if (a.s == 0.0f) return b;
    const float m = fmaxf(a.m, b.m), fa = __expf(beta * (a.m - m)), fb = __expf(beta * (b.m - m));
    Soft r; r.m = m; r.s = a.s * fa + b.s * fb; r.sx = a.sx * fa + b.sx * fb; r.sy = a.sy * fa + b.sy * fb;
    return r;
}

// NHWC heat-maps (n, H, W, 17) float32: one workgroup per person.  Pixel tiles of 256 x 17 floats are staged through LDS
// with coalesced 16-byte loads; each lane then owns one pixel and reads its 17 values at stride 17 words (odd stride:
// conflict-free), keeping 17 running (max, index) pairs in registers.
#define TILE_PX 1024
#define DEC_T 1024            // 16 waves per person: only n (~20) workgroups exist, so each one is as wide as it can be
__global__ __launch_bounds__(DEC_T) void k_decode_nhwc(int n, const float* __restrict__ hm, int hm_h, int hm_w,
                                                     const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                     const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                     float* __restrict__ kp) {
    __shared__ __attribute__((aligned(16))) float tile[TILE_PX * J];
    __shared__ Best red[DEC_T / 64][J];
    const int crop = blockIdx.x, tid = threadIdx.x;
    const int HW = hm_h * hm_w;
    const float* src = hm + (size_t)crop * HW * J;
    Best best[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { best[j].v = -__builtin_huge_valf(); best[j].i = 0x7fffffff; }
    for (int base = 0; base < HW; base += TILE_PX) {
        const int npx = min(TILE_PX, HW - base);
        const int nfl = npx * J;
        const float* g = src + (size_t)base * J;
        if ((nfl & 3) == 0 && (((uintptr_t)g & 15) == 0)) {
            const float4* g4 = (const float4*)g; float4* t4 = (float4*)tile;
            for (int e = tid; e < nfl / 4; e += DEC_T) t4[e] = g4[e];
        } else {
            for (int e = tid; e < nfl; e += DEC_T) tile[e] = g[e];
        }
        __syncthreads();
        if (tid < npx) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float v = tile[tid * J + j];
                if (v > best[j].v) { best[j].v = v; best[j].i = base + tid; }   // strictly greater: earlier index wins ties
            }
        }
        __syncthreads();
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        Best b = wave_argmax(best[j]);
        if (lane == 0) red[wave][j] = b;
    }
    __syncthreads();
    if (tid < J) {
        Best b = red[0][tid];
#pragma unroll
        for (int w = 1; w < DEC_T / 64; ++w) b = better(b, red[w][tid]);
        double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
        write_keypoint(tid, b, hm_h, hm_w, boxes + crop * 4, row, kp ? kp + (size_t)crop * J * 3 : nullptr);
    }
}

// NCHW heat-maps (n, 17, H, W): one workgroup per (person, joint), plain coalesced scan.
__global__ __launch_bounds__(256) void k_decode_nchw(int n, const float* __restrict__ hm, int hm_h, int hm_w,
                                                     const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                     const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                     float* __restrict__ kp) {
    __shared__ Best red[4];
    const int crop = blockIdx.x / J, j = blockIdx.x % J, tid = threadIdx.x;
    const int HW = hm_h * hm_w;
    const float* src = hm + ((size_t)crop * J + j) * HW;
    Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
    for (int e = tid; e < HW; e += 256) { const float v = src[e]; if (v > b.v) { b.v = v; b.i = e; } }
    b = wave_argmax(b);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        b = better(better(red[0], red[1]), better(red[2], red[3]));
        double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
        write_keypoint(j, b, hm_h, hm_w, boxes + crop * 4, row, kp ? kp + (size_t)crop * J * 3 : nullptr);
    }
}

// ---- final 1x1 convolution of the pose network: features NHWC bf16 (C channels) -> heat-maps NHWC float32 (J maps) ----------------
// One thread per pixel: 16-byte feature loads, the J x C float32 weights broadcast from LDS, J running sums in registers
// (float32 FMA chain over the channels in order, bias first); the workgroup's 256 x J outputs are contiguous in memory and
// leave through LDS as full 16-byte stores.  Streaming: C*2 bytes in, J*4 bytes out per pixel.
#define HEAD_T 256
template <int JN>
__global__ __launch_bounds__(HEAD_T) void k_head(int npix, const uint16_t* __restrict__ feat, int C, const float* __restrict__ w,
                                                 const float* __restrict__ bias, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];       // [JN*C] weights, then [HEAD_T*JN] output staging
    float* ws = hsm; float* os = hsm + JN * C;
    for (int i = threadIdx.x; i < JN * C; i += HEAD_T) ws[i] = w[i];
    __syncthreads();
    const int px = blockIdx.x * HEAD_T + threadIdx.x;
    float acc[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[j] = bias ? bias[j] : 0.0f;
    if (px < npix) {
        const uint16_t* f = feat + (size_t)px * C;
        for (int c8 = 0; c8 < C; c8 += 8) {
            const uint4 v = *(const uint4*)(f + c8);
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            float x[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[2 * k] = bf16_lo(d[k]); x[2 * k + 1] = bf16_hi(d[k]); }
#pragma unroll
            for (int j = 0; j < JN; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[j] = fmaf(x[k], ws[j * C + c8 + k], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < JN; ++j) os[threadIdx.x * JN + j] = acc[j];
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * HEAD_T * JN;             // this workgroup's outputs: [base, base + HEAD_T*JN) floats
    const size_t total = (size_t)npix * JN;
    for (int i = threadIdx.x * 4; i < HEAD_T * JN; i += HEAD_T * 4) {
        if (base + i + 3 < total) *(float4*)(out + base + i) = *(const float4*)(os + i);
        else for (int k = 0; k < 4; ++k) if (base + i + k < total) out[base + i + k] = os[i + k];
    }
}

extern "C" int pam_head_heatmaps(void* stream, int n_pix, const void* feat_bf16, int C, const float* w, const float* bias,
                                 int J_, float* out) {
    if (n_pix < 0 || !feat_bf16 || !w || !out || C <= 0 || C % 8 != 0 || J_ != PAM_J || (HEAD_T * J_) % 4 != 0) return PAM_E_ARG;
    if (n_pix == 0) return PAM_OK;
    const size_t lds = ((size_t)J_ * C + (size_t)HEAD_T * J_) * sizeof(float);
    hipLaunchKernelGGL((k_head<PAM_J>), dim3((n_pix + HEAD_T - 1) / HEAD_T), dim3(HEAD_T), lds, (hipStream_t)stream, n_pix,
                       (const uint16_t*)feat_bf16, C, w, bias, out);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---- head + arg-max in one pass: the heat-maps never reach memory ----------------------------------------------------------------
// k_head_argmax: workgroup = 256 consecutive pixels of ONE crop; every thread has its pixel's J values in registers (same FMA
// chain as k_head, so the values are bit-identical), the workgroup reduces (max, first index) per joint -- wave shuffles, then
// LDS staging, 8 lanes per joint -- and writes J candidates to cand[crop][tile][J].  k_argmax_finish: one wave per crop folds the
// tiles in order (strictly greater replaces: the lowest flat index wins ties, np.argmax's rule) and writes the keypoint rows.
template <int JN, bool SOFT>
__global__ __launch_bounds__(HEAD_T) void k_head_argmax(int HW, int tiles, const uint16_t* __restrict__ feat, int C,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ heat /* optional */, Best* __restrict__ cand,
                                                        int hm_w, float beta, Soft* __restrict__ scand /* SOFT only */) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];       // [JN*C] (unused: see ws), then Best[4][JN]
    // The weights are read through the kernel argument with wave-uniform indices: scalar loads (3.3 KB, resident in the scalar cache) feeding
    // the FMAs as SGPR operands, instead of an LDS copy broadcast-read 204 times per thread.  Head + finish 17.0 -> 15.5 us at 20 crops
    // (13 us of it is there at 8 crops too: two launches and their serial chains); the FMA chain and its order are unchanged.
    const float* __restrict__ ws = w; Best* red = (Best*)(hsm + JN * C);
    const int crop = blockIdx.x / tiles, tile = blockIdx.x - crop * tiles;
    const int lp = tile * HEAD_T + threadIdx.x;                       // pixel inside the crop = flat heat-map index
    const bool ok = lp < HW;
    float acc[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[j] = bias ? bias[j] : 0.0f;
    if (ok) {
        const uint16_t* f = feat + ((size_t)crop * HW + lp) * C;
        auto fma8 = [&](const uint4 v, int c8) {
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            float x[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) { x[2 * k] = bf16_lo(d[k]); x[2 * k + 1] = bf16_hi(d[k]); }
#pragma unroll
            for (int j = 0; j < JN; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[j] = fmaf(x[k], ws[j * C + c8 + k], acc[j]);
        };
        if (C == 48) {                                   // HRNet-W48: all six 16-byte pieces of the pixel in flight at once (same FMA order)
            uint4 v[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) v[q] = *(const uint4*)(f + 8 * q);
#pragma unroll
            for (int q = 0; q < 6; ++q) fma8(v[q], 8 * q);
        } else {
            for (int c8 = 0; c8 < C; c8 += 8) fma8(*(const uint4*)(f + c8), c8);
        }
        if (heat) {
            float* o = heat + ((size_t)crop * HW + lp) * JN;
#pragma unroll
            for (int j = 0; j < JN; ++j) o[j] = acc[j];
        }
    }
    // per-joint (max, first index) over the workgroup's 256 pixels: the values go through LDS pixel-major (pitch JN + 1 words), then
    // 8 lanes per joint scan 32 pixels each -- lane `part` takes pixels part, part + 8, ...: increasing index inside a lane, and the 8
    // lanes of a joint read 8 consecutive rows (different banks; blocks of 32 rows would all fall on one) -- and fold by 3 shuffles
    float* vs = (float*)(red + (HEAD_T / 64) * JN);                   // [HEAD_T][JN + 1]
#pragma unroll
    for (int j = 0; j < JN; ++j) vs[threadIdx.x * (JN + 1) + j] = ok ? acc[j] : -__builtin_huge_valf();
    __syncthreads();
    if (threadIdx.x < JN * 8) {
        const int j = threadIdx.x >> 3, part = threadIdx.x & 7;
        Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
#pragma unroll 8
        for (int q = 0; q < HEAD_T / 8; ++q) {
            const int px = q * 8 + part;
            const float v = vs[px * (JN + 1) + j];
            if (v > b.v) { b.v = v; b.i = tile * HEAD_T + px; }            // strictly greater: the first maximum of the part
        }
#pragma unroll
        for (int off = 4; off >= 1; off >>= 1) {
            Best o; o.v = __shfl_xor(b.v, off, 64); o.i = __shfl_xor(b.i, off, 64);
            b = better(b, o);
        }
        if (part == 0) cand[((size_t)crop * tiles + tile) * JN + j] = b;
        if constexpr (SOFT) {
            // after the butterfly every lane of the joint holds the tile's maximum: second pass over the same LDS values, weights
            // relative to it, then plain sums over the 8 lanes (all on the same maximum)
            float s0 = 0.f, sx = 0.f, sy = 0.f;
            if (b.v > -__builtin_huge_valf()) {
#pragma unroll 8
                for (int q = 0; q < HEAD_T / 8; ++q) {
                    const int px = q * 8 + part, lp2 = tile * HEAD_T + px;
                    const float e = __expf(beta * (vs[px * (JN + 1) + j] - b.v));       // pixels past the crop hold -inf: weight 0
                    const int yy = lp2 / hm_w, xx = lp2 - yy * hm_w;
                    s0 += e; sx += e * (float)xx; sy += e * (float)yy;
                }
            }
#pragma unroll
            for (int off = 4; off >= 1; off >>= 1) { s0 += __shfl_xor(s0, off, 64); sx += __shfl_xor(sx, off, 64); sy += __shfl_xor(sy, off, 64); }
            if (part == 0) { Soft r; r.m = b.v; r.s = s0; r.sx = sx; r.sy = sy; scand[((size_t)crop * tiles + tile) * JN + j] = r; }
        }
    }
}
// soft-arg-max finish: one lane per joint merges the tiles' partials in order and writes the expected (column, row) through the box;
// the score is the maximum, as in the hard decode
__global__ __launch_bounds__(64) void k_softmax_finish(int tiles, const Soft* __restrict__ scand, float beta, int hm_h, int hm_w,
                                                       const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                       const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                       float* __restrict__ kp) {
    const int crop = blockIdx.x, j = threadIdx.x;
    if (j >= J) return;
    Soft a; a.m = -__builtin_huge_valf(); a.s = 0.f; a.sx = 0.f; a.sy = 0.f;
    for (int t = 0; t < tiles; ++t) a = soft_merge(a, scand[((size_t)crop * tiles + t) * J + j], beta);
    double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
    const double inv = a.s > 0.f ? 1.0 / (double)a.s : 0.0;
    write_keypoint_at(j, (double)a.sy * inv, (double)a.sx * inv, a.m, hm_h, hm_w, boxes + crop * 4, row, kp ? kp + (size_t)crop * J * 3 : nullptr);
}
__global__ __launch_bounds__(64) void k_argmax_finish(int tiles, const Best* __restrict__ cand, int hm_h, int hm_w,
                                                      const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                      const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                      float* __restrict__ kp) {
    const int crop = blockIdx.x, j = threadIdx.x;
    if (j >= J) return;
    Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
    for (int t0 = 0; t0 < tiles; t0 += 8) {                          // 8 candidates in flight at a time (a serial chain of 27 loads took 11 us)
        Best c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int t = min(t0 + q, tiles - 1);
            c[q] = cand[((size_t)crop * tiles + t) * J + j];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (t0 + q < tiles && c[q].v > b.v) b = c[q];            // tiles are in index order: strictly greater keeps the first maximum
    }
    double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
    write_keypoint(j, b, hm_h, hm_w, boxes + crop * 4, row, kp ? kp + (size_t)crop * J * 3 : nullptr);
}

extern "C" long long pam_head_decode_scratch_bytes(int n, int hm_h, int hm_w) {
    if (n < 0 || hm_h <= 0 || hm_w <= 0) return -1;
    const long long tiles = ((long long)hm_h * hm_w + HEAD_T - 1) / HEAD_T;
    return (long long)n * tiles * J * (long long)sizeof(Best);
}

extern "C" int pam_head_decode(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias,
                               int J_, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                               const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (n < 0 || !feat_bf16 || !w || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || !dev_scratch || hm_h <= 0 || hm_w <= 0 ||
        C <= 0 || C % 8 != 0 || J_ != PAM_J)
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int HW = hm_h * hm_w, tiles = (HW + HEAD_T - 1) / HEAD_T;
    const size_t lds = (size_t)J_ * C * sizeof(float) + (size_t)(HEAD_T / 64) * J_ * sizeof(Best) + (size_t)HEAD_T * (J_ + 1) * sizeof(float);
    hipLaunchKernelGGL((k_head_argmax<PAM_J, false>), dim3(n * tiles), dim3(HEAD_T), lds, (hipStream_t)stream, HW, tiles,
                       (const uint16_t*)feat_bf16, C, w, bias, dev_heatmaps_or_null, (Best*)dev_scratch, hm_w, 0.0f, (Soft*)nullptr);
    hipLaunchKernelGGL(k_argmax_finish, dim3(n), dim3(64), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                       dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// the same pass with a soft-arg-max decode: keypoint = sum_p softmax(beta * heat)_p * (column, row)_p per joint (sub-pixel), score = max
extern "C" long long pam_head_decode_soft_scratch_bytes(int n, int hm_h, int hm_w) {
    const long long b = pam_head_decode_scratch_bytes(n, hm_h, hm_w);
    return b < 0 ? b : b + b / (long long)sizeof(Best) * (long long)sizeof(Soft);
}
extern "C" int pam_head_decode_soft(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias,
                                    int J_, float beta, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                                    const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (n < 0 || !feat_bf16 || !w || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || !dev_scratch || hm_h <= 0 || hm_w <= 0 ||
        C <= 0 || C % 8 != 0 || J_ != PAM_J || !(beta > 0.0f))
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int HW = hm_h * hm_w, tiles = (HW + HEAD_T - 1) / HEAD_T;
    const size_t lds = (size_t)J_ * C * sizeof(float) + (size_t)(HEAD_T / 64) * J_ * sizeof(Best) + (size_t)HEAD_T * (J_ + 1) * sizeof(float);
    Best* cand = (Best*)dev_scratch;
    Soft* scand = (Soft*)(cand + (size_t)n * tiles * J_);                 // 16-byte records behind the 8-byte ones (n * tiles * 17 * 8 is a multiple of 8)
    hipLaunchKernelGGL((k_head_argmax<PAM_J, true>), dim3(n * tiles), dim3(HEAD_T), lds, (hipStream_t)stream, HW, tiles,
                       (const uint16_t*)feat_bf16, C, w, bias, dev_heatmaps_or_null, cand, hm_w, beta, scand);
    hipLaunchKernelGGL(k_softmax_finish, dim3(n), dim3(64), 0, (hipStream_t)stream, tiles, (const Soft*)scand, beta, hm_h, hm_w,
                       dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---- flip test: head of a plain and a mirrored crop merged in registers, arg-max, optional quarter-pixel offset -------------------------
// The official HRNet / Simple Baselines test protocol (FLIP_TEST, SHIFT_HEATMAP, POST_PROCESS): M[j][y][x] = 0.5f * (P[j][y][x] +
// F[pair(j)][y][xs]) with P / F the head's maps of the plain / the mirrored crop (the FMA chain of k_head, bit for bit), pair() the COCO
// left/right swap, xs = w - 1 - x, or with the one-column shift xs = w - x for x >= 1 and w - 1 at x = 0 (the official
// flipped[..., 1:] = flipped[..., :-1] after the flip-back: column 0 keeps its own value).  One float32 add, then an exact halving.
__host__ __device__ constexpr int flip_pair(int j) { return j == 0 ? 0 : ((j & 1) ? j + 1 : j - 1); }      // 1<->2, 3<->4, ... 15<->16
__device__ __forceinline__ int flip_column(int x, int hm_w, int shift) { return shift ? (x ? hm_w - x : hm_w - 1) : hm_w - 1 - x; }

// k_head_argmax_flip: k_head_argmax with a second accumulator set fed from pixel (y, xs) of crop flip_row0 + crop.  Workgroup = 256
// consecutive flat pixels of one crop; a tile may straddle rows, the mirrored pixel may lie in another tile's range (it is only read).
// The lanes of a row segment read their mirrored pixels at descending addresses, each still as full 16-byte pieces.  The joint swap is
// a compile-time permutation of registers.  Weights through wave-uniform scalar loads as in k_head_argmax.
template <int JN>
__global__ __launch_bounds__(HEAD_T) void k_head_argmax_flip(int HW, int tiles, const uint16_t* __restrict__ feat, int C,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ heat /* optional */, Best* __restrict__ cand,
                                                             int hm_w, int flip_row0, int shift) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];       // [HEAD_T][JN + 1]: the merged values on their way to the reduction
    const float* __restrict__ ws = w;
    const int crop = blockIdx.x / tiles, tile = blockIdx.x - crop * tiles;
    const int lp = tile * HEAD_T + threadIdx.x;
    const bool ok = lp < HW;
    float acc[JN], acf[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[j] = acf[j] = bias ? bias[j] : 0.0f;
    if (ok) {
        const int y = lp / hm_w, x = lp - y * hm_w;
        const uint16_t* f = feat + ((size_t)crop * HW + lp) * C;
        const uint16_t* g = feat + ((size_t)(flip_row0 + crop) * HW + y * hm_w + flip_column(x, hm_w, shift)) * C;
        auto fma8 = [&](float (&a)[JN], const uint4 v, int c8) {
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            float xk[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) { xk[2 * k] = bf16_lo(d[k]); xk[2 * k + 1] = bf16_hi(d[k]); }
#pragma unroll
            for (int j = 0; j < JN; ++j)
#pragma unroll
                for (int k = 0; k < 8; ++k) a[j] = fmaf(xk[k], ws[j * C + c8 + k], a[j]);
        };
        if (C == 48) {                                   // HRNet-W48: the six pieces of each of the two pixels in flight at once
            uint4 v[6], u[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) { v[q] = *(const uint4*)(f + 8 * q); u[q] = *(const uint4*)(g + 8 * q); }
#pragma unroll
            for (int q = 0; q < 6; ++q) { fma8(acc, v[q], 8 * q); fma8(acf, u[q], 8 * q); }
        } else {
            for (int c8 = 0; c8 < C; c8 += 8) {
                const uint4 v = *(const uint4*)(f + c8), u = *(const uint4*)(g + c8);
                fma8(acc, v, c8); fma8(acf, u, c8);
            }
        }
#pragma unroll
        for (int j = 0; j < JN; ++j) acc[j] = 0.5f * (acc[j] + acf[flip_pair(j)]);
        if (heat) {
            float* o = heat + ((size_t)crop * HW + lp) * JN;
#pragma unroll
            for (int j = 0; j < JN; ++j) o[j] = acc[j];
        }
    }
    // the reduction of k_head_argmax: values through LDS pixel-major, 8 lanes per joint scan 32 pixels each, 3 shuffles
    float* vs = hsm;                                                  // [HEAD_T][JN + 1]
#pragma unroll
    for (int j = 0; j < JN; ++j) vs[threadIdx.x * (JN + 1) + j] = ok ? acc[j] : -__builtin_huge_valf();
    __syncthreads();
    if (threadIdx.x < JN * 8) {
        const int j = threadIdx.x >> 3, part = threadIdx.x & 7;
        Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
#pragma unroll 8
        for (int q = 0; q < HEAD_T / 8; ++q) {
            const int px = q * 8 + part;
            const float v = vs[px * (JN + 1) + j];
            if (v > b.v) { b.v = v; b.i = tile * HEAD_T + px; }            // strictly greater: the first maximum of the part
        }
#pragma unroll
        for (int off = 4; off >= 1; off >>= 1) {
            Best o; o.v = __shfl_xor(b.v, off, 64); o.i = __shfl_xor(b.i, off, 64);
            b = better(b, o);
        }
        if (part == 0) cand[((size_t)crop * tiles + tile) * JN + j] = b;
    }
}
// One value of the head's map of joint jj at the pixel whose features start at f, recomputed with the head's own chain: the map's own bits.
__device__ __forceinline__ float head_chain(const uint16_t* __restrict__ f, int C, const float* __restrict__ w, const float* __restrict__ bias, int jj) {
    float a = bias ? bias[jj] : 0.0f;
    for (int c8 = 0; c8 < C; c8 += 8) {
        const uint4 v = *(const uint4*)(f + c8);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a = fmaf(bf16_lo(d[k]), w[jj * C + c8 + 2 * k], a);
            a = fmaf(bf16_hi(d[k]), w[jj * C + c8 + 2 * k + 1], a);
        }
    }
    return a;
}
// k_argmax_finish with the official get_final_preds offset: at an arg-max strictly inside (1 < px < w - 1 and 1 < py < h - 1) the cell
// moves a quarter towards the higher neighbour along each axis; a difference that is neither > 0 nor < 0 (zero, NaN) moves nothing.
// The winner is known only after the fold, so its four neighbours are recomputed from the features: 8 lanes per joint, lane `part`
// takes neighbour part & 3 (x + 1, x - 1, y + 1, y - 1) of the plain (part < 4) or the mirrored crop (MERGE only) -- one chain of C FMAs
// each, side by side (one lane per joint ran the 8 chains one after the other: + 9 us at C = 48, + 26 us at C = 256 for 20 crops) --
// and three shuffles form the merged values and the two differences.  Every lane of a joint folds the tiles (the same loads).
#define FIN_T 192             // 17 joints x 8 lanes = 136 lanes in 3 waves; a joint's 8 lanes sit in one wave
template <bool MERGE>
__global__ __launch_bounds__(FIN_T) void k_argmax_finish_flip(int tiles, const Best* __restrict__ cand, int hm_h, int hm_w,
                                                              const uint16_t* __restrict__ feat, int C, const float* __restrict__ w,
                                                              const float* __restrict__ bias, int flip_row0, int shift, int post,
                                                              const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                              const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                              float* __restrict__ kp) {
    const int crop = blockIdx.x, j = threadIdx.x >> 3, part = threadIdx.x & 7;
    if (j >= J) return;                                  // whole 8-lane groups leave: no shuffle below reads a lane that left
    Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
    for (int t0 = 0; t0 < tiles; t0 += 8) {
        Best c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int t = min(t0 + q, tiles - 1);
            c[q] = cand[((size_t)crop * tiles + t) * J + j];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (t0 + q < tiles && c[q].v > b.v) b = c[q];
    }
    if (b.i == 0x7fffffff) b.i = 0;        // no value above -inf: cell 0 (never strictly inside: no offset)
    const int py = b.i / hm_w, px = b.i - py * hm_w, HW = hm_h * hm_w;
    const bool inside = post && 1 < px && px < hm_w - 1 && 1 < py && py < hm_h - 1;      // the same for the 8 lanes of a joint
    float v = 0.0f;
    if (inside && (MERGE || part < 4)) {
        const int c = part & 3, y = py + (c == 2) - (c == 3), x = px + (c == 0) - (c == 1);
        v = part < 4 ? head_chain(feat + ((size_t)crop * HW + y * hm_w + x) * C, C, w, bias, j)
                     : head_chain(feat + ((size_t)(flip_row0 + crop) * HW + y * hm_w + flip_column(x, hm_w, shift)) * C, C, w, bias, flip_pair(j));
    }
    if constexpr (MERGE) v = 0.5f * (v + __shfl_xor(v, 4, 64));       // lanes 0 .. 3: plain + mirrored, the sum k_head_argmax_flip forms
    const float e = v - __shfl_xor(v, 1, 64);                        // lane 0: M[py][px+1] - M[py][px-1]; lane 2: M[py+1][px] - M[py-1][px]
    const float ey = __shfl_xor(e, 2, 64);
    if (part != 0) return;
    double dy = 0.0, dx = 0.0;
    if (inside) {
        dx = e > 0.0f ? 0.25 : (e < 0.0f ? -0.25 : 0.0);
        dy = ey > 0.0f ? 0.25 : (ey < 0.0f ? -0.25 : 0.0);
    }
    double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
    write_keypoint_at(j, (double)py + dy, (double)px + dx, b.v, hm_h, hm_w, boxes + crop * 4, row, kp ? kp + (size_t)crop * J * 3 : nullptr);
}

extern "C" long long pam_head_decode_flip_scratch_bytes(int n, int hm_h, int hm_w) { return pam_head_decode_scratch_bytes(n, hm_h, hm_w); }

extern "C" int pam_head_decode_flip(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                                    const float* bias, int J_, int flags, float* dev_heatmaps_or_null, const int32_t* dev_view_of,
                                    const int32_t* dev_slot_of, const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc,
                                    void* dev_scratch) {
    const int merge = flags & PAM_FLIP_MERGE, shift = (flags & PAM_FLIP_SHIFT) ? 1 : 0, post = (flags & PAM_FLIP_QUARTER) ? 1 : 0;
    if (n < 0 || !feat_bf16 || !w || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || !dev_scratch || hm_h <= 0 || hm_w <= 0 ||
        C <= 0 || C % 8 != 0 || J_ != PAM_J || (flags & ~(PAM_FLIP_MERGE | PAM_FLIP_SHIFT | PAM_FLIP_QUARTER)) || (shift && !merge) ||
        (merge && flip_row0 < n))
        return PAM_E_ARG;
    if (flags == 0)                                                    // nothing asked for: pam_head_decode itself
        return pam_head_decode(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, J_, dev_heatmaps_or_null, dev_view_of, dev_slot_of, dev_boxes,
                               max_dets, dev_det, dev_kp_xyc, dev_scratch);
    if (n == 0) return PAM_OK;
    const int HW = hm_h * hm_w, tiles = (HW + HEAD_T - 1) / HEAD_T;
    const uint16_t* f = (const uint16_t*)feat_bf16;
    if (merge) {
        hipLaunchKernelGGL((k_head_argmax_flip<PAM_J>), dim3(n * tiles), dim3(HEAD_T), (size_t)HEAD_T * (J_ + 1) * sizeof(float),
                           (hipStream_t)stream, HW, tiles, f, C, w, bias, dev_heatmaps_or_null, (Best*)dev_scratch, hm_w, flip_row0, shift);
        hipLaunchKernelGGL((k_argmax_finish_flip<true>), dim3(n), dim3(FIN_T), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                           f, C, w, bias, flip_row0, shift, post, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    } else {                                                           // quarter-pixel offset on the plain maps: the mirrored rows are never read
        const size_t lds = (size_t)J_ * C * sizeof(float) + (size_t)(HEAD_T / 64) * J_ * sizeof(Best) + (size_t)HEAD_T * (J_ + 1) * sizeof(float);
        hipLaunchKernelGGL((k_head_argmax<PAM_J, false>), dim3(n * tiles), dim3(HEAD_T), lds, (hipStream_t)stream, HW, tiles, f, C, w, bias,
                           dev_heatmaps_or_null, (Best*)dev_scratch, hm_w, 0.0f, (Soft*)nullptr);
        hipLaunchKernelGGL((k_argmax_finish_flip<false>), dim3(n), dim3(FIN_T), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                           f, C, w, bias, 0, 0, post, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    }
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---- DARK decode (Zhang et al., CVPR 2020): Gaussian blur, logarithm, one Newton step at the arg-max -- contract in include/pam.h --------
// The winner is known only after the fold, and the step needs the blurred map at 13 cells round it: the cross px +- 2 / py +- 2 and the four
// diagonal neighbours.  Those depend on the (2R + 5)^2 window of M round the winner (R = (k - 1) / 2; 21 x 21 at k = 17), which is recomputed
// from the features with head_chain -- the map's own bits, as in k_argmax_finish_flip -- so the maps still never reach memory.
// One workgroup per (crop, joint): the joint is uniform, so the weight row of every chain comes through scalar loads.
//   1. every thread folds the tile candidates (the same loads); a winner outside 1 < px < w - 2, 1 < py < h - 2 is written as it is
//   2. window -> LDS as float32, 0 outside the map: one chain per thread and step (MERGE: the mirrored crop's chains of joint pair(j) are
//      further steps of the same loop, then one pass forms 0.5f * (p + f), the sum k_head_argmax_flip forms)
//   3. horizontal pass, float64, ascending taps: the 5 columns px - 2 .. px + 2 of all 2R + 5 rows
//   4. vertical pass over those: the 13 cells
//   5. thread 0: clamp at 1e-10, 13 logarithms, the 2 x 2 solve, write_keypoint_at
// The taps are the host's doubles, passed by value; t is wave-uniform in both passes, so they too are scalar operands.
struct DarkTaps { double g[17]; };
#define DARK_T 256
#define DARK_W 21             // 2 R + 5 at the largest blur, k = 17
template <bool MERGE>
__global__ __launch_bounds__(DARK_T) void k_dark_finish(int tiles, const Best* __restrict__ cand, int hm_h, int hm_w,
                                                        const uint16_t* __restrict__ feat, int C, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int flip_row0, int shift, int R, DarkTaps taps,
                                                        const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                        const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                        float* __restrict__ kp) {
    __shared__ float win[MERGE ? 2 : 1][DARK_W * DARK_W];
    __shared__ double bh[DARK_W * 5];
    __shared__ double bv[13];
    const int crop = blockIdx.x / J, j = blockIdx.x - crop * J, tid = threadIdx.x;
    Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff;
    for (int t0 = 0; t0 < tiles; t0 += 8) {
        Best c[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int t = min(t0 + q, tiles - 1);
            c[q] = cand[((size_t)crop * tiles + t) * J + j];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (t0 + q < tiles && c[q].v > b.v) b = c[q];
    }
    if (b.i == 0x7fffffff) b.i = 0;        // no value above -inf: cell 0 (never inside: no offset)
    const int py = b.i / hm_w, px = b.i - py * hm_w, HW = hm_h * hm_w;
    double* row = det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
    float* kp_row = kp ? kp + (size_t)crop * J * 3 : nullptr;
    if (!(1 < px && px < hm_w - 2 && 1 < py && py < hm_h - 2)) {       // the same for the whole workgroup: nobody waits at a barrier below
        if (tid == 0) write_keypoint_at(j, (double)py, (double)px, b.v, hm_h, hm_w, boxes + crop * 4, row, kp_row);
        return;
    }
    const int W = 2 * R + 5, cells = W * W, y0 = py - R - 2, x0 = px - R - 2, k = 2 * R + 1;
    for (int i = tid; i < (MERGE ? 2 : 1) * cells; i += DARK_T) {
        const int part = i >= cells, c = i - part * cells;
        const int wy = c / W, wx = c - wy * W, y = y0 + wy, x = x0 + wx;
        float v = 0.0f;
        if (y >= 0 && y < hm_h && x >= 0 && x < hm_w)
            v = part ? head_chain(feat + ((size_t)(flip_row0 + crop) * HW + y * hm_w + flip_column(x, hm_w, shift)) * C, C, w, bias, flip_pair(j))
                     : head_chain(feat + ((size_t)crop * HW + y * hm_w + x) * C, C, w, bias, j);
        win[part][c] = v;
    }
    __syncthreads();
    if constexpr (MERGE) {
        for (int c = tid; c < cells; c += DARK_T) win[0][c] = 0.5f * (win[0][c] + win[1][c]);      // (outside the map: 0.5f * (0 + 0))
        __syncthreads();
    }
    for (int i = tid; i < W * 5; i += DARK_T) {                        // B_h[row][px - 2 + d]: window columns d .. d + 2R
        const int r = i / 5, d = i - r * 5;
        double s = 0.0;
        for (int t = 0; t < k; ++t) s += taps.g[t] * (double)win[0][r * W + d + t];
        bh[i] = s;
    }
    __syncthreads();
    if (tid < 13) {                                                    // (dy, dx) of cell tid: 0 | x+1 x-1 x+2 x-2 | y+1 y-1 y+2 y-2 | ++ -+ +- --
        const int dy = tid < 5 ? 0 : (tid < 9 ? ((tid & 1) ? 1 : -1) * (tid < 7 ? 1 : 2) : ((tid & 1) ? 1 : -1));
        const int dx = tid == 0 || (tid >= 5 && tid < 9) ? 0 : (tid < 5 ? ((tid & 1) ? 1 : -1) * (tid < 3 ? 1 : 2) : (tid < 11 ? 1 : -1));
        double s = 0.0;
        for (int t = 0; t < k; ++t) s += taps.g[t] * bh[(2 + dy + t) * 5 + 2 + dx];     // window rows 2 + dy .. 2 + dy + 2R
        bv[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double L[13];
#pragma unroll
    for (int q = 0; q < 13; ++q) L[q] = log(bv[q] > 1e-10 ? bv[q] : 1e-10);                // (a NaN clamps too)
    const double gx = 0.5 * (L[1] - L[2]), gy = 0.5 * (L[5] - L[6]);
    const double dxx = 0.25 * (L[3] - 2.0 * L[0] + L[4]), dyy = 0.25 * (L[7] - 2.0 * L[0] + L[8]);
    const double dxy = 0.25 * (L[9] - L[10] - L[11] + L[12]);
    const double dt = dxx * dyy - dxy * dxy;
    double ox = 0.0, oy = 0.0;
    if (dt != 0.0) {                                                   // -H^-1 g; nothing clamps the step, as in the official code
        ox = -(dyy * gx - dxy * gy) / dt;
        oy = -(dxx * gy - dxy * gx) / dt;
    }
    write_keypoint_at(j, (double)py + oy, (double)px + ox, b.v, hm_h, hm_w, boxes + crop * 4, row, kp_row);
}

extern "C" long long pam_head_decode_dark_scratch_bytes(int n, int hm_h, int hm_w) { return pam_head_decode_scratch_bytes(n, hm_h, hm_w); }

extern "C" int pam_head_decode_dark(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                                    const float* bias, int J_, int flags, int blur_kernel, float* dev_heatmaps_or_null,
                                    const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes, int max_dets,
                                    double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    const int merge = flags & PAM_FLIP_MERGE, shift = (flags & PAM_FLIP_SHIFT) ? 1 : 0;
    if (n < 0 || !feat_bf16 || !w || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || !dev_scratch || hm_h <= 0 || hm_w <= 0 ||
        C <= 0 || C % 8 != 0 || J_ != PAM_J || (flags & ~(PAM_FLIP_MERGE | PAM_FLIP_SHIFT)) || (shift && !merge) ||
        (merge && flip_row0 < n) || blur_kernel < 9 || blur_kernel > 17 || blur_kernel % 2 == 0)
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int HW = hm_h * hm_w, tiles = (HW + HEAD_T - 1) / HEAD_T, R = (blur_kernel - 1) / 2;
    DarkTaps taps;                                                     // OpenCV's getGaussianKernel(k, 0): sigma from k, taps normalised to 1
    const double sigma = 0.3 * ((blur_kernel - 1) * 0.5 - 1.0) + 0.8;
    double sum = 0.0;
    for (int i = 0; i < 17; ++i) {
        taps.g[i] = i < blur_kernel ? exp(-(double)((i - R) * (i - R)) / (2.0 * sigma * sigma)) : 0.0;
        sum += taps.g[i];
    }
    for (int i = 0; i < 17; ++i) taps.g[i] /= sum;
    const uint16_t* f = (const uint16_t*)feat_bf16;
    if (merge) {
        hipLaunchKernelGGL((k_head_argmax_flip<PAM_J>), dim3(n * tiles), dim3(HEAD_T), (size_t)HEAD_T * (J_ + 1) * sizeof(float),
                           (hipStream_t)stream, HW, tiles, f, C, w, bias, dev_heatmaps_or_null, (Best*)dev_scratch, hm_w, flip_row0, shift);
        hipLaunchKernelGGL((k_dark_finish<true>), dim3(n * J_), dim3(DARK_T), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                           f, C, w, bias, flip_row0, shift, R, taps, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    } else {
        const size_t lds = (size_t)J_ * C * sizeof(float) + (size_t)(HEAD_T / 64) * J_ * sizeof(Best) + (size_t)HEAD_T * (J_ + 1) * sizeof(float);
        hipLaunchKernelGGL((k_head_argmax<PAM_J, false>), dim3(n * tiles), dim3(HEAD_T), lds, (hipStream_t)stream, HW, tiles, f, C, w, bias,
                           dev_heatmaps_or_null, (Best*)dev_scratch, hm_w, 0.0f, (Soft*)nullptr);
        hipLaunchKernelGGL((k_dark_finish<false>), dim3(n * J_), dim3(DARK_T), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                           f, C, w, bias, 0, 0, R, taps, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    }
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_preprocess_crops_ex(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w,
                                       const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w,
                                       int out_c, void* dev_out_bf16, int antialias) {
    if (n < 0 || n_total < n || !dev_frames || !dev_view_of || !dev_boxes || !dev_out_bf16 || out_h <= 0 || out_w <= 0 || (out_c != 3 && out_c != 8)) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    dim3 grid((out_h * out_w + 255) / 256, n_total);
    hipLaunchKernelGGL(k_preprocess_crops, grid, dim3(256), 0, (hipStream_t)stream, n, (const uint8_t* const*)dev_frames,
                       frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, (uint16_t*)dev_out_bf16, antialias ? 1 : 0);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
extern "C" int pam_preprocess_crops(void* stream, int n, const void* const* dev_frames, int frame_h, int frame_w,
                                    const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w,
                                    int out_c, void* dev_out_bf16) {
    return pam_preprocess_crops_ex(stream, n, n, dev_frames, frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, dev_out_bf16, 0);
}

extern "C" int pam_preprocess_crops_flip(void* stream, int n, int n_total, const void* const* dev_frames, int frame_h, int frame_w,
                                         const int32_t* dev_view_of, const float* dev_boxes, int out_h, int out_w,
                                         int out_c, void* dev_out_bf16, int antialias) {
    if (n < 0 || n_total < 2 * (long long)n || !dev_frames || !dev_view_of || !dev_boxes || !dev_out_bf16 || out_h <= 0 || out_w <= 0 || (out_c != 3 && out_c != 8)) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    dim3 grid((out_h * out_w + 255) / 256, n_total);
    hipLaunchKernelGGL(k_preprocess_crops_flip, grid, dim3(256), 0, (hipStream_t)stream, n, (const uint8_t* const*)dev_frames,
                       frame_h, frame_w, dev_view_of, dev_boxes, out_h, out_w, out_c, (uint16_t*)dev_out_bf16, antialias ? 1 : 0);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_preprocess_crops_affine(void* stream, int n, int n_total, int flip, const void* const* dev_frames, int frame_h, int frame_w,
                                           const int32_t* dev_view_of, const float* dev_boxes, float box_scale, int out_h, int out_w,
                                           int out_c, void* dev_out_bf16, int antialias, float* dev_eff_xywh) {
    if (n < 0 || n_total < (flip ? 2 : 1) * (long long)n || !dev_frames || !dev_view_of || !dev_boxes || !dev_out_bf16 || out_h <= 0 ||
        out_w <= 0 || (out_c != 3 && out_c != 8) || !dev_eff_xywh || !(box_scale > 0.0f))
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    dim3 grid((out_h * out_w + 255) / 256, n_total);
    if (flip)
        hipLaunchKernelGGL(k_preprocess_crops_affine_flip, grid, dim3(256), 0, (hipStream_t)stream, n, (const uint8_t* const*)dev_frames,
                           frame_h, frame_w, dev_view_of, dev_boxes, box_scale, out_h, out_w, out_c, (uint16_t*)dev_out_bf16,
                           antialias ? 1 : 0, dev_eff_xywh);
    else
        hipLaunchKernelGGL(k_preprocess_crops_affine, grid, dim3(256), 0, (hipStream_t)stream, n, (const uint8_t* const*)dev_frames,
                           frame_h, frame_w, dev_view_of, dev_boxes, box_scale, out_h, out_w, out_c, (uint16_t*)dev_out_bf16,
                           antialias ? 1 : 0, dev_eff_xywh);
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
        eff[i * 4 + 0] = e.x; eff[i * 4 + 1] = e.y; eff[i * 4 + 2] = e.w; eff[i * 4 + 3] = e.h;
    }
    return PAM_OK;
}

extern "C" int pam_decode_heatmaps(void* stream, int n, const float* dev_heatmaps, int nchw, int hm_h, int hm_w,
                                   const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes,
                                   int max_dets, double* dev_det, float* dev_kp_xyc) {
    if (n < 0 || !dev_heatmaps || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || hm_h <= 0 || hm_w <= 0) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    if (nchw)
        hipLaunchKernelGGL(k_decode_nchw, dim3(n * J), dim3(256), 0, (hipStream_t)stream, n, dev_heatmaps, hm_h, hm_w,
                           dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    else
        hipLaunchKernelGGL(k_decode_nhwc, dim3(n), dim3(DEC_T), 0, (hipStream_t)stream, n, dev_heatmaps, hm_h, hm_w,
                           dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---- measurement aid (bench.py): the shader clock the chip holds at this point of a stream ---------------------------------
// One wave spins for `ticks` periods of the 100 MHz reference counter and reports (delta s_memtime, delta s_memrealtime): shader
// clock [MHz] = 100 * d_memtime / d_memrealtime (MI355X guide, 'DVFS give-back' item 6).  Enqueued right before and right after the
// timed region it shows whether a run sat in a lower power state; it carries no data of the path.
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long* out, unsigned long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(8); r1 = __builtin_amdgcn_s_memrealtime(); }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    out[0] = c1 - c0; out[1] = r1 - r0;
}
extern "C" int pam_clock_probe(void* stream, unsigned long long* dev_out2, int microseconds) {
    if (!dev_out2 || microseconds < 1 || microseconds > 100000) return PAM_E_ARG;
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, dev_out2, (unsigned long long)microseconds * 100ull);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
