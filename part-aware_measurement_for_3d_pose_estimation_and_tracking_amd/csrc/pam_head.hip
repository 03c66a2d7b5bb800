// libpam_hip.so, head part of a1 (HRNetPose.predict post-processing; call site: the reference's src/ivclabpose.py:210).
// The pose network's final 1x1 convolution behind the conv stack (csrc/pam_conv.hip and its pam_conv_*.hip kernel families) and the keypoint
// decodes behind it: arg-max, soft-arg-max, flip test with quarter-pixel offset, DARK, and heat-maps already in memory.  HBM-bound streaming
// kernels.  Shared parts first (candidates, keypoint rows, the FMA step of k_head), then the kernels, then the entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

#define J PAM_J
// ---- candidates ------------------------------------------------------------------------------------------------------------------------
struct Best { float v; int i; };
__device__ __forceinline__ Best no_best() { Best b; b.v = -__builtin_huge_valf(); b.i = 0x7fffffff; return b; }      // nothing yet
__device__ __forceinline__ int best_cell(Best b) { return b.i == 0x7fffffff ? 0 : b.i; }    // no value was greater than -inf (a map of -inf or NaN): cell 0, as np.argmax
__device__ __forceinline__ Best better(Best a, Best b) {    // larger value wins; ties -> smaller flat index (np.argmax)
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <int LANES>
__device__ __forceinline__ Best lanes_argmax(Best x) {      // butterfly over aligned groups of LANES lanes: every lane gets the result
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) {
        Best o; o.v = __shfl_xor(x.v, off, 64); o.i = __shfl_xor(x.i, off, 64);
        x = better(x, o);
    }
    return x;
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
// ---- keypoint rows -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double* det_row_of(double* det, const int* view_of, const int* slot_of, int max_dets, int crop) {
    return det + ((size_t)view_of[crop] * max_dets + slot_of[crop]) * J * 3;
}
__device__ __forceinline__ float* kp_row_of(float* kp, int crop) { return kp ? kp + (size_t)crop * J * 3 : nullptr; }
__device__ __forceinline__ void write_keypoint_at(int j, double py, double pxx, float score, int hm_h, int hm_w, const float* box,
                                                  double* det_row, float* kp_row) {
    // upstream SimpleHRNet.predict: pt / (res // 4) * box extent + box origin, stored float32
    const float y = (float)(py / (double)hm_h * (double)box[3] + (double)box[1]);
    const float x = (float)(pxx / (double)hm_w * (double)box[2] + (double)box[0]);
    det_row[j * 3 + 0] = (double)y; det_row[j * 3 + 1] = (double)x; det_row[j * 3 + 2] = (double)score;
    if (kp_row) { kp_row[j * 3 + 0] = x; kp_row[j * 3 + 1] = y; kp_row[j * 3 + 2] = score; }
}
__device__ __forceinline__ void write_keypoint(int j, Best b, int hm_h, int hm_w, const float* box, double* det_row, float* kp_row) {
    const int cell = best_cell(b);
    write_keypoint_at(j, (double)(cell / hm_w), (double)(cell % hm_w), b.v, hm_h, hm_w, box, det_row, kp_row);
}

// ---- the head's FMA chain: float32, over the channels in order, bias first -------------------------------------------------------------
// Features NHWC bf16 (C channels, C % 8 == 0), weights float32 [joint][C].  Every kernel below that needs a value of the head's map forms
// it in the same unpack and FMA order, so the value has the map's own bits wherever it is recomputed.  k_head uses fma8 below; k_head_argmax,
// k_head_argmax_flip and head_chain spell the same statements out in their own text (see k_head_argmax).
__device__ __forceinline__ void bf16x8_to_f32(const uint4 v, float (&x)[8]) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[2 * k] = bf16_lo(d[k]); x[2 * k + 1] = bf16_hi(d[k]); }
}
// One 16-byte piece of a pixel's features (channels c8 .. c8 + 7) into the JN running sums: joints outside, channels in order inside.
template <int JN>
__device__ __forceinline__ void fma8(float (&acc)[JN], const uint4 v, const float* ws, int C, int c8) {
    float x[8];
    bf16x8_to_f32(v, x);
#pragma unroll
    for (int j = 0; j < JN; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j] = fmaf(x[k], ws[j * C + c8 + k], acc[j]);
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
// ---- flip test: M[j][y][x] = 0.5f * (P[j][y][x] + F[pair(j)][y][xs]) ---------------------------------------------------------------------
// The official HRNet / Simple Baselines test protocol (FLIP_TEST, SHIFT_HEATMAP, POST_PROCESS): P / F the head's maps of the plain / the
// mirrored crop, pair() the COCO left/right swap, xs = w - 1 - x, or with the one-column shift xs = w - x for x >= 1 and w - 1 at x = 0 (the
// official flipped[..., 1:] = flipped[..., :-1] after the flip-back: column 0 keeps its own value).  One float32 add, then an exact halving.
__host__ __device__ constexpr int flip_pair(int j) { return j == 0 ? 0 : ((j & 1) ? j + 1 : j - 1); }      // 1<->2, 3<->4, ... 15<->16
__device__ __forceinline__ int flip_column(int x, int hm_w, int shift) { return shift ? (x ? hm_w - x : hm_w - 1) : hm_w - 1 - x; }
#define HEAD_T 256            // a tile: 256 consecutive flat pixels of one crop, one per thread
__device__ __forceinline__ size_t cand_at(int crop, int tiles, int tile, int j) { return ((size_t)crop * tiles + tile) * J + j; }
// ---- decode of heat-maps in memory -----------------------------------------------------------------------------------------------------
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
    for (int j = 0; j < J; ++j) best[j] = no_best();
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
        Best b = lanes_argmax<64>(best[j]);
        if (lane == 0) red[wave][j] = b;
    }
    __syncthreads();
    if (tid < J) {
        Best b = red[0][tid];
#pragma unroll
        for (int w = 1; w < DEC_T / 64; ++w) b = better(b, red[w][tid]);
        double* row = det_row_of(det, view_of, slot_of, max_dets, crop);
        write_keypoint(tid, b, hm_h, hm_w, boxes + crop * 4, row, kp_row_of(kp, crop));
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
    Best b = no_best();
    for (int e = tid; e < HW; e += 256) { const float v = src[e]; if (v > b.v) { b.v = v; b.i = e; } }
    b = lanes_argmax<64>(b);
    if ((tid & 63) == 0) red[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        b = better(better(red[0], red[1]), better(red[2], red[3]));
        double* row = det_row_of(det, view_of, slot_of, max_dets, crop);
        write_keypoint(j, b, hm_h, hm_w, boxes + crop * 4, row, kp_row_of(kp, crop));
    }
}

// ---- final 1x1 convolution of the pose network: features NHWC bf16 (C channels) -> heat-maps NHWC float32 (J maps) ----------------
// One thread per pixel: 16-byte feature loads, the J x C float32 weights broadcast from LDS, J running sums in registers; the
// workgroup's 256 x J outputs are contiguous in memory and leave through LDS as full 16-byte stores.  Streaming: C*2 bytes in, J*4 bytes
// out per pixel.
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
        for (int c8 = 0; c8 < C; c8 += 8) fma8(acc, *(const uint4*)(f + c8), ws, C, c8);
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

// ---- head + arg-max in one pass: the heat-maps never reach memory ----------------------------------------------------------------
// First pass, one workgroup per tile: every thread has its pixel's J values in registers (the chain above, so the values are
// bit-identical to k_head's), optionally stores them to `heat`, and the tile reduction writes J candidates to cand[crop][tile][J].
// Second pass, a finish kernel per decode: the fold over the tiles in order, then the keypoint rows.
// The weights come through the kernel argument: scalar loads (3.3 KB, resident in the scalar cache) instead of an LDS copy broadcast-read
// 204 times per thread.  Head + finish 17.0 -> 15.5 us at 20 crops (13 us of it is there at 8 crops too: two launches and their serial
// chains).
// This kernel and k_head_argmax_flip keep the chain and the tile reduction, the three finish kernels behind them the tile fold, in their own
// text (why: DESIGN.md, section 10p).  A change to the unpack, the FMA order, the staging pitch or the tie rule is made in every one of
// them AND in fma8 / head_chain; tests/test_gpu_flip.py, test_gpu_dark.py and test_gpu_image_shapes.py hold all forms to the same bits.
template <int JN, bool SOFT>
__global__ __launch_bounds__(HEAD_T) void k_head_argmax(int HW, int tiles, const uint16_t* __restrict__ feat, int C,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ heat /* optional */, Best* __restrict__ cand,
                                                        int hm_w, float beta, Soft* __restrict__ scand /* SOFT only */) {
    extern __shared__ __attribute__((aligned(16))) float hsm[];       // layout: head_argmax_lds() below
    const float* __restrict__ ws = w; Best* red = (Best*)(hsm + JN * C);
    const int crop = blockIdx.x / tiles, tile = blockIdx.x - crop * tiles;
    const int lp = tile * HEAD_T + threadIdx.x;                       // pixel inside the crop = flat heat-map index
    const bool ok = lp < HW;
    float acc[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[j] = bias ? bias[j] : 0.0f;
    if (ok) {
        const uint16_t* f = feat + ((size_t)crop * HW + lp) * C;
        auto piece = [&](const uint4 v, int c8) {
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
            for (int q = 0; q < 6; ++q) piece(v[q], 8 * q);
        } else {
            for (int c8 = 0; c8 < C; c8 += 8) piece(*(const uint4*)(f + c8), c8);
        }
        if (heat) {
            float* o = heat + ((size_t)crop * HW + lp) * JN;
#pragma unroll
            for (int j = 0; j < JN; ++j) o[j] = acc[j];
        }
    }
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
            // every lane of the joint holds the tile's maximum: second pass over the same LDS values, weights relative to it, then plain
            // sums over the 8 lanes (all on the same maximum)
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
// k_head_argmax with a second accumulator set fed from pixel (y, xs) of crop flip_row0 + crop.  A tile may straddle rows, the mirrored
// pixel may lie in another tile's range (it is only read).  The lanes of a row segment read their mirrored pixels at descending addresses,
// each still as full 16-byte pieces.  The joint swap is a compile-time permutation of registers.
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

// arg-max finish: one lane per joint
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
// soft-arg-max finish: one lane per joint merges the tiles' partials in order and writes the expected (column, row) through the box;
// the score is the maximum, as in the hard decode
__global__ __launch_bounds__(64) void k_softmax_finish(int tiles, const Soft* __restrict__ scand, float beta, int hm_h, int hm_w,
                                                       const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                       const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                       float* __restrict__ kp) {
    const int crop = blockIdx.x, j = threadIdx.x;
    if (j >= J) return;
    Soft a; a.m = -__builtin_huge_valf(); a.s = 0.f; a.sx = 0.f; a.sy = 0.f;
    for (int t = 0; t < tiles; ++t) a = soft_merge(a, scand[cand_at(crop, tiles, t, j)], beta);
    double* row = det_row_of(det, view_of, slot_of, max_dets, crop);
    const double inv = a.s > 0.f ? 1.0 / (double)a.s : 0.0;
    write_keypoint_at(j, (double)a.sy * inv, (double)a.sx * inv, a.m, hm_h, hm_w, boxes + crop * 4, row, kp_row_of(kp, crop));
}
// arg-max finish with the official get_final_preds offset: at an arg-max strictly inside (1 < px < w - 1 and 1 < py < h - 1) the cell
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

// ---- UDP decode (Huang et al., "The Devil is in the Details: Delving into Unbiased Data Processing for Human Pose Estimation", CVPR 2020):
// the UDP form of DARK and the align-corners cell mapping -- contract in include/pam.h ---------------------------------------------------
// The mapping: a cell is a point of the grid whose first and last points are the effective box's edges, pitch We / (hm_w - 1).
__device__ __forceinline__ void write_keypoint_udp(int j, double py, double pxx, float score, int hm_h, int hm_w, const float* box,
                                                   double* det_row, float* kp_row) {
    // UDP's transform_preds: pt * (box extent / (size - 1)) + box origin, stored float32
    const float y = (float)((double)box[1] + py * ((double)box[3] / (double)(hm_h - 1)));
    const float x = (float)((double)box[0] + pxx * ((double)box[2] / (double)(hm_w - 1)));
    det_row[j * 3 + 0] = (double)y; det_row[j * 3 + 1] = (double)x; det_row[j * 3 + 2] = (double)score;
    if (kp_row) { kp_row[j * 3 + 0] = x; kp_row[j * 3 + 1] = y; kp_row[j * 3 + 2] = score; }
}
// blur_kernel == 0: k_argmax_finish with the UDP mapping, one lane per joint
__global__ __launch_bounds__(64) void k_argmax_finish_udp(int tiles, const Best* __restrict__ cand, int hm_h, int hm_w,
                                                          const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                          const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                          float* __restrict__ kp) {
    const int crop = blockIdx.x, j = threadIdx.x;
    if (j >= J) return;
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
    const int cell = best_cell(b);
    write_keypoint_udp(j, (double)(cell / hm_w), (double)(cell % hm_w), b.v, hm_h, hm_w, boxes + crop * 4,
                       det_row_of(det, view_of, slot_of, max_dets, crop), kp_row_of(kp, crop));
}
// The plan of k_dark_finish with UDP's step (mmpose post_dark_udp).  The blur reflects at the map's border (BORDER_REFLECT_101) and the log map
// is read edge-replicated, so every winner takes the step, border and corner winners too: no workgroup leaves before the last barrier.
// The seven samples sit at the clamped cells (py + dy, px + dx); their taps lie inside the (2R + 3)^2 window round the winner (19 x 19 at
// k = 17), whose cell (wy, wx) holds M at the REFLECTED cell of (py - R - 1 + wy, px - R - 1 + wx): an in-map cell, never a zero.
//   1. every thread folds the tile candidates (the same loads)
//   2. window -> LDS as float32: one chain per thread and step (MERGE: as k_dark_finish)
//   3. horizontal pass, float64, ascending taps: the 3 clamped columns px - 1, px, px + 1 of all 2R + 3 rows
//   4. vertical pass over those: the 7 cells
//   5. thread 0: clamp into [0.001, 50], 7 logarithms, the 2 x 2 solve with e = 2^-23 on the diagonal, write_keypoint_udp
__device__ __forceinline__ int reflect101(int i, int n) {            // n >= 2; holds however far outside i lies
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}
#define UDP_W 19              // 2 R + 3 at the largest blur, k = 17
template <bool MERGE>
__global__ __launch_bounds__(DARK_T) void k_udp_finish(int tiles, const Best* __restrict__ cand, int hm_h, int hm_w,
                                                       const uint16_t* __restrict__ feat, int C, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int flip_row0, int shift, int R, DarkTaps taps,
                                                       const int* __restrict__ view_of, const int* __restrict__ slot_of,
                                                       const float* __restrict__ boxes, int max_dets, double* __restrict__ det,
                                                       float* __restrict__ kp) {
    __shared__ float win[MERGE ? 2 : 1][UDP_W * UDP_W];
    __shared__ double bh[UDP_W * 3];
    __shared__ double bv[7];
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
    if (b.i == 0x7fffffff) b.i = 0;        // no value above -inf: cell 0 (it takes the step like any other cell)
    const int py = b.i / hm_w, px = b.i - py * hm_w, HW = hm_h * hm_w;
    const int W = 2 * R + 3, cells = W * W, y0 = py - R - 1, x0 = px - R - 1, k = 2 * R + 1;
    for (int i = tid; i < (MERGE ? 2 : 1) * cells; i += DARK_T) {
        const int part = i >= cells, c = i - part * cells;
        const int wy = c / W, wx = c - wy * W, y = reflect101(y0 + wy, hm_h), x = reflect101(x0 + wx, hm_w);
        win[part][c] = part ? head_chain(feat + ((size_t)(flip_row0 + crop) * HW + y * hm_w + flip_column(x, hm_w, shift)) * C, C, w, bias, flip_pair(j))
                            : head_chain(feat + ((size_t)crop * HW + y * hm_w + x) * C, C, w, bias, j);
    }
    __syncthreads();
    if constexpr (MERGE) {
        for (int c = tid; c < cells; c += DARK_T) win[0][c] = 0.5f * (win[0][c] + win[1][c]);
        __syncthreads();
    }
    for (int i = tid; i < W * 3; i += DARK_T) {                        // B_h[row][clamp(px - 1 + d)]: window columns cx - px + 1 .. + 2R
        const int r = i / 3, d = i - r * 3;
        const int o = min(max(px - 1 + d, 0), hm_w - 1) - px + 1;
        double s = 0.0;
        for (int t = 0; t < k; ++t) s += taps.g[t] * (double)win[0][r * W + o + t];
        bh[i] = s;
    }
    __syncthreads();
    if (tid < 7) {                                                     // (dy, dx) of cell tid: 0 | x+1 x-1 | y+1 y-1 | ++ --
        const int dy = tid == 3 || tid == 5 ? 1 : (tid == 4 || tid == 6 ? -1 : 0);
        const int dx = tid == 1 || tid == 5 ? 1 : (tid == 2 || tid == 6 ? -1 : 0);
        const int o = min(max(py + dy, 0), hm_h - 1) - py + 1;         // window rows cy - py + 1 .. + 2R
        double s = 0.0;
        for (int t = 0; t < k; ++t) s += taps.g[t] * bh[(o + t) * 3 + 1 + dx];
        bv[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double L[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) L[q] = log(bv[q] > 0.001 ? (bv[q] < 50.0 ? bv[q] : 50.0) : 0.001);      // (a NaN clamps to 0.001)
    const double gx = 0.5 * (L[1] - L[2]), gy = 0.5 * (L[3] - L[4]);
    const double dxx = L[1] - 2.0 * L[0] + L[2], dyy = L[3] - 2.0 * L[0] + L[4];
    const double dxy = 0.5 * (L[5] - L[1] - L[3] + 2.0 * L[0] - L[2] - L[4] + L[6]);
    const double e = 1.1920928955078125e-07;                           // np.finfo(np.float32).eps on the diagonal
    const double hxx = dxx + e, hyy = dyy + e, dt = hxx * hyy - dxy * dxy;
    double ox = 0.0, oy = 0.0;
    if (dt != 0.0 && isfinite(dt)) {                                   // -H'^-1 g; nothing clamps the step
        ox = -(hyy * gx - dxy * gy) / dt;
        oy = -(hxx * gy - dxy * gx) / dt;
    }
    write_keypoint_udp(j, (double)py + oy, (double)px + ox, b.v, hm_h, hm_w, boxes + crop * 4,
                       det_row_of(det, view_of, slot_of, max_dets, crop), kp_row_of(kp, crop));
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------------
static bool head_ok(int n, const void* feat, const float* w, int C, int J_) { return n >= 0 && feat && w && C > 0 && C % 8 == 0 && J_ == PAM_J; }
// what every pam_head_decode* entry requires (bias, the heat-map and the kp pointer may be null)
static bool head_decode_ok(int n, int hm_h, int hm_w, const void* feat, int C, const float* w, int J_, const int32_t* view_of,
                           const int32_t* slot_of, const float* boxes, const double* det, const void* scratch) {
    return head_ok(n, feat, w, C, J_) && view_of && slot_of && boxes && det && scratch && hm_h > 0 && hm_w > 0;
}
static bool flip_flags_ok(int flags, int allowed, int n, int flip_row0) {
    const int merge = flags & PAM_FLIP_MERGE;
    return !(flags & ~allowed) && !((flags & PAM_FLIP_SHIFT) && !merge) && !(merge && flip_row0 < n);
}
static int head_tiles(int hm_h, int hm_w) { return (hm_h * hm_w + HEAD_T - 1) / HEAD_T; }
// Dynamic LDS of k_head_argmax: JN * C floats and Best[4][JN] that nothing reads any more (the weights once sat there, and the waves'
// partial maxima), then the [HEAD_T][JN + 1] staging of the tile reduction.  The dead part stays: dropping it changes the occupancy, which is a
// measured change of its own.
static size_t head_stage_lds() { return (size_t)HEAD_T * (J + 1) * sizeof(float); }       // the [HEAD_T][JN + 1] staging of the tile reduction
static size_t head_argmax_lds(int C) { return (size_t)J * C * sizeof(float) + (size_t)(HEAD_T / 64) * J * sizeof(Best) + head_stage_lds(); }
static DarkTaps gaussian_taps(int blur_kernel) {                       // OpenCV's getGaussianKernel(k, 0): sigma from k, taps normalised to 1
    DarkTaps taps;
    const int R = (blur_kernel - 1) / 2;
    const double sigma = 0.3 * ((blur_kernel - 1) * 0.5 - 1.0) + 0.8;
    double sum = 0.0;
    for (int i = 0; i < 17; ++i) {
        taps.g[i] = i < blur_kernel ? exp(-(double)((i - R) * (i - R)) / (2.0 * sigma * sigma)) : 0.0;
        sum += taps.g[i];
    }
    for (int i = 0; i < 17; ++i) taps.g[i] /= sum;
    return taps;
}
static int launched() { return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP; }

// The first pass of every decode: the tile candidates of n crops into `scratch` (Best[n][tiles][J]; beta > 0: also the soft partials,
// 16-byte records behind the 8-byte ones -- n * tiles * 17 * 8 is a multiple of 8; merge: plain + mirrored rows).  -> tiles
static int head_first_pass(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias, float* heat,
                           void* scratch, float beta, int merge, int flip_row0, int shift) {
    const int HW = hm_h * hm_w, tiles = head_tiles(hm_h, hm_w);
    const dim3 grid(n * tiles), block(HEAD_T);
    const hipStream_t st = (hipStream_t)stream;
    const uint16_t* feat = (const uint16_t*)feat_bf16;
    Best* cand = (Best*)scratch;
    if (merge)
        hipLaunchKernelGGL((k_head_argmax_flip<PAM_J>), grid, block, head_stage_lds(), st, HW, tiles, feat, C, w, bias, heat, cand, hm_w, flip_row0, shift);
    else if (beta > 0.0f)
        hipLaunchKernelGGL((k_head_argmax<PAM_J, true>), grid, block, head_argmax_lds(C), st, HW, tiles, feat, C, w, bias, heat, cand, hm_w, beta,
                           (Soft*)(cand + (size_t)n * tiles * J));
    else
        hipLaunchKernelGGL((k_head_argmax<PAM_J, false>), grid, block, head_argmax_lds(C), st, HW, tiles, feat, C, w, bias, heat, cand, hm_w, 0.0f,
                           (Soft*)nullptr);
    return tiles;
}

extern "C" int pam_head_heatmaps(void* stream, int n_pix, const void* feat_bf16, int C, const float* w, const float* bias, int J_, float* out) {
    if (!head_ok(n_pix, feat_bf16, w, C, J_) || !out || (HEAD_T * J_) % 4 != 0) return PAM_E_ARG;
    if (n_pix == 0) return PAM_OK;
    const size_t lds = ((size_t)J_ * C + (size_t)HEAD_T * J_) * sizeof(float);
    hipLaunchKernelGGL((k_head<PAM_J>), dim3((n_pix + HEAD_T - 1) / HEAD_T), dim3(HEAD_T), lds, (hipStream_t)stream, n_pix,
                       (const uint16_t*)feat_bf16, C, w, bias, out);
    return launched();
}

extern "C" long long pam_head_decode_scratch_bytes(int n, int hm_h, int hm_w) {
    if (n < 0 || hm_h <= 0 || hm_w <= 0) return -1;
    const long long tiles = ((long long)hm_h * hm_w + HEAD_T - 1) / HEAD_T;
    return (long long)n * tiles * J * (long long)sizeof(Best);
}
extern "C" long long pam_head_decode_soft_scratch_bytes(int n, int hm_h, int hm_w) {
    const long long b = pam_head_decode_scratch_bytes(n, hm_h, hm_w);
    return b < 0 ? b : b + b / (long long)sizeof(Best) * (long long)sizeof(Soft);
}
extern "C" long long pam_head_decode_flip_scratch_bytes(int n, int hm_h, int hm_w) { return pam_head_decode_scratch_bytes(n, hm_h, hm_w); }
extern "C" long long pam_head_decode_dark_scratch_bytes(int n, int hm_h, int hm_w) { return pam_head_decode_scratch_bytes(n, hm_h, hm_w); }
extern "C" int pam_head_decode(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias,
                               int J_, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                               const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (!head_decode_ok(n, hm_h, hm_w, feat_bf16, C, w, J_, dev_view_of, dev_slot_of, dev_boxes, dev_det, dev_scratch)) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int tiles = head_first_pass(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, dev_heatmaps_or_null, dev_scratch, 0.0f, 0, 0, 0);
    hipLaunchKernelGGL(k_argmax_finish, dim3(n), dim3(64), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w,
                       dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return launched();
}
// the same pass with a soft-arg-max decode: keypoint = sum_p softmax(beta * heat)_p * (column, row)_p per joint (sub-pixel), score = max
extern "C" int pam_head_decode_soft(void* stream, int n, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w, const float* bias,
                                    int J_, float beta, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                                    const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (!head_decode_ok(n, hm_h, hm_w, feat_bf16, C, w, J_, dev_view_of, dev_slot_of, dev_boxes, dev_det, dev_scratch) || !(beta > 0.0f))
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int tiles = head_first_pass(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, dev_heatmaps_or_null, dev_scratch, beta, 0, 0, 0);
    hipLaunchKernelGGL(k_softmax_finish, dim3(n), dim3(64), 0, (hipStream_t)stream, tiles, (const Soft*)((const Best*)dev_scratch + (size_t)n * tiles * J), beta,
                       hm_h, hm_w, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return launched();
}
// flip test and / or the quarter-pixel offset; without MERGE the offset is taken on the plain maps and the mirrored rows are never read
extern "C" int pam_head_decode_flip(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                                    const float* bias, int J_, int flags, float* dev_heatmaps_or_null, const int32_t* dev_view_of, const int32_t* dev_slot_of,
                                    const float* dev_boxes, int max_dets, double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (!head_decode_ok(n, hm_h, hm_w, feat_bf16, C, w, J_, dev_view_of, dev_slot_of, dev_boxes, dev_det, dev_scratch) ||
        !flip_flags_ok(flags, PAM_FLIP_MERGE | PAM_FLIP_SHIFT | PAM_FLIP_QUARTER, n, flip_row0))
        return PAM_E_ARG;
    if (flags == 0)                                                    // nothing asked for: pam_head_decode itself
        return pam_head_decode(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, J_, dev_heatmaps_or_null, dev_view_of, dev_slot_of, dev_boxes,
                               max_dets, dev_det, dev_kp_xyc, dev_scratch);
    if (n == 0) return PAM_OK;
    const int merge = flags & PAM_FLIP_MERGE, shift = (flags & PAM_FLIP_SHIFT) ? 1 : 0, post = (flags & PAM_FLIP_QUARTER) ? 1 : 0;
    const int tiles = head_first_pass(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, dev_heatmaps_or_null, dev_scratch, 0.0f, merge, flip_row0, shift);
    hipLaunchKernelGGL(merge ? k_argmax_finish_flip<true> : k_argmax_finish_flip<false>, dim3(n), dim3(FIN_T), 0, (hipStream_t)stream, tiles,
                       (const Best*)dev_scratch, hm_h, hm_w, (const uint16_t*)feat_bf16, C, w, bias, merge ? flip_row0 : 0, shift, post, dev_view_of, dev_slot_of,
                       dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return launched();
}
extern "C" int pam_head_decode_dark(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                                    const float* bias, int J_, int flags, int blur_kernel, float* dev_heatmaps_or_null,
                                    const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes, int max_dets,
                                    double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (!head_decode_ok(n, hm_h, hm_w, feat_bf16, C, w, J_, dev_view_of, dev_slot_of, dev_boxes, dev_det, dev_scratch) ||
        !flip_flags_ok(flags, PAM_FLIP_MERGE | PAM_FLIP_SHIFT, n, flip_row0) || blur_kernel < 9 || blur_kernel > 17 || blur_kernel % 2 == 0)
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int merge = flags & PAM_FLIP_MERGE, shift = (flags & PAM_FLIP_SHIFT) ? 1 : 0, R = (blur_kernel - 1) / 2;
    const DarkTaps taps = gaussian_taps(blur_kernel);
    const int tiles = head_first_pass(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, dev_heatmaps_or_null, dev_scratch, 0.0f, merge, flip_row0, shift);
    hipLaunchKernelGGL(merge ? k_dark_finish<true> : k_dark_finish<false>, dim3(n * J), dim3(DARK_T), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch,
                       hm_h, hm_w, (const uint16_t*)feat_bf16, C, w, bias, merge ? flip_row0 : 0, shift, R, taps, dev_view_of, dev_slot_of, dev_boxes, max_dets,
                       dev_det, dev_kp_xyc);
    return launched();
}
extern "C" long long pam_head_decode_udp_scratch_bytes(int n, int hm_h, int hm_w) {
    return hm_h < 2 || hm_w < 2 ? -1 : pam_head_decode_scratch_bytes(n, hm_h, hm_w);
}
extern "C" int pam_head_decode_udp(void* stream, int n, int flip_row0, int hm_h, int hm_w, const void* feat_bf16, int C, const float* w,
                                   const float* bias, int J_, int flags, int blur_kernel, float* dev_heatmaps_or_null,
                                   const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes, int max_dets,
                                   double* dev_det, float* dev_kp_xyc, void* dev_scratch) {
    if (!head_decode_ok(n, hm_h, hm_w, feat_bf16, C, w, J_, dev_view_of, dev_slot_of, dev_boxes, dev_det, dev_scratch) ||
        !flip_flags_ok(flags, PAM_FLIP_MERGE | PAM_FLIP_SHIFT, n, flip_row0) || hm_h < 2 || hm_w < 2 ||
        (blur_kernel != 0 && (blur_kernel < 9 || blur_kernel > 17 || blur_kernel % 2 == 0)))
        return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    const int merge = flags & PAM_FLIP_MERGE, shift = (flags & PAM_FLIP_SHIFT) ? 1 : 0;
    const int tiles = head_first_pass(stream, n, hm_h, hm_w, feat_bf16, C, w, bias, dev_heatmaps_or_null, dev_scratch, 0.0f, merge, flip_row0, shift);
    if (blur_kernel == 0)                                              // no sub-pixel step: the plain arg-max of M through the UDP mapping
        hipLaunchKernelGGL(k_argmax_finish_udp, dim3(n), dim3(64), 0, (hipStream_t)stream, tiles, (const Best*)dev_scratch, hm_h, hm_w, dev_view_of,
                           dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    else
        hipLaunchKernelGGL(merge ? k_udp_finish<true> : k_udp_finish<false>, dim3(n * J), dim3(DARK_T), 0, (hipStream_t)stream, tiles,
                           (const Best*)dev_scratch, hm_h, hm_w, (const uint16_t*)feat_bf16, C, w, bias, merge ? flip_row0 : 0, shift,
                           (blur_kernel - 1) / 2, gaussian_taps(blur_kernel), dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return launched();
}
extern "C" int pam_decode_heatmaps(void* stream, int n, const float* dev_heatmaps, int nchw, int hm_h, int hm_w,
                                   const int32_t* dev_view_of, const int32_t* dev_slot_of, const float* dev_boxes,
                                   int max_dets, double* dev_det, float* dev_kp_xyc) {
    if (n < 0 || !dev_heatmaps || !dev_view_of || !dev_slot_of || !dev_boxes || !dev_det || hm_h <= 0 || hm_w <= 0) return PAM_E_ARG;
    if (n == 0) return PAM_OK;
    hipLaunchKernelGGL(nchw ? k_decode_nchw : k_decode_nhwc, dim3(nchw ? n * J : n), dim3(nchw ? 256 : DEC_T), 0, (hipStream_t)stream, n,
                       dev_heatmaps, hm_h, hm_w, dev_view_of, dev_slot_of, dev_boxes, max_dets, dev_det, dev_kp_xyc);
    return launched();
}
