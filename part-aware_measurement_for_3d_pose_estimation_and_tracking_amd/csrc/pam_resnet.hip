// PoseResNet's own layers (poseresnet.py, hrnet_hip.HipPoseResNet): the stem -- 7x7 stride-2 convolution + bias + ReLU + 3x3 stride-2
// max-pool in one launch -- and the 4x4 stride-2 transposed convolutions of the deconvolution head.  The backbone's other layers
// are the shared conv stack's (pam_conv.hip and its pam_conv_*.hip kernel families, pam_pw.hip, pam_bneck.hip).
//
// k_resnet_stem: one workgroup per pooled output row (n, py).  Pooled row py reads conv rows 2 py - 1 .. 2 py + 1 (one halo row shared with
// each neighbour, recomputed): they are computed into LDS as bf16 after bias + ReLU ([3 rows][Wc][64]), then pooled.  The H/2 map never
// reaches HBM.  After the ReLU every value is >= 0 and every pooling window holds at least one valid cell, so the max over the valid cells
// (start 0) equals PyTorch's -inf padding; bf16 rounding is monotone, so rounding before the max equals rounding after it.
// The convolution is k_conv_stem's scheme with 7 tap rows: K per tap row = 7 taps x 8 channels, two v_mfma_f32_16x16x32_bf16 per tap row
// (taps kx = 4 s + g of lane group g; kx = 7 reads zeros).  Wave w owns output channels 32 (w & 1) .. + 31 (two n-tiles, 28 A fragments in
// registers) and every other 16-pixel tile of the three rows (w >> 1).
//
// k_deconv4x4s2: ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) + bias [+ ReLU].  Output row oy = 2 iy - 1 + ky, so output parity p
// reads two taps: row 2 m from (ky 1, input row m) and (ky 3, m - 1), row 2 m + 1 from (ky 2, m) and (ky 0, m + 1); columns alike.  Each of
// the four parity classes is a 2x2 convolution over the input grid: an implicit GEMM with M = N H W, N = Cout, K = 4 Cin.  One workgroup
// computes all four (wave w = parity 2 py + px) for a band of TR input rows (all W columns) and 64 output channels: the band's input patch
// with a one-pixel halo ((TR + 2) x (W + 2) pixels, 32 channels per k-step) sits in LDS once for the four parities, and every result goes
// straight to its interleaved output position.  A wave keeps up to 8 pixel tiles x 4 channel tiles of accumulators; its 16 weight
// fragments of a k-step come from global memory (the image is per parity: see include/pam.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

typedef __attribute__((ext_vector_type(8))) short s16x8;

struct RStemArgs { const uint16_t* in; const uint16_t* wfrag; const float* bias; uint16_t* out; int N, H, W, Hc, Wc, Hp, Wp; };

__global__ __launch_bounds__(256) void k_resnet_stem(RStemArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t conv_rows[];        // [3][Wc][64] bf16
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x / a.Hp, py = blockIdx.x - n * a.Hp;
    const int px = lane & 15, g = lane >> 4, h = wave & 1, pq = wave >> 1;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((size_t)a.N * a.H * a.W * 16), 0x00020000);
    bf16x8 wf[2][7][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                wf[jj][ky][s] = *(const bf16x8*)(a.wfrag + ((size_t)(((2 * h + jj) * 7 + ky) * 2 + s) * 64 + lane) * 8);
    f32x4 b4[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) b4[jj] = *(const f32x4*)(a.bias + 16 * g + 4 * (2 * h + jj));
    const int ntx = (a.Wc + 15) >> 4;
    for (int k = pq; k < 3 * ntx; k += 2) {
        const int r = k / ntx, t = k - r * ntx;
        const int cy = 2 * py - 1 + r;
        if (cy < 0 || cy >= a.Hc) continue;                                      // wave-uniform
        const int cx = t * 16 + px;
        f32x4 acc[2] = {b4[0], b4[1]};
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = 2 * cy + ky - 3;
            const bool rowok = iy >= 0 && iy < a.H && cx < a.Wc;
            bf16x8 b[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int kx = 4 * s + g, ix = 2 * cx + kx - 3;
                const bool ok = rowok && kx < 7 && ix >= 0 && ix < a.W;
                const unsigned off = ok ? ((unsigned)((n * a.H + iy) * a.W + ix)) * 16u : OOB_OFFSET;
                b[s] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
                    acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[jj][ky][s]),
                                                                     __builtin_bit_cast(bf16x8_t, b[s]), acc[jj], 0, 0, 0);
        }
        if (cx < a.Wc) {                                                         // channels 16 g + 8 h .. + 7 of conv pixel (cy, cx)
            uint32_t d[4];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                d[2 * jj] = pack_bf16x2(fmaxf(acc[jj][0], 0.0f), fmaxf(acc[jj][1], 0.0f));
                d[2 * jj + 1] = pack_bf16x2(fmaxf(acc[jj][2], 0.0f), fmaxf(acc[jj][3], 0.0f));
            }
            *(u32x4*)(conv_rows + ((size_t)(r * a.Wc + cx) * 64 + 16 * g + 8 * h)) = (u32x4){d[0], d[1], d[2], d[3]};
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < a.Wp * 8; e += 256) {
        const int ox = e >> 3, c8 = e & 7;
        s16x8 m = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};                              // ReLU output: bf16 bits order like int16 for values >= 0
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int cy = 2 * py - 1 + r;
            if (cy < 0 || cy >= a.Hc) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int cx = 2 * ox - 1 + dx;
                if (cx < 0 || cx >= a.Wc) continue;
                m = __builtin_elementwise_max(m, *(const s16x8*)(conv_rows + (size_t)(r * a.Wc + cx) * 64 + 8 * c8));
            }
        }
        *(s16x8*)(a.out + (((size_t)n * a.Hp + py) * a.Wp + ox) * 64 + 8 * c8) = m;
    }
}

extern "C" int pam_resnet_stem_nhwc_bf16(void* stream, const void* in, const void* wfrag, const float* bias, void* out, int N, int H, int W) {
    if (!in || !wfrag || !bias || !out || N <= 0 || H < 2 || W < 2) return PAM_E_ARG;
    RStemArgs a;
    a.in = (const uint16_t*)in; a.wfrag = (const uint16_t*)wfrag; a.bias = bias; a.out = (uint16_t*)out;
    a.N = N; a.H = H; a.W = W;
    a.Hc = (H - 1) / 2 + 1; a.Wc = (W - 1) / 2 + 1; a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;
    if (a.Wc > 192 || (size_t)N * H * W * 16 >= (1ull << 31) || (size_t)N * a.Hp * a.Wp * 64 * 2 >= (1ull << 31)) return PAM_E_ARG;
    const int lds = 3 * a.Wc * 64 * 2;
    if (!pam_max_dynamic_lds((const void*)k_resnet_stem, lds)) return PAM_E_HIP;
    pam_launch(k_resnet_stem, dim3(N * a.Hp), dim3(256), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int DC_MT = 8;                 // pixel tiles of 16 per wave: a band holds at most 128 input pixels
constexpr int DC_MAXP = 8;               // 16-byte patch pieces per thread and k-step: (TR + 2) (W + 2) <= 512 pixels
struct DeconvArgs { const uint16_t* in; const uint16_t* wimg; const float* bias; uint16_t* out; int N, H, W, Cin, Cout, TR, row_tiles, relu; };

__device__ __forceinline__ int dc_slot(int P, int q) { return P * 32 + 8 * (q ^ ((P >> 2) & 3)); }   // bf16 offset of piece q of patch pixel P

__global__ __launch_bounds__(256) void k_deconv4x4s2(DeconvArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t patch[];           // [(TR + 2) (W + 2) pixels][4 pieces, swizzled][8] bf16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int py = wave >> 1, px = wave & 1;
    const int slab = blockIdx.y;
    const int n = blockIdx.x / a.row_tiles, r0 = (blockIdx.x - n * a.row_tiles) * a.TR;
    const int rows = min(a.TR, a.H - r0), npix = rows * a.W;
    const int PW = a.W + 2, npatch = (rows + 2) * PW, npieces = 4 * npatch;
    const int ntile = (npix + 15) >> 4;
    const int col = lane & 15, g = lane >> 4;
    // the wave's four taps: offsets of the source pixel in the patch (dy, dx in {-1, 0, 1}: see DECONV_TAPS in poseresnet.py)
    const int dy1 = py ? 1 : -1, dx1 = px ? 1 : -1;
    const int toff[4] = {0, dx1, dy1 * PW, dy1 * PW + dx1};
    int pc[DC_MT];
#pragma unroll
    for (int mt = 0; mt < DC_MT; ++mt) {
        int idx = mt * 16 + col;
        if (idx >= npix) idx = npix - 1;                                          // read a real pixel, store nothing
        const int r = idx / a.W, x = idx - r * a.W;
        pc[mt] = (r + 1) * PW + x + 1;
    }
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((size_t)a.N * a.H * a.W * a.Cin * 2), 0x00020000);
    const int nc = a.Cin >> 5;
    bf16x8 pre[DC_MAXP];
    auto fetch = [&](int c) {
#pragma unroll
        for (int i = 0; i < DC_MAXP; ++i) {
            const int k = tid + 256 * i;
            const int P = k >> 2, q = k & 3;
            const int pr = P / PW, pcol = P - pr * PW;
            const int iy = r0 - 1 + pr, ix = pcol - 1;
            const bool ok = k < npieces && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const unsigned off = ok ? ((unsigned)((n * a.H + iy) * a.W + ix) * (unsigned)a.Cin + (unsigned)(32 * c + 8 * q)) * 2u : OOB_OFFSET;
            pre[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < DC_MAXP; ++i) {
            const int k = tid + 256 * i;
            if (k < npieces) *(bf16x8*)(patch + dc_slot(k >> 2, k & 3)) = pre[i];
        }
    };
    f32x4 acc[DC_MT][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 b = *(const f32x4*)(a.bias + 64 * slab + 16 * g + 4 * j);
#pragma unroll
        for (int mt = 0; mt < DC_MT; ++mt) acc[mt][j] = b;
    }
    // weight image: [parity][slab][k-step][tap][n-tile j][lane][8]
    const uint16_t* wb = a.wimg + ((size_t)(wave * (a.Cout >> 6) + slab) * nc) * (16 * 512) + lane * 8;
    fetch(0);
    store();
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
        if (c + 1 < nc) fetch(c + 1);
        const uint16_t* wc = wb + (size_t)c * (16 * 512);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            bf16x8 af[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) af[j] = *(const bf16x8*)(wc + (t * 4 + j) * 512);
#pragma unroll
            for (int mt = 0; mt < DC_MT; ++mt) {
                if (mt < ntile) {                                                 // wave-uniform
                    const int P = pc[mt] + toff[t];
                    const bf16x8 b = *(const bf16x8*)(patch + dc_slot(P, g));
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[j]), __builtin_bit_cast(bf16x8_t, b),
                                                                             acc[mt][j], 0, 0, 0);
                }
            }
        }
        if (c + 1 < nc) {
            __syncthreads();
            store();
            __syncthreads();
        }
    }
    // epilogue: lane (col, g) of tile mt holds output channels 64 slab + 16 g .. + 15 of input pixel mt * 16 + col -> output (2 iy + py, 2 x + px)
    const int Ho = 2 * a.H, Wo = 2 * a.W;
#pragma unroll
    for (int mt = 0; mt < DC_MT; ++mt) {
        const int idx = mt * 16 + col;
        if (mt < ntile && idx < npix) {
            const int r = idx / a.W, x = idx - r * a.W;
            const int oy = 2 * (r0 + r) + py, ox = 2 * x + px;
            uint32_t d[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v = acc[mt][j];
                if (a.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
                }
                d[2 * j] = pack_bf16x2(v[0], v[1]); d[2 * j + 1] = pack_bf16x2(v[2], v[3]);
            }
            uint16_t* o = a.out + (((size_t)n * Ho + oy) * Wo + ox) * a.Cout + 64 * slab + 16 * g;
            *(u32x4*)o = (u32x4){d[0], d[1], d[2], d[3]};
            *(u32x4*)(o + 8) = (u32x4){d[4], d[5], d[6], d[7]};
        }
    }
}

// rows of input per workgroup: all W columns, at most 16 * DC_MT pixels
static int deconv_rows(int H, int W) {
    int tr = (16 * DC_MT) / W;
    if (tr < 1) tr = 1;
    return tr < H ? tr : H;
}

extern "C" int pam_deconv4x4s2_nhwc_bf16(void* stream, const void* in, const void* wimg, const float* bias, void* out, int N, int H, int W,
                                         int Cin, int Cout, int relu) {
    if (!in || !wimg || !bias || !out || N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin % 32 != 0 || Cout % 64 != 0 ||
        (relu != 0 && relu != 1) || W > 16 * DC_MT)
        return PAM_E_ARG;
    if ((size_t)N * H * W * Cin * 2 >= (1ull << 31) || (size_t)N * 4 * H * W * Cout * 2 >= (1ull << 31) || Cout / 64 > 65535) return PAM_E_ARG;
    DeconvArgs a;
    a.in = (const uint16_t*)in; a.wimg = (const uint16_t*)wimg; a.bias = bias; a.out = (uint16_t*)out;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.relu = relu;
    a.TR = deconv_rows(H, W);
    a.row_tiles = (H + a.TR - 1) / a.TR;
    const int npatch = (a.TR + 2) * (W + 2);
    if (4 * npatch > 256 * DC_MAXP || (size_t)N * a.row_tiles >= (1ull << 31)) return PAM_E_ARG;
    const int lds = npatch * 64;
    if (!pam_max_dynamic_lds((const void*)k_deconv4x4s2, lds)) return PAM_E_HIP;
    pam_launch(k_deconv4x4s2, dim3(N * a.row_tiles, Cout / 64), dim3(256), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
