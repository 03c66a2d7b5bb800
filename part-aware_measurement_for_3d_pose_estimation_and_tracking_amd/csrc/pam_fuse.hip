// libpam_hip.so, fuse-layer part of a1 (round 5): one output of an HR module's fuse layer in ONE launch
//     out_i = ReLU( x_i + sum_{j < i} down_ij + sum_{j > i} nearest_up_{2^(j-i)}( W_ij x_j + b_ij ) )
// (hrnet_model.py, HighResolutionModule; stands inside the absent HRNet backend behind /root/reference/src/ivclabpose.py:210).
// down_ij = the result of the strided-convolution chain from the finer branch j (already at out_i's resolution: a "plain" term);
// the coarser branches j > i enter through a 1x1 convolution at THEIR resolution, up-sampled by pixel replication.
//
// Until round 5 the 1x1 products were launches of their own (18 per forward on the generic gather kernel: 2 % of the MFMA roof, 12 % of
// the HBM roof, each on some branch's tail in front of the module's join) whose results went to HBM and came back into k_upsample_add.
// k_fuse_sum: MANY SMALL, INDEPENDENT workgroups of NT = C / 16 waves (3, 6 or 12); wave j owns the output-channel tile j and holds the
// 1x1 weights of ALL sources for it in REGISTERS (host-packed MFMA A fragments, one 16-byte global load per lane and fragment, statically
// indexed: 84 VGPRs for output 0 of a four-branch module, 48 for output 2).  A workgroup's unit is 16 pixels of an ANCHOR level L (a
// UA x UB rectangle of 2^L x 2^L output blocks): MFMA row r is anchor pixel r.  A source coarser than L multiplies the ancestor of each
// anchor pixel (duplicate rows are recomputed: that IS the pixel replication), a source finer than L has 4^(L - shift) M tiles whose row
// r is a child of anchor pixel r.  The source pixels go from global memory straight into MFMA B fragments; accumulators start from the
// bias, k-steps ascend, one bf16 rounding per product: exactly the arithmetic of the convolution launches they replace.  A lane then
// holds, for its four channels, every source's products under its anchor pixel, and the sum base + plain terms + products (ascending
// shift) -> ReLU -> out is k_upsample_add's.  The products go through a few KB of LDS behind one __syncthreads, and the workgroup covers
// its output rectangle 16 bytes per lane (a lane-by-lane walk of the pixels under the anchor pixel, 8 bytes per access and no LDS, lost
// by 1.3 - 3.3 us at 20 crops and was taken out).  No persistent walk, no specialised wave, no dependence between workgroups: the
// latencies hide behind the other workgroups of the CU.  Nothing but base, plain terms, sources, weights and out touches memory.
// Bit-identical to pam_conv2d_nhwc_bf16 (1x1) + pam_upsample_add_nhwc_bf16.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

namespace {

struct FSArgs {
    const uint16_t* base; uint16_t* out;
    const uint16_t* plain[2]; int plain_cs[2]; int nplain;
    const uint16_t* src[3]; const char* wimg[3]; const float* ubias[3];
    int N, H, W, relu;
    int ua_log, ub_log, units_y, units_x;    // a unit = 2^ua_log x 2^ub_log anchor pixels (16 of them), units_y x units_x units per image
};

// the weight fragments W[j][0 .. KS) of one source: lane-ordered 1 KiB images, 16 bytes per lane
template <int KS>
__device__ __forceinline__ void fs_weights(const char* wimg, int j, int lane, bf16x8 (&w)[KS]) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w[ks] = *(const bf16x8*)(wimg + ((size_t)(j * KS + ks) * 64 + lane) * 16);
}

// the pixels of ONE source under the lane's anchor pixel (ay, ax), straight into MFMA B fragments: x[t][ks] = the lane's 8 channels
// 32 ks + 8 g .. of the ancestor of the anchor pixel (a source at or above the anchor level: one M tile) or of its child t
template <int SH, int L, int KS, int NTL>
__device__ __forceinline__ void fs_pixels(const uint16_t* src, int n, int H, int W, int ay, int ax, int g, bf16x8 (&x)[NTL][KS]) {
    constexpr int Cs = KS * 32, D = SH < L ? L - SH : 0;
    static_assert(NTL == 1 << (2 * D), "M tiles of a source");
    const int Hs = H >> SH, Ws = W >> SH;
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
        int sy, sx;
        if constexpr (SH >= L) { sy = ay >> (SH - L); sx = ax >> (SH - L); }
        else { sy = (ay << D) + (t >> D); sx = (ax << D) + (t & ((1 << D) - 1)); }
        const uint16_t* xp = src + (((size_t)n * Hs + sy) * Ws + sx) * Cs + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) x[t][ks] = *(const bf16x8*)(xp + 32 * ks);
    }
}

// term[t] = bf16(W . x[t] + bias) for the lane's channels 16 j + 4 g .. + 3: accumulators start from the bias, k-steps ascend
template <int KS, int NTL>
__device__ __forceinline__ void fs_multiply(const bf16x8 (&w)[KS], const bf16x8 (&x)[NTL][KS], f32x4 b, u32x2 (&term)[NTL]) {
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
        f32x4 acc = b;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[ks]), __builtin_bit_cast(bf16x8_t, x[t][ks]), acc, 0, 0, 0);
        term[t] = (u32x2){pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3])};
    }
}

__device__ __forceinline__ f32x4 fs_bias(const float* bias, int c) {
    return bias ? (f32x4){bias[c], bias[c + 1], bias[c + 2], bias[c + 3]} : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
}

// M tile of a source of shift SH that holds the output pixel (dy, dx) of an anchor pixel's 2^L x 2^L block
template <int SH, int L>
__device__ __forceinline__ int fs_tile_of(int dy, int dx) {
    if constexpr (SH >= L) return 0;
    else return ((dy >> SH) << (L - SH)) | (dx >> SH);
}

// C: channels of the output; NUP sources of shifts SH0 < SH1 < SH2 with C << shift channels; L: anchor level (1 or 2, at most the
// coarsest shift); NPL plain terms
template <int C, int NUP, int SH0, int SH1, int SH2, int L, int NPL>
__global__ __launch_bounds__(C / 16 * 64, 2) void k_fuse_sum(FSArgs a) {
    constexpr int NT = C / 16, C8 = C / 8, NTHR = NT * 64;
    constexpr int KS0 = (C << SH0) / 32, KS1 = NUP > 1 ? (C << SH1) / 32 : 1, KS2 = NUP > 2 ? (C << SH2) / 32 : 1;
    constexpr int NTL0 = SH0 < L ? 1 << (2 * (L - SH0)) : 1, NTL1 = (NUP > 1 && SH1 < L) ? 1 << (2 * (L - SH1)) : 1, NTL2 = (NUP > 2 && SH2 < L) ? 1 << (2 * (L - SH2)) : 1;
    constexpr int BL = (1 << L) - 1;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, r = lane & 15;
    const int j = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per_img = a.units_y * a.units_x;
    int u = (int)blockIdx.x;
    const int n = u / per_img; u -= n * per_img;
    const int uy = u / a.units_x, ux = u - uy * a.units_x;
    // the lane's anchor pixel; a unit that hangs over the map's edge multiplies the edge pixel again there (the output pass skips it)
    const int HA = a.H >> L, WA = a.W >> L;
    const int ay0 = (uy << a.ua_log) + (r >> a.ub_log), ax0 = (ux << a.ub_log) + (r & ((1 << a.ub_log) - 1));
    const int ay = min(ay0, HA - 1), ax = min(ax0, WA - 1);

    // ---- everything the products need is requested in one go, with no branch in between (biases first: theirs is the only one), so
    // that a workgroup's life is two memory round trips and its stores: [base, plain terms,] weights, source pixels | products, sum
    const f32x4 b0 = fs_bias(a.ubias[0], 16 * j + 4 * g), b1 = NUP > 1 ? fs_bias(a.ubias[1], 16 * j + 4 * g) : b0, b2 = NUP > 2 ? fs_bias(a.ubias[2], 16 * j + 4 * g) : b0;
    bf16x8 w0[KS0], w1[KS1], w2[KS2];
    bf16x8 x0[NTL0][KS0], x1[NTL1][KS1], x2[NTL2][KS2];
    u32x2 t0[NTL0], t1[NTL1], t2[NTL2];
    auto products = [&]() {
        fs_weights<KS0>(a.wimg[0], j, lane, w0);
        if constexpr (NUP > 1) fs_weights<KS1>(a.wimg[1], j, lane, w1);
        if constexpr (NUP > 2) fs_weights<KS2>(a.wimg[2], j, lane, w2);
        fs_pixels<SH0, L, KS0, NTL0>(a.src[0], n, a.H, a.W, ay, ax, g, x0);
        if constexpr (NUP > 1) fs_pixels<SH1, L, KS1, NTL1>(a.src[1], n, a.H, a.W, ay, ax, g, x1);
        if constexpr (NUP > 2) fs_pixels<SH2, L, KS2, NTL2>(a.src[2], n, a.H, a.W, ay, ax, g, x2);
        __builtin_amdgcn_sched_barrier(0);               // the scheduler otherwise sinks every load to its MFMA: one round trip per k-step
        fs_multiply<KS0, NTL0>(w0, x0, b0, t0);
        if constexpr (NUP > 1) fs_multiply<KS1, NTL1>(w1, x1, b1, t1);
        if constexpr (NUP > 2) fs_multiply<KS2, NTL2>(w2, x2, b2, t2);
    };

    // ---- output pass: products -> LDS term tiles [source][M tile][anchor pixel][C]; then the workgroup covers its output rectangle
    // 16 bytes per lane: item e = (pixel of the rectangle, 8-channel group), 4^L / 2 items per thread, in batches of up to 8
    constexpr int NPT = NTL0 + (NUP > 1 ? NTL1 : 0) + (NUP > 2 ? NTL2 : 0);
    constexpr int NITEM = (16 << (2 * L)) * C8 / NTHR, B = NITEM < 8 ? NITEM : 8;
    static_assert(NITEM * NTHR == (16 << (2 * L)) * C8 && NPT * 16 * C * 2 <= 16 * 1024, "items per thread, LDS");
    __shared__ __attribute__((aligned(16))) uint16_t terms[NPT * 16 * C];
    const int ow_log = a.ub_log + L, oy0 = uy << (a.ua_log + L), ox0 = ux << ow_log;
    bf16x8 vb[B], vp[NPL ? NPL : 1][B];
    int po[B];                                         // pixel index in the output tensor, -1: outside the map
    int pl[B];                                         // (row in the rectangle << 16) | (column << 8) | 8-channel group
    auto request = [&](int b0) {
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const int e = tid + NTHR * (b0 + k);
            const int pix = e / C8, c8 = e - pix * C8;
            const int ry = pix >> ow_log, rx = pix & ((1 << ow_log) - 1);
            const bool ok = oy0 + ry < a.H && ox0 + rx < a.W;
            const long p = ((long)n * a.H + oy0 + ry) * a.W + ox0 + rx;
            po[k] = ok ? (int)p : -1; pl[k] = (ry << 16) | (rx << 8) | c8;
            const long pz = ok ? p : 0;
            vb[k] = *(const bf16x8*)(a.base + pz * C + c8 * 8);
#pragma unroll
            for (int t = 0; t < NPL; ++t) vp[t][k] = *(const bf16x8*)(a.plain[t] + pz * a.plain_cs[t] + c8 * 8);
        }
    };
    if constexpr (L == 1) request(0);
    products();
    if constexpr (L > 1) request(0);
    {
        uint16_t* tp = terms + r * C + 16 * j + 4 * g;
#pragma unroll
        for (int t = 0; t < NTL0; ++t) *(u32x2*)(tp + t * 16 * C) = t0[t];
        if constexpr (NUP > 1) {
#pragma unroll
            for (int t = 0; t < NTL1; ++t) *(u32x2*)(tp + (NTL0 + t) * 16 * C) = t1[t];
        }
        if constexpr (NUP > 2) {
#pragma unroll
            for (int t = 0; t < NTL2; ++t) *(u32x2*)(tp + (NTL0 + NTL1 + t) * 16 * C) = t2[t];
        }
    }
    __syncthreads();                                                             // the term tiles are complete: the only barrier
#pragma unroll
    for (int b0 = 0; b0 < NITEM; b0 += B) {
        if (b0) request(b0);
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const int ry = pl[k] >> 16, rx = (pl[k] >> 8) & 255, c8 = pl[k] & 255;
            const int ra = ((ry >> L) << a.ub_log) | (rx >> L), dy = ry & BL, dx = rx & BL;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = bf16_to_f32((uint16_t)vb[k][e]);
#pragma unroll
            for (int t = 0; t < NPL; ++t) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)vp[t][k][e]);
            }
            auto add = [&](int tile) {
                const bf16x8 q = *(const bf16x8*)(terms + (tile * 16 + ra) * C + c8 * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)q[e]);
            };
            add(fs_tile_of<SH0, L>(dy, dx));
            if constexpr (NUP > 1) add(NTL0 + fs_tile_of<SH1, L>(dy, dx));
            if constexpr (NUP > 2) add(NTL0 + NTL1 + fs_tile_of<SH2, L>(dy, dx));
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (short)f32_to_bf16(a.relu ? fmaxf(v[e], 0.0f) : v[e]);
            if (po[k] >= 0) *(bf16x8*)(a.out + (long)po[k] * C + c8 * 8) = o;
        }
    }
}

template <int C, int NUP, int SH0, int SH1, int SH2, int L>
int launch_fs(hipStream_t s, const FSArgs& a, unsigned grid) {
    const dim3 g(grid), b(C / 16 * 64);
    switch (a.nplain) {
        case 0: pam_launch(k_fuse_sum<C, NUP, SH0, SH1, SH2, L, 0>, g, b, 0, s, a); break;
        case 1: pam_launch(k_fuse_sum<C, NUP, SH0, SH1, SH2, L, 1>, g, b, 0, s, a); break;
        default: pam_launch(k_fuse_sum<C, NUP, SH0, SH1, SH2, L, 2>, g, b, 0, s, a); break;
    }
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// one (C, shifts): the anchor levels 1 .. min(2, the coarsest shift).  Level 3 is not built: 135 units at 20 crops leave half the CUs
// idle, and a lane-by-lane walk of its 64 pixels did not fit the registers of two waves per SIMD without scratch.
template <int C, int NUP, int SH0, int SH1, int SH2>
int dispatch_fs(hipStream_t s, const FSArgs& a, unsigned grid, int L) {
    constexpr int LMAX = NUP > 2 ? SH2 : (NUP > 1 ? SH1 : SH0);
    if (L == 1) return launch_fs<C, NUP, SH0, SH1, SH2, 1>(s, a, grid);
    if constexpr (LMAX >= 2)
        if (L == 2) return launch_fs<C, NUP, SH0, SH1, SH2, 2>(s, a, grid);
    return PAM_E_ARG;
}

// ---- the persistent form the sums had until DESIGN section 10s, kept for the shapes where it is still the faster one (see the entry
// point): one 576-thread workgroup per CU at most (eight worker waves + one loader wave), the 1x1 weights of all sources resident in
// LDS (64 - 147 KB), tiles of TA x TB pixels of the coarsest source walked by each workgroup, the next tile's source pixels arriving by
// LDS-DMA while this one's products run out of LDS into term tiles.  Same arithmetic, same results.
constexpr int FL_MAXI = 5;                 // 16-byte items of the output tile per thread at most

struct FLArgs {
    const uint16_t* base; uint16_t* out;
    const uint16_t* plain[2]; int plain_cs[2]; int nplain;
    const uint16_t* src[3]; const char* wimg[3]; const float* ubias[3]; int shift[3]; int src_c[3]; int nup;
    int N, H, W, relu, TA, TB, tiles_y, tiles_x, ntiles, OTH, OTW, smax;
    int w_off[3], w_bytes[3];               // LDS: the sources' weight images
    int bias_off;                           // float32 [nup][C]
    int src_off[3], src_bytes;              // a source-pixel buffer: [source][tile row][tile column][Cs]; two of them from src_base on
    int src_base, term_off[3];              // term tiles [source][pixel][C]
    float inv_otw;
};

template <int C>
__global__ __launch_bounds__(576) void k_fuse_sum_lds(FLArgs a) {
    constexpr int C8 = C / 8, NT = C / 16;
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per_img = a.tiles_y * a.tiles_x;

    // ---- once per launch: every source's weight fragments and biases -> LDS
    for (int s = 0; s < a.nup; ++s) {
        {
            const char* wsrc = a.wimg[s] + lane * 16;
            for (int p = wave; p * 1024 < a.w_bytes[s]; p += 9)
                __builtin_amdgcn_global_load_lds((glb_void*)(wsrc + p * 1024), (lds_void*)(smem + a.w_off[s] + p * 1024), 16, 0, 0);
            float* bs = (float*)(smem + a.bias_off) + s * C;
            if (tid < C) bs[tid] = a.ubias[s] ? a.ubias[s][tid] : 0.0f;            // C <= 192 < 512
        }
    }
    // source pixels under tile T -> buffer b, row by row (a tile row of a source is contiguous in the image), pieces of 1 KiB: all of them
    // by the LOADER wave (wave 8), which does nothing else -- the eight worker waves never wait for a DMA or for their own stores
    auto src_dma = [&](int T, int b) {
        const int n = T / per_img, trem = T - n * per_img, ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
        char* dst0 = smem + a.src_base + b * a.src_bytes;
        for (int s = 0; s < a.nup; ++s) {
            {
                const int sh = a.shift[s], d = a.smax - sh, th = a.TA << d, tw = a.TB << d, Cs = a.src_c[s];
                const int Hs = a.H >> sh, Ws = a.W >> sh, sy0 = (ty * a.TA) << d, sx0 = (tx * a.TB) << d;
                const int rowb = min(tw, Ws - sx0) * Cs * 2, pitch = tw * Cs * 2, npc = (rowb + 1023) >> 10;
                for (int r = 0; r < th && sy0 + r < Hs; ++r)
                    for (int k = 0; k < npc; ++k)
                        if (k * 1024 + lane * 16 < rowb)
                            __builtin_amdgcn_global_load_lds((glb_void*)((const char*)a.src[s] + ((((size_t)n * Hs + sy0 + r) * Ws + sx0) * Cs) * 2 + k * 1024 + lane * 16),
                                                             (lds_void*)(dst0 + a.src_off[s] + r * pitch + k * 1024), 16, 0, 0);
            }
        }
    };
    // the thread's items of a tile (the same positions in every tile): (tile row << 16) | (tile column << 8) | 8-channel group
    const int nitem = a.OTH * a.OTW * C8;
    int trc[FL_MAXI];
#pragma unroll
    for (int k = 0; k < FL_MAXI; ++k) {
        const int e = tid + 512 * k;
        const int pix = e / C8, c8 = e - pix * C8;
        const int r = fdiv_small(pix, a.inv_otw), c = pix - r * a.OTW;
        trc[k] = (tid < 512 && e < nitem) ? (r << 16) | (c << 8) | c8 : -1;
    }
    // jobs of a tile = (source, 16-pixel tile, 16-channel tile), coarsest (deepest K) source first; wave w takes jobs w, w + 8, ...
    int job0[4];
    {
        int acc_j = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            job0[q] = acc_j;
            if (q < a.nup) {
                const int d = a.smax - a.shift[a.nup - 1 - q];
                acc_j += ((((a.TA << d) * (a.TB << d)) + 15) >> 4) * NT;
            }
        }
        job0[3] = acc_j;
    }

    int T = (int)blockIdx.x;
    if (wave == 8) {
        // ---- loader: tile t + 1's source pixels go into the other buffer while the workers are on tile t (its last readers, the
        // products of tile t - 1, finished before the barrier at the top of tile t)
        if (T < a.ntiles) src_dma(T, 0);
        for (int it = 0; T < a.ntiles; T += (int)gridDim.x, ++it) {
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");             // top: tile t's pixels (and, first, my share of the weights) have landed
            if (T + (int)gridDim.x < a.ntiles) src_dma(T + (int)gridDim.x, (it + 1) & 1);
            asm volatile("s_barrier" ::: "memory");                                      // mid
        }
        return;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                    // my share of the weights has landed
    for (int it = 0; T < a.ntiles; T += (int)gridDim.x, ++it) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                 // top: this tile's source pixels are in LDS; the term tiles are free
        const int n = T / per_img, trem = T - n * per_img, ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
        const int oy0 = ty * a.OTH, ox0 = tx * a.OTW;
        // ---- base and plain terms of the thread's items: requested now, summed behind the products
        bf16x8 vb[FL_MAXI], vp[2][FL_MAXI];
        int eo[FL_MAXI];                                  // pixel index of the item in the output tensor (-1: none); the host checks N H W < 2^31
#pragma unroll
        for (int k = 0; k < FL_MAXI; ++k) {
            const int r = trc[k] >> 16, c = (trc[k] >> 8) & 255;
            const int oy = oy0 + r, ox = ox0 + c;
            const bool ok = trc[k] >= 0 && oy < a.H && ox < a.W;
            const int p = (n * a.H + oy) * a.W + ox;
            eo[k] = ok ? p : -1;
            const long pz = ok ? p : 0;
            const int c8 = ok ? trc[k] & 255 : 0;
            vb[k] = *(const bf16x8*)(a.base + pz * C + c8 * 8);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                vp[t][k] = t < a.nplain ? *(const bf16x8*)(a.plain[t] + pz * a.plain_cs[t] + c8 * 8) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
        // ---- the 1x1 products of the source pixels under the tile, out of LDS -> term tiles
        const char* sbuf = smem + a.src_base + (it & 1) * a.src_bytes;
        for (int job = wave; job < job0[3]; job += 8) {
            const int q = job >= job0[2] ? 2 : (job >= job0[1] ? 1 : 0);
            const int s = a.nup - 1 - q, jj = job - job0[q];
            const int mt = jj / NT, j = jj - mt * NT;
            const int d = a.smax - a.shift[s], npx = (a.TA << d) * (a.TB << d);
            const int Cs = a.src_c[s], KS = Cs >> 5;
            const int p = mt * 16 + l15, pq = min(p, npx - 1);
            const char* xp = sbuf + a.src_off[s] + pq * Cs * 2 + g * 16;
            const char* wp = smem + a.w_off[s] + (j * KS * 64 + lane) * 16;
            f32x4 acc = *(const f32x4*)(smem + a.bias_off + (s * C + 16 * j + 4 * g) * 4);
            for (int k0 = 0; k0 < KS; k0 += 3) {                                          // three k-steps' fragments read together, then multiplied
                bf16x8 fa[3], fb[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int ks = min(k0 + u, KS - 1);
                    fa[u] = *(const bf16x8*)(wp + ks * 1024); fb[u] = *(const bf16x8*)(xp + ks * 64);
                }
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (k0 + u < KS)
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[u]), __builtin_bit_cast(bf16x8_t, fb[u]), acc, 0, 0, 0);
            }
            if (p < npx)
                *(u32x2*)(smem + a.term_off[s] + (p * C + 16 * j + 4 * g) * 2) = (u32x2){pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3])};
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                    // the term tiles are complete

        // ---- out = [ReLU](base + plain terms + replicated products), k_upsample_add's order: base, then the terms in branch order
#pragma unroll
        for (int k = 0; k < FL_MAXI; ++k) {
            if (eo[k] < 0) continue;
            const int r = trc[k] >> 16, c = (trc[k] >> 8) & 255, c8 = trc[k] & 255;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = bf16_to_f32((uint16_t)vb[k][e]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (t < a.nplain) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)vp[t][k][e]);
                }
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (s < a.nup) {
                    const int sh = a.shift[s], tw = a.TB << (a.smax - sh);
                    const bf16x8 q = *(const bf16x8*)(smem + a.term_off[s] + (((r >> sh) * tw + (c >> sh)) * C + c8 * 8) * 2);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)q[e]);
                }
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (short)f32_to_bf16(a.relu ? fmaxf(v[e], 0.0f) : v[e]);
            *(bf16x8*)(a.out + (long)eo[k] * C + c8 * 8) = o;
        }
    }
}

template <int C>
int launch_fl(hipStream_t s, const FLArgs& a, size_t lds, int grid) {
    if (!pam_max_dynamic_lds((const void*)k_fuse_sum_lds<C>, 160 * 1024)) return PAM_E_HIP;
    pam_launch(k_fuse_sum_lds<C>, dim3(grid), dim3(576), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// the persistent form's host side: LDS plan, tile choice (tile_a x tile_b pixels of the coarsest source, <= 0: the largest that fits),
// at most max_workgroups workgroups when that is > 0
int fuse_sum_lds(void* stream, const void* base, int n_plain, const void* const* plain, const int32_t* plain_cstrides,
                  int n_up, const void* const* up_src, const int32_t* up_shifts, const int32_t* up_channels,
                  const void* const* up_wimg, const float* const* up_bias, void* out, int N, int H, int W, int C,
                  int relu, int tile_a, int tile_b, int max_workgroups) {
    if (!base || !out || N < 1 || H < 1 || W < 1 || (C != 48 && C != 96 && C != 192) || n_plain < 0 || n_plain > 2 || n_up < 1 || n_up > 3) return PAM_E_ARG;
    if ((size_t)N * H * W >= (1ull << 31)) return PAM_E_ARG;
    FLArgs a;
    a.base = (const uint16_t*)base; a.out = (uint16_t*)out; a.nplain = n_plain; a.nup = n_up;
    for (int t = 0; t < 2; ++t) {
        a.plain[t] = t < n_plain ? (const uint16_t*)plain[t] : nullptr;
        a.plain_cs[t] = (t < n_plain && plain_cstrides && plain_cstrides[t] > 0) ? plain_cstrides[t] : C;
        if (t < n_plain && (!a.plain[t] || a.plain_cs[t] < C || a.plain_cs[t] % 8 != 0)) return PAM_E_ARG;
    }
    int prev = 0;
    for (int s = 0; s < 3; ++s) {
        const bool on = s < n_up;
        a.src[s] = on ? (const uint16_t*)up_src[s] : nullptr; a.wimg[s] = on ? (const char*)up_wimg[s] : nullptr;
        a.ubias[s] = (on && up_bias) ? up_bias[s] : nullptr; a.shift[s] = on ? up_shifts[s] : 0; a.src_c[s] = on ? up_channels[s] : 0;
        a.w_off[s] = a.w_bytes[s] = a.src_off[s] = a.term_off[s] = 0;
        if (!on) continue;
        // sources in ascending shift (= branch) order; the map must be a whole number of source pixels (PyTorch's up-sampling needs that too)
        if (!a.src[s] || !a.wimg[s] || a.shift[s] <= prev || a.shift[s] > 5 || a.src_c[s] < 32 || a.src_c[s] % 32 != 0) return PAM_E_ARG;
        if (H % (1 << a.shift[s]) != 0 || W % (1 << a.shift[s]) != 0) return PAM_E_ARG;
        prev = a.shift[s];
    }
    a.smax = a.shift[n_up - 1];
    a.N = N; a.H = H; a.W = W; a.relu = relu ? 1 : 0;
    // LDS plan for a tile of TA x TB pixels of the coarsest source; false = does not fit
    const int c8 = C / 8;
    size_t lds = 0;
    auto plan = [&](int TA, int TB) {
        if ((long)(TA << a.smax) * (TB << a.smax) * c8 > 512L * FL_MAXI || (TA << a.smax) > 32767 || (TB << a.smax) > 255) return false;
        size_t o = 0;
        for (int s = 0; s < n_up; ++s) { a.w_off[s] = (int)o; a.w_bytes[s] = C * a.src_c[s] * 2; o += (size_t)a.w_bytes[s]; }
        a.bias_off = (int)o; o += (size_t)n_up * C * 4; o = (o + 1023) / 1024 * 1024;
        size_t sb = 0;
        for (int s = 0; s < n_up; ++s) { const int d = a.smax - a.shift[s]; a.src_off[s] = (int)sb; sb += (size_t)(TA << d) * (TB << d) * a.src_c[s] * 2; sb = (sb + 1023) / 1024 * 1024; }
        a.src_bytes = (int)sb; a.src_base = (int)o; o += 2 * sb;
        for (int s = 0; s < n_up; ++s) { const int d = a.smax - a.shift[s]; a.term_off[s] = (int)o; o += (size_t)(TA << d) * (TB << d) * C * 2; o = (o + 15) / 16 * 16; }
        lds = o;
        return o <= 160 * 1024;
    };
    int TA = tile_a, TB = tile_b;
    if (TA <= 0 || TB <= 0) {
        // the largest candidate that fits (FL_MAXI items per thread, LDS) and divides the coarsest map: an iteration costs two barriers and a
        // round of latencies whatever its size; a 16 x 24 tile of output 0 is 2 304 items
        const int Hc = H >> a.smax, Wc = W >> a.smax;
        const int cand[8][2] = {{8, 12}, {4, 6}, {4, 3}, {2, 3}, {1, 3}, {1, 2}, {1, 1}, {0, 0}};
        TA = 0;
        for (int pass = 0; pass < 2 && TA == 0; ++pass)
            for (int k = 0; cand[k][0] && TA == 0; ++k)
                if ((pass == 1 || (Hc % cand[k][0] == 0 && Wc % cand[k][1] == 0)) && plan(cand[k][0], cand[k][1])) { TA = cand[k][0]; TB = cand[k][1]; }
        if (TA == 0) return PAM_E_ARG;
    }
    if (!plan(TA, TB)) return PAM_E_ARG;
    a.TA = TA; a.TB = TB; a.OTH = TA << a.smax; a.OTW = TB << a.smax;
    a.tiles_y = (H + a.OTH - 1) / a.OTH; a.tiles_x = (W + a.OTW - 1) / a.OTW;
    const long long nt = (long long)N * a.tiles_y * a.tiles_x;
    if (nt >= (1ll << 30)) return PAM_E_ARG;
    a.ntiles = (int)nt;
    a.inv_otw = 1.0f / (float)a.OTW;
    const int ncu = pam_cu_count();
    // every workgroup walks the same number of tiles: 360 tiles -> 180 workgroups x 2 (not 256 of which 104 walk two); the CUs left over
    // take the other outputs' sums, which run on the branch streams at the same time
    int grid = max_workgroups > 0 && max_workgroups < ncu ? max_workgroups : ncu;
    const int per_wg = (a.ntiles + grid - 1) / grid;
    grid = (a.ntiles + per_wg - 1) / per_wg;
    switch (C) {
        case 48: return launch_fl<48>((hipStream_t)stream, a, lds, grid);
        case 96: return launch_fl<96>((hipStream_t)stream, a, lds, grid);
        default: return launch_fl<192>((hipStream_t)stream, a, lds, grid);
    }
}

}  // namespace

// up_wimg[s]: the 1x1 weights W (C x src_channels[s]) as MFMA A fragments, bf16 [C / 16][src_channels / 32][64 lanes][8]: lane l of fragment
// (j, ks) holds W[16 j + (l & 15)][32 ks + 8 (l >> 4) .. + 7].
// tile_a > 0: the anchor level L of the register-weights kernel (clamped to 1 .. min(2, the coarsest shift)); <= 0: the library's choice
// of level and kernel.  tile_b is not used.  max_workgroups caps the persistent kernel where the library takes it, and nothing else.
extern "C" int pam_fuse_sum_nhwc_bf16(void* stream, const void* base, int n_plain, const void* const* plain, const int32_t* plain_cstrides,
                                      int n_up, const void* const* up_src, const int32_t* up_shifts, const int32_t* up_channels,
                                      const void* const* up_wimg, const float* const* up_bias, void* out, int N, int H, int W, int C,
                                      int relu, int tile_a, int tile_b, int max_workgroups) {
    if (!base || !out || N < 1 || H < 1 || W < 1 || (C != 48 && C != 96 && C != 192) || n_plain < 0 || n_plain > 2 || n_up < 1 || n_up > 3) return PAM_E_ARG;
    if ((size_t)N * H * W >= (1ull << 31)) return PAM_E_ARG;
    FSArgs a;
    a.base = (const uint16_t*)base; a.out = (uint16_t*)out; a.nplain = n_plain;
    for (int t = 0; t < 2; ++t) {
        a.plain[t] = t < n_plain ? (const uint16_t*)plain[t] : nullptr;
        a.plain_cs[t] = (t < n_plain && plain_cstrides && plain_cstrides[t] > 0) ? plain_cstrides[t] : C;
        if (t < n_plain && (!a.plain[t] || a.plain_cs[t] < C || a.plain_cs[t] % 8 != 0)) return PAM_E_ARG;
    }
    int prev = 0, key = 0, ksteps = 0;
    for (int s = 0; s < 3; ++s) {
        const bool on = s < n_up;
        a.src[s] = on ? (const uint16_t*)up_src[s] : nullptr; a.wimg[s] = on ? (const char*)up_wimg[s] : nullptr;
        a.ubias[s] = (on && up_bias) ? up_bias[s] : nullptr;
        if (!on) continue;
        const int sh = up_shifts[s], cs = up_channels[s];
        // sources in ascending shift (= branch) order; the map must be a whole number of source pixels (PyTorch's up-sampling needs that too)
        if (!a.src[s] || !a.wimg[s] || sh <= prev || sh > 5 || cs < 32 || cs % 32 != 0) return PAM_E_ARG;
        if (H % (1 << sh) != 0 || W % (1 << sh) != 0) return PAM_E_ARG;
        // the k loops are unrolled per (C, source channels): a source of shift s has C << s channels, as in every HRNet
        if (cs != C << sh) return PAM_E_ARG;
        prev = sh; key = key * 8 + sh; ksteps += cs / 32;
    }
    const int smax = prev;
    a.N = N; a.H = H; a.W = W; a.relu = relu ? 1 : 0;
    // the unit's rectangle of 16 anchor pixels at level L: the shape that covers the anchor map with the fewest units (ties: the squarest)
    auto plan = [&](int L) {
        const int HA = H >> L, WA = W >> L;
        const int shapes[5][2] = {{2, 2}, {1, 3}, {3, 1}, {0, 4}, {4, 0}};
        long long best = -1;
        for (int k = 0; k < 5; ++k) {
            const int uy = (HA + (1 << shapes[k][0]) - 1) >> shapes[k][0], ux = (WA + (1 << shapes[k][1]) - 1) >> shapes[k][1];
            if (best < 0 || (long long)uy * ux < best) { best = (long long)uy * ux; a.ua_log = shapes[k][0]; a.ub_log = shapes[k][1]; a.units_y = uy; a.units_x = ux; }
        }
        return best;
    };
    // Which kernel (stand-alone times at 2 / 20 / 40 crops): the persistent LDS-weights form stays where it was not
    // beaten.  C = 192 (12-wave workgroups, one per CU at a time): 18 units 8.2 us against its 7.7, 180 units 8.9 against 11.9, 360 units
    // 16.9 against 16.8 -> register weights only for more than 64 units and no more than one per CU.  C = 96 under two sources: 540 units
    // (level 1) 13.3 us against 14.3, 1 080 units 25.0 against 20.2 -> register weights up to 768 units.  The thresholds lie between the
    // measured points; a caller that names a level (tile_a > 0) gets the register-weights kernel at any size.
    if (tile_a <= 0) {
        const long long u1 = (long long)N * plan(1);
        if ((C == 192 && (u1 <= 64 || u1 > pam_cu_count())) || (C == 96 && n_up == 2 && u1 > 768))
            return fuse_sum_lds(stream, base, n_plain, plain, plain_cstrides, n_up, up_src, up_shifts, up_channels, up_wimg, up_bias, out, N, H, W, C,
                                relu, 0, 0, max_workgroups);
    }
    // the anchor level unless the caller names it: level 2 reads a wave's weights and the coarse sources' pixels a quarter as often, which
    // pays from 18 k-steps of weights on (72 VGPRs) and only while there are units for half the CUs (level 1 below that: 4 times the
    // workgroups)
    int L = tile_a > 0 ? tile_a : ((smax >= 2 && ksteps >= 18 && (long long)N * plan(2) >= 128) ? 2 : 1);
    L = L > smax ? smax : L; L = L > 2 ? 2 : L;
    const long long best = plan(L);
    const long long nu = (long long)N * best;
    if (nu >= (1ll << 31)) return PAM_E_ARG;
    const unsigned grid = (unsigned)nu;
    hipStream_t st = (hipStream_t)stream;
    switch (C * 1000 + key) {                    // key: the shifts as octal digits
        case 48 * 1000 + 01: return dispatch_fs<48, 1, 1, 0, 0>(st, a, grid, L);
        case 48 * 1000 + 012: return dispatch_fs<48, 2, 1, 2, 0>(st, a, grid, L);
        case 48 * 1000 + 0123: return dispatch_fs<48, 3, 1, 2, 3>(st, a, grid, L);
        case 96 * 1000 + 01: return dispatch_fs<96, 1, 1, 0, 0>(st, a, grid, L);
        case 96 * 1000 + 012: return dispatch_fs<96, 2, 1, 2, 0>(st, a, grid, L);
        case 96 * 1000 + 02: return dispatch_fs<96, 1, 2, 0, 0>(st, a, grid, L);
        case 192 * 1000 + 01: return dispatch_fs<192, 1, 1, 0, 0>(st, a, grid, L);
        default: return PAM_E_ARG;               // a combination no network here uses: not instantiated
    }
}
