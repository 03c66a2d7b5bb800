// libpam_hip.so, fuse-layer part of a1 (round 5): one output of an HR module's fuse layer in ONE launch
//     out_i = ReLU( x_i + sum_{j < i} down_ij + sum_{j > i} nearest_up_{2^(j-i)}( W_ij x_j + b_ij ) )
// (hrnet_model.py, HighResolutionModule; stands inside the absent HRNet backend behind /root/reference/src/ivclabpose.py:210).
// down_ij = the result of the strided-convolution chain from the finer branch j (already at out_i's resolution: a "plain" term);
// the coarser branches j > i enter through a 1x1 convolution at THEIR resolution, up-sampled by pixel replication.
//
// ONE FRONT, TWO KERNELS.  The entry point at the end of the file checks the pointers, asks fuse_plan() (pam_fuse_plan.hpp: the argument
// check, the table FUSE_COMBOS of instantiated (C, shifts), which kernel, level, units or tiles, grid, LDS layout -- every shape rule, as
// pure integer arithmetic that pam_fuse_sum_plan and a test without a GPU ask too), fills the chosen kernel's argument struct from the
// plan and launches: k_fuse_sum (register weights, below) or, for the sizes where it was not beaten, the earlier k_fuse_sum_lds
// (persistent, weights in LDS; further down).  Both compute the sum of sum8_start / sum8_add / sum8_finish (pam_kernel.hpp), which is
// k_upsample_add's: bit-identical to pam_conv2d_nhwc_bf16 (1x1) + pam_upsample_add_nhwc_bf16.
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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"
#include "pam_fuse_plan.hpp"

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
            sum8_start(v, vb[k]);
#pragma unroll
            for (int t = 0; t < NPL; ++t) sum8_add(v, vp[t][k]);
            auto add = [&](int tile) { sum8_add(v, *(const bf16x8*)(terms + (tile * 16 + ra) * C + c8 * 8)); };
            add(fs_tile_of<SH0, L>(dy, dx));
            if constexpr (NUP > 1) add(NTL0 + fs_tile_of<SH1, L>(dy, dx));
            if constexpr (NUP > 2) add(NTL0 + NTL1 + fs_tile_of<SH2, L>(dy, dx));
            bf16x8 o;
            sum8_finish(v, a.relu, o);
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

// row I of FUSE_COMBOS: the anchor levels 1 .. min(2, the coarsest shift).  Level 3 is not built: 135 units at 20 crops leave half the
// CUs idle, and a lane-by-lane walk of its 64 pixels did not fit the registers of two waves per SIMD without scratch.
template <int I>
int dispatch_fs(hipStream_t s, const FSArgs& a, unsigned grid, int L) {
    constexpr FuseCombo K = FUSE_COMBOS[I];
    if (L == 1) return launch_fs<K.C, K.n_up, K.sh[0], K.sh[1], K.sh[2], 1>(s, a, grid);
    if constexpr (K.sh[K.n_up - 1] >= 2)
        if (L == 2) return launch_fs<K.C, K.n_up, K.sh[0], K.sh[1], K.sh[2], 2>(s, a, grid);
    return PAM_E_ARG;
}
// every row of the table is instantiated, and nothing else
template <int... I>
int dispatch_fs(std::integer_sequence<int, I...>, int combo, hipStream_t s, const FSArgs& a, unsigned grid, int L) {
    int rc = PAM_E_ARG;
    ((combo == I ? (void)(rc = dispatch_fs<I>(s, a, grid, L)) : (void)0), ...);
    return rc;
}

// ---- the persistent form the sums had until DESIGN section 10s, kept for the shapes where it is still the faster one (fuse_takes_lds
// in pam_fuse_plan.hpp): one 576-thread workgroup per CU at most (eight worker waves + one loader wave), the 1x1 weights of all sources resident in
// LDS (64 - 147 KB), tiles of TA x TB pixels of the coarsest source walked by each workgroup, the next tile's source pixels arriving by
// LDS-DMA while this one's products run out of LDS into term tiles.  Same arithmetic, same results.
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

        // ---- out = [ReLU](base + plain terms + replicated products), k_upsample_add's order: base, then the terms in branch order.
        // The arithmetic of sum8_start / sum8_add / sum8_finish (pam_kernel.hpp) written out: with the helpers this kernel compiles to
        // other code (134 -> 168 VGPRs and three spilled registers), so it keeps its text, and the bit-for-bit tests hold it to them
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
    if (!pam_max_dynamic_lds((const void*)k_fuse_sum_lds<C>, FL_LDS_MAX)) return PAM_E_HIP;
    pam_launch(k_fuse_sum_lds<C>, dim3(grid), dim3(576), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// what FSArgs and FLArgs have in common.  The caller has checked every pointer the counts name.
template <typename A>
void fuse_fill(A& a, const FuseQuery& q, const void* base, const void* const* plain, const void* const* up_src, const void* const* up_wimg,
               const float* const* up_bias, void* out, int relu) {
    a.base = (const uint16_t*)base; a.out = (uint16_t*)out; a.nplain = q.n_plain;
    for (int t = 0; t < 2; ++t) {
        a.plain[t] = t < q.n_plain ? (const uint16_t*)plain[t] : nullptr;
        a.plain_cs[t] = (t < q.n_plain && q.plain_cs[t] > 0) ? q.plain_cs[t] : q.C;
    }
    for (int s = 0; s < 3; ++s) {
        const bool on = s < q.n_up;
        a.src[s] = on ? (const uint16_t*)up_src[s] : nullptr; a.wimg[s] = on ? (const char*)up_wimg[s] : nullptr;
        a.ubias[s] = (on && up_bias) ? up_bias[s] : nullptr;
    }
    a.N = q.N; a.H = q.H; a.W = q.W; a.relu = relu ? 1 : 0;
}

}  // namespace

// Which kernel, level, units or tiles, grid and dynamic LDS bytes pam_fuse_sum_nhwc_bf16 would launch with: fuse_plan() asked without a
// launch (include/pam.h).  n_cu <= 0: the current device's compute units.
extern "C" int pam_fuse_sum_plan(int N, int H, int W, int C, int n_plain, int n_up, const int32_t* up_shifts, const int32_t* up_channels,
                                 int tile_a, int tile_b, int max_workgroups, int n_cu, int32_t* out8) {
    if (!out8 || (n_up > 0 && (!up_shifts || !up_channels))) return PAM_E_ARG;
    const FusePlan p = fuse_plan(fuse_query(N, H, W, C, n_plain, nullptr, n_up, up_shifts, up_channels, tile_a, tile_b, max_workgroups,
                                            n_cu > 0 ? n_cu : pam_cu_count()));
    if (p.rc == PAM_OK) fuse_plan_out8(p, out8);
    return p.rc;
}

// up_wimg[s]: the 1x1 weights W (C x src_channels[s]) as MFMA A fragments, bf16 [C / 16][src_channels / 32][64 lanes][8]: lane l of fragment
// (j, ks) holds W[16 j + (l & 15)][32 ks + 8 (l >> 4) .. + 7].
// tile_a > 0: the anchor level L of the register-weights kernel (clamped to 1 .. min(2, the coarsest shift)); <= 0: the library's choice
// of level and kernel.  tile_b is not used.  max_workgroups caps the persistent kernel where the library takes it, and nothing else.
extern "C" int pam_fuse_sum_nhwc_bf16(void* stream, const void* base, int n_plain, const void* const* plain, const int32_t* plain_cstrides,
                                      int n_up, const void* const* up_src, const int32_t* up_shifts, const int32_t* up_channels,
                                      const void* const* up_wimg, const float* const* up_bias, void* out, int N, int H, int W, int C,
                                      int relu, int tile_a, int tile_b, int max_workgroups) {
    if (!base || !out || (n_up > 0 && (!up_src || !up_shifts || !up_channels || !up_wimg))) return PAM_E_ARG;
    for (int t = 0; t < n_plain && t < 2; ++t) if (!plain || !plain[t]) return PAM_E_ARG;
    for (int s = 0; s < n_up && s < 3; ++s) if (!up_src[s] || !up_wimg[s]) return PAM_E_ARG;
    const FuseQuery q = fuse_query(N, H, W, C, n_plain, plain_cstrides, n_up, up_shifts, up_channels, tile_a, tile_b, max_workgroups, pam_cu_count());
    const FusePlan p = fuse_plan(q);
    if (p.rc != PAM_OK) return p.rc;
    if (p.kernel == 1) {
        FSArgs a;
        fuse_fill(a, q, base, plain, up_src, up_wimg, up_bias, out, relu);
        a.ua_log = p.ua_log; a.ub_log = p.ub_log; a.units_y = p.units_y; a.units_x = p.units_x;
        return dispatch_fs(std::make_integer_sequence<int, FUSE_NCOMBO>{}, p.combo, (hipStream_t)stream, a, p.grid, p.L);
    }
    FLArgs a;
    fuse_fill(a, q, base, plain, up_src, up_wimg, up_bias, out, relu);
    a.nup = q.n_up; a.smax = q.shift[q.n_up - 1];
    for (int s = 0; s < 3; ++s) {                // (the entries behind n_up are 0 in the query and in the plan)
        a.shift[s] = q.shift[s]; a.src_c[s] = q.src_c[s];
        a.w_off[s] = p.w_off[s]; a.w_bytes[s] = p.w_bytes[s]; a.src_off[s] = p.src_off[s]; a.term_off[s] = p.term_off[s];
    }
    a.bias_off = p.bias_off; a.src_bytes = p.src_bytes; a.src_base = p.src_base;
    a.TA = p.TA; a.TB = p.TB; a.OTH = p.TA << a.smax; a.OTW = p.TB << a.smax;
    a.tiles_y = p.tiles_y; a.tiles_x = p.tiles_x; a.ntiles = p.ntiles;
    a.inv_otw = 1.0f / (float)a.OTW;
    switch (q.C) {                               // fuse_lds_rows_are_96_192 (pam_fuse_plan.hpp): no other C is planned for this kernel
        case 96: return launch_fl<96>((hipStream_t)stream, a, (size_t)p.lds_bytes, (int)p.grid);
        case 192: return launch_fl<192>((hipStream_t)stream, a, (size_t)p.lds_bytes, (int)p.grid);
        default: return PAM_E_ARG;
    }
}
