// Shared by the kernels whose weights stay RESIDENT in LDS while a wave walks K once over them: the fused BasicBlocks k_bblock2_48
// (csrc/pam_block2.hip) and k_bblock2_32 (csrc/pam_block32.hip) and the strided k_down48 (csrc/pam_down.hip).  Device side: the k-step
// images and the pass itself; host side: the cost model, the tile search and the launcher of the two blocks.
//
// The scheme.  A convolution's weights lie in LDS as one image per k-step of 32 K elements ([rows][64 B], 16 rows = 1 KiB per N tile),
// the activations as slots of one pixel's channels.  After the prologue nothing in LDS moves, so the K loop needs no barrier and no ring
// protocol: the eight waves of an item run free, two per SIMD, each one's fragment reads, waits and address arithmetic beside its
// partner's MFMAs.  A wave keeps MT x NTW accumulator tiles, reads the NTW + MT fragments of k-step st + 1 under the MT x NTW MFMAs of
// k-step st (fragments double-buffered in registers) and pins that issue order with spread<> and one sched_barrier per k-step.
#pragma once
#include "../../include/pam.h"
#include "pam_kernel.hpp"

// ---- k-step images ------------------------------------------------------------------------------------------------------------------
// PA: bytes of an activation slot; NST: k-steps per convolution; SUB: bytes of one k-step's weight image; WIMG: bytes per convolution.

// C = 48, K = (tap, cin) flattened: 432 = 13.5 x 32, the tail's weights are zero.  The format of one convolution of k_bblock2_48 and of
// one 48-channel slab of k_down48 (packing.kstep48_image): rows permuted so that a lane's 12 output channels are 8 g .. 8 g + 7 (N tiles
// 0, 1) and 32 + 4 g .. + 3 (N tile 2), the 16-byte pieces of a row swizzled by sigma = (0, 2, 3, 1)[(row % 16) >> 2].
struct KStep48 {
    static constexpr int PA = 96, NST = 14, SUB = 48 * 64, WIMG = NST * SUB;      // 43 008 B per convolution = 42 DMA pieces
    // the piece swizzle of the row a lane with l15 = lane & 15 reads: logical piece g lies at physical piece g ^ sigma (0x78 = sigma, 2 bits each)
    static __device__ __forceinline__ int sigma(int l15) { return (0x78 >> ((l15 >> 2) * 2)) & 3; }
    // a lane's 12 channels of one pixel (slot: the pixel's channel 0): one aligned 16-byte and one aligned 8-byte store
    static __device__ __forceinline__ void store12(uint16_t* slot, int g, const uint32_t (&v)[6]) {
        *(u32x4*)(slot + 8 * g) = (u32x4){v[0], v[1], v[2], v[3]};
        *(u32x2*)(slot + 32 + 4 * g) = (u32x2){v[4], v[5]};
    }
};

// C = 32, K = (tap, cin) = 9 x 32: one k-step per tap, no tail (csrc/pam_block32.hip has the row permutation and the swizzle)
struct KStep32 {
    static constexpr int PA = 64, NST = 9, SUB = 32 * 64, WIMG = NST * SUB;       // 18 432 B per convolution = 18 DMA pieces
};

// ---- the pass -----------------------------------------------------------------------------------------------------------------------
// One pass of a wave over weights resident in LDS: MT M tiles x NTW N tiles, K walked once in K::NST k-steps of 32; the fragments of
// k-step st + 1 are read under the MFMAs of k-step st.  wl: this lane's row of k-step 0 in the weight image (k-step images K::SUB bytes
// apart, N tile j at + j KiB); xaddr(i, st): address of the lane's 8-channel slice of k-step st for M tile i; top(st) runs ahead of
// k-step st's reads.  acc may hold more M tiles than the pass multiplies (a wave multiplies only those that carry real positions).
template <typename K, int MT, int NTW, int MTA, typename XAddr, typename Top>
__device__ __forceinline__ void resident_pass(f32x4 (&acc)[MTA][NTW], const char* wl, XAddr xaddr, Top top) {
    bf16x8 af[2][NTW], bf[2][MT];
    auto ld = [&](int st, bf16x8* a_, bf16x8* b_) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) a_[j] = *(const bf16x8*)(wl + st * K::SUB + j * 1024);
#ifdef PAM_KO_PIXREADS                                     // timing knock-out (wrong results): pixel fragments read every third k-step only
        if (st % 3 == 0)
#endif
#pragma unroll
        for (int i = 0; i < MT; ++i) b_[i] = *(const bf16x8*)xaddr(i, st);
    };
    ld(0, af[0], bf[0]);
#pragma unroll
    for (int st = 0; st < K::NST; ++st) {
        const int cur = st & 1, nxt = cur ^ 1;
        top(st);
        if (st + 1 < K::NST) ld(st + 1, af[nxt], bf[nxt]);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NTW; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[cur][j]), __builtin_bit_cast(bf16x8_t, bf[cur][i]), acc[i][j], 0, 0, 0);
        if constexpr (NTW * MT >= MT + NTW) spread<NTW * MT, MT + NTW>();      // one M tile: fewer MFMAs than reads, nothing to spread
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
constexpr int RESIDENT_LDS_MAX = 160 * 1024;

// Cost model: the M tiles of the busiest SIMD when a pass has nt M tiles (tile t -> wave t % 8 -> SIMD t % 4; a wave multiplies the
// instantiated count that holds its tiles, `lo` at least).
static inline int simd_tiles(int nt, int lo) {
    int worst = 0;
    for (int s = 0; s < 4; ++s) {
        int sum = 0;
        for (int w = s; w < 8; w += 4) { int m = nt > w ? (nt - w + 7) >> 3 : 0; sum += m < lo ? lo : m; }
        if (sum > worst) worst = sum;
    }
    return worst;
}

// A fused BasicBlock on k-step images K.  LDS = [X tile: (TR+4) x (TC+4) slots, rounded up to 1 KiB][bias 1 KiB][W1][W2]; a wave keeps
// MW1 M tiles (16 slots each) for conv1 and MW2 for conv2, its tiles TST bytes apart (tile = wave + 8 i).
template <typename K>
struct ResidentBlock : K {
    using Block = ResidentBlock;           // for what derives from it (one tile memo per block, not per derived type)
    static constexpr int MW1 = 6, MW2 = 5, TST = 8 * 16 * K::PA;
    static constexpr int WPIECES = 1 + 2 * K::WIMG / 1024;                          // bias piece + both weight images, in DMA pieces of 1 KiB
    static constexpr int XSLOTS_MAX = (RESIDENT_LDS_MAX - WPIECES * 1024) / K::PA;
    static bool fits(int tr, int tc) { return (tr + 2) * (tc + 4) <= 16 * 8 * MW1 && tr * (tc + 2) <= 16 * 8 * MW2 && (tr + 4) * (tc + 4) <= XSLOTS_MAX; }
};
using Block48 = ResidentBlock<KStep48>;    // 85 DMA pieces of bias + weights, 800 X slots
using Block32 = ResidentBlock<KStep32>;    // 37 DMA pieces; the X tile has ~120 KB, so the M tiles a wave keeps bound the tile, not LDS
static_assert(Block48::WPIECES == 85 && Block48::XSLOTS_MAX == 800 && Block32::WPIECES == 37 && Block32::XSLOTS_MAX == 1968, "LDS plan");

// Tile of block B for an N x H x W tensor: the (TR, TC) that minimises rounds of 256 workgroups x time of an item, ties -> fewer items.
// An item's time: a fixed prologue (the X tile and the first weights must land before the first MFMA: ~8 M tiles' worth) plus, per
// convolution, the M tiles of the busiest SIMD (3-6 instantiated for conv1, 2-5 for conv2).  The search is ~H x W steps, so every B
// keeps its last answer (the memo belongs to the instantiation: its key is B and (N, H, W), all the answer depends on).
template <typename B>
static bool resident_pick_tile(int N, int H, int W, int& TR, int& TC) {
    static thread_local int cN = 0, cH = 0, cW = 0, cTR = 0, cTC = 0;
    if (N == cN && H == cH && W == cW) { TR = cTR; TC = cTC; return true; }
    long best = -1;
    for (int tr = 1; tr <= H; ++tr)
        for (int tc = 1; tc <= W; ++tc) {
            if (!B::fits(tr, tc)) continue;
            const int s1 = (tr + 2) * (tc + 4), s2 = tr * (tc + 2);
            const long items = (long)N * ((H + tr - 1) / tr) * ((W + tc - 1) / tc);
            const long per = 8 + simd_tiles((s1 + 15) / 16, 3) + simd_tiles((s2 + 15) / 16, 2);
            const long cost = ((items + 255) / 256) * per * 4096 + items;
            if (best < 0 || cost < best) { best = cost; TR = tr; TC = tc; }
        }
    if (best < 0) return false;
    cN = N; cH = H; cW = W; cTR = TR; cTC = TC;
    return true;
}

// Launch of a fused block.  T = its ResidentBlock plus Args (the kernel's argument struct), kernel, REACH (whether the junk M tiles'
// reads can pass the end of the plan above) and diag(Args&) (the diagnostic build's extra arguments).
template <typename T>
static int resident_block_launch(void* stream, const void* in, const void* wpack, void* out, int N, int H, int W, int tile_rows, int tile_cols) {
    typename T::Args a;
    a.in = (const uint16_t*)in; a.wpack = (const char*)wpack; a.out = (uint16_t*)out;
    a.N = N; a.H = H; a.W = W;
    if (tile_rows > 0 && tile_cols > 0) { a.TR = tile_rows; a.TC = tile_cols; }
    else if (!resident_pick_tile<typename T::Block>(N, H, W, a.TR, a.TC)) return PAM_E_ARG;
    if (!T::fits(a.TR, a.TC)) return PAM_E_ARG;
    a.tiles_y = (H + a.TR - 1) / a.TR; a.tiles_x = (W + a.TC - 1) / a.TC;
    a.nitems = N * a.tiles_y * a.tiles_x;
    a.inv_pwx = 1.0f / (float)(a.TC + 4); a.inv_pwi = 1.0f / (float)(a.TC + 2);
    a.xbytes = ((a.TR + 4) * (a.TC + 4) * T::PA + 1023) / 1024 * 1024;
    size_t lds = (size_t)a.xbytes + (size_t)T::WPIECES * 1024;
    if constexpr (T::REACH) {
        // junk M tiles of conv1 read up to 2 rows + 2 slots past the wave's last tile (a wave multiplies 3 tiles at least): keep those
        // reads inside the allocation
        const int mt_max = ((((a.TR + 2) * (a.TC + 4) + 15) >> 4) + 7) >> 3;
        const size_t reach = (size_t)(16 * 8 * (mt_max < 3 ? 3 : mt_max) + 2 * (a.TC + 4) + 3) * T::PA;
        if (reach > lds) lds = reach;
        if (lds > (size_t)RESIDENT_LDS_MAX) return PAM_E_ARG;
    }
    if (!pam_max_dynamic_lds((const void*)T::kernel, RESIDENT_LDS_MAX)) return PAM_E_HIP;
    T::diag(a);
    pam_launch(T::kernel, dim3(a.nitems), dim3(512), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// C = 32 (HRNet-W32): k_bblock2_32 lives in csrc/pam_block32.hip, the blocks' entry points in csrc/pam_block2.hip
int pam_bb32_launch(void* stream, const void* in, const void* wpack, void* out, int N, int H, int W, int tile_rows, int tile_cols);
