// libpam_hip.so, fused-block part for HRNet-W32: one BasicBlock of the 32-channel branch
//     out = ReLU( conv3x3( ReLU(conv3x3(x) + b1) ) + b2 + x )            (3x3, stride 1, pad 1, 32 -> 32 -> 32, BN folded)
// per work item with the weights of BOTH convolutions resident in LDS -- k_bblock2_48 (csrc/pam_block2.hip) at 32 channels.
//   * K = (tap, cin) = 9 x 32: exactly 9 k-steps of 32 per convolution, no zero tail.  A k-step's weight image is [32 rows][64 B]; a
//     convolution is 18 KB, both 36 KB, so the input tile has ~120 KB of LDS (75 KB at C = 48).  The tile is bounded by the M tiles a
//     wave keeps (6 for conv1, 5 for conv2, as at C = 48), not by LDS.
//   * activation slots are 64 B (32 bf16).  16 consecutive slots at a 64-byte pitch hit only 4 distinct 16-byte slots of a 256-byte bank
//     row (a 4-way conflict for ds_read_b128), so the four 16-byte pieces of slot s are stored swizzled: physical piece p holds logical
//     piece p ^ ((s >> 2) & 3).  Any 16 consecutive slots then cover all 16 (s % 4, piece) pairs: conflict-free at every tap offset.
//     The weight rows are swizzled the same way by their row index (physical piece p of row R holds logical piece p ^ ((R >> 2) & 3)).
//   * LDS = [X tile: (TR+4) x (TC+4) slots, rounded up to 1 KiB][bias 1 KB][W1 18 KB][W2 18 KB].  Bias, W1 and X arrive by LDS-DMA
//     before conv1; W2's 18 pieces are issued beside conv1's first k-steps.
//   * weight rows are permuted so that row j * 16 + q = output channel 8 (q >> 2) + 4 j + (q & 3): a lane's 8 accumulator channels are
//     8 g .. 8 g + 7 -- ONE 16-byte piece of a slot for the intermediate, the residual and the output.
// Same K order per output element as k_conv3x3<32> (bias first, then tap by tap, the tap's 32 input channels as one k-step): the block
// is bit-identical to the two launches of that kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_resident.hpp"

namespace {

// 64-byte slots, 9 k-step images of [32 rows][64 B], 6 / 5 M tiles per wave for conv1 / conv2, 37 DMA pieces of bias + weights (csrc/pam_resident.hpp)
constexpr int PA = Block32::PA, NST = Block32::NST, WIMG = Block32::WIMG, MW1 = Block32::MW1, MW2 = Block32::MW2, TST = Block32::TST, WPIECES = Block32::WPIECES;

struct BB32Args {
    const uint16_t* in; const char* wpack; uint16_t* out;
    int N, H, W, TR, TC, tiles_y, tiles_x, nitems, xbytes;
    float inv_pwx, inv_pwi;
};

__device__ __attribute__((aligned(64))) const uint32_t g_bb32_zero[16] = {0};

// byte offset of piece `logical` of slot s in a swizzled activation image
__device__ __forceinline__ unsigned slot_piece(int s, int logical) { return (unsigned)(s * PA + ((logical ^ ((s >> 2) & 3)) << 4)); }

__global__ __launch_bounds__(512) void k_bblock2_32(BB32Args a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = xcd_order(blockIdx.x, a.nitems);
    const int per_img = a.tiles_y * a.tiles_x;
    const int n = bx / per_img, trem = bx - n * per_img, tyi = trem / a.tiles_x, txi = trem - tyi * a.tiles_x;
    const int ty0 = tyi * a.TR, tx0 = txi * a.TC;
    const int PWx = a.TC + 4, PWi = a.TC + 2, XS = (a.TR + 4) * PWx;
    char* Xb = smem;
    char* Bs = smem + a.xbytes;                          // bias piece, then W1, W2: the packed image as it lies in global memory
    char* W1 = Bs + 1024;

    // ---- bias, W1 and the X tile by LDS-DMA (1 KiB = 16 slots per wave-instruction) --------------------------------------------
    const char* wsrc = a.wpack + lane * 16;
    auto wdma = [&](int p) { __builtin_amdgcn_global_load_lds((glb_void*)(wsrc + p * 1024), (lds_void*)(Bs + p * 1024), 16, 0, 0); };
    for (int p = wave; p < 1 + WIMG / 1024; p += 8) wdma(p);
    {
        // lane l of instruction k fills LDS bytes k KiB + 16 l: slot s = 16 k + l / 4, physical piece l & 3 = logical piece
        // (l & 3) ^ ((s >> 2) & 3) of the pixel at X row s / PWx, column s % PWx (zeros outside the image and past the tile)
        const char* img = (const char*)a.in + (size_t)n * a.H * a.W * PA;
        for (int k = wave; k * 1024 < a.xbytes; k += 8) {
            const int s = 16 * k + (lane >> 2);
            const int r = fdiv_small(s, a.inv_pwx), c = s - r * PWx;
            const int iy = ty0 - 2 + r, ix = tx0 - 2 + c;
            const bool ok = s < XS && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const int logical = (lane & 3) ^ ((s >> 2) & 3);
            const char* src = ok ? img + ((size_t)iy * a.W + ix) * PA + logical * 16 : (const char*)g_bb32_zero;
            __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(Xb + k * 1024), 16, 0, 0);
        }
    }

    // per-lane byte offsets of the 9 k-steps in an activation image of pitch PW slots, relative to the lane's slot in M tile 0 of its
    // wave; a wave's tiles lie 128 slots apart, so the swizzle of a tap's slot is the same in all of them
    const int b0 = wave * 16 + l15;
    auto mk_koff = [&](int PW, unsigned (&koff)[NST]) {
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int ky = st / 3, kx = st - 3 * ky, d = ky * PW + kx;
            koff[st] = slot_piece(b0 + d, g) - (unsigned)(b0 * PA);
        }
    };
    unsigned koff[NST];
    mk_koff(PWx, koff);
    const char* xl = Xb + b0 * PA;
    const char* wl = W1 + l15 * 64 + ((g ^ (l15 >> 2)) << 4);
    auto xaddr = [&](int i, int st) { return xl + koff[st] + i * TST; };
    const int nt1 = ((a.TR + 2) * PWx + 15) >> 4, nt2 = (a.TR * PWi + 15) >> 4;          // M tiles that carry real slots
    const int mt1 = (nt1 - wave + 7) >> 3, mt2 = (nt2 - wave + 7) >> 3;                    // ... of this wave (tile = wave + 8 i)

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // bias, W1 and X have landed (this wave's share) ...
    __syncthreads();                                     // ... and everybody's
    const float* bias = (const float*)Bs;

    f32x4 acc[MW1][2];
    // ---- conv1 -------------------------------------------------------------------------------------------------------------------
    {
        const f32x4 c0 = *(const f32x4*)(bias + 8 * g), c1 = *(const f32x4*)(bias + 8 * g + 4);
#pragma unroll
        for (int i = 0; i < MW1; ++i) { acc[i][0] = c0; acc[i][1] = c1; }
    }
    // W2 (18 pieces) is requested beside conv1's first three k-steps
    auto top1 = [&](int st) {
        if (st < 3) {
            const int p = 1 + WIMG / 1024 + wave + 8 * st;
            if (p < WPIECES) wdma(p);
        }
    };
    if (mt1 > 5) resident_pass<KStep32, 6>(acc, wl, xaddr, top1);
    else if (mt1 == 5) resident_pass<KStep32, 5>(acc, wl, xaddr, top1);
    else if (mt1 == 4) resident_pass<KStep32, 4>(acc, wl, xaddr, top1);
    else resident_pass<KStep32, 3>(acc, wl, xaddr, top1);

    // intermediate = ReLU(conv1 + b1) as bf16 on a grid of pitch PWi, zero where the position lies outside the image
    u32x4 mid[MW1];
    int maddr[MW1];
#pragma unroll
    for (int i = 0; i < MW1; ++i) {
        const int p = (wave + 8 * i) * 16 + l15;
        const int r1 = fdiv_small(p, a.inv_pwx), c1 = p - r1 * PWx;
        const int iy = ty0 - 1 + r1, ix = tx0 - 1 + c1;
        const bool ok = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        maddr[i] = (r1 < a.TR + 2 && c1 < a.TC + 2) ? (int)slot_piece(r1 * PWi + c1, g) : -1;
        const uint32_t keep = ok ? 0xffffffffu : 0u;
        mid[i] = (u32x4){relu_bf16x2(pack_bf16x2(acc[i][0][0], acc[i][0][1])) & keep, relu_bf16x2(pack_bf16x2(acc[i][0][2], acc[i][0][3])) & keep,
                         relu_bf16x2(pack_bf16x2(acc[i][1][0], acc[i][1][1])) & keep, relu_bf16x2(pack_bf16x2(acc[i][1][2], acc[i][1][3])) & keep};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's W2 pieces have landed
    __syncthreads();                                     // every wave is done reading X, and W2 is complete
#pragma unroll
    for (int i = 0; i < MW1; ++i)
        if (maddr[i] >= 0) *(u32x4*)(Xb + maddr[i]) = mid[i];
    __syncthreads();                                     // the intermediate is visible

    // ---- conv2 + epilogue ------------------------------------------------------------------------------------------------------------
    // residual = the block's input at this lane's output pixels (L2-hot), requested now, used after the K loop
    u32x4 rq[MW2];
    long ooff[MW2];
#pragma unroll
    for (int i = 0; i < MW2; ++i) {
        const int q = (wave + 8 * i) * 16 + l15;
        const int r2 = fdiv_small(q, a.inv_pwi), c2 = q - r2 * PWi;
        const int oy = ty0 + r2, ox = tx0 + c2;
        const bool ok = r2 < a.TR && c2 < a.TC && oy < a.H && ox < a.W;
        ooff[i] = ok ? (long)((((size_t)n * a.H + oy) * a.W + ox) * 32) : -1;
        rq[i] = *(const u32x4*)(a.in + (ok ? ooff[i] : 0) + 8 * g);
    }
    mk_koff(PWi, koff);
    {
        const f32x4 c0 = *(const f32x4*)(bias + 32 + 8 * g), c1 = *(const f32x4*)(bias + 32 + 8 * g + 4);
#pragma unroll
        for (int i = 0; i < MW2; ++i) { acc[i][0] = c0; acc[i][1] = c1; }
    }
    auto top2 = [](int) {};
    if (mt2 > 4) resident_pass<KStep32, 5>(acc, wl + WIMG, xaddr, top2);
    else if (mt2 == 4) resident_pass<KStep32, 4>(acc, wl + WIMG, xaddr, top2);
    else if (mt2 == 3) resident_pass<KStep32, 3>(acc, wl + WIMG, xaddr, top2);
    else resident_pass<KStep32, 2>(acc, wl + WIMG, xaddr, top2);
#pragma unroll
    for (int i = 0; i < MW2; ++i) {
        if (ooff[i] < 0) continue;
        uint32_t ov[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t lo = rq[i][2 * j], hi = rq[i][2 * j + 1];
            ov[2 * j] = relu_bf16x2(pack_bf16x2(acc[i][j][0] + bf16_lo(lo), acc[i][j][1] + bf16_hi(lo)));
            ov[2 * j + 1] = relu_bf16x2(pack_bf16x2(acc[i][j][2] + bf16_lo(hi), acc[i][j][3] + bf16_hi(hi)));
        }
        *(u32x4*)(a.out + ooff[i] + 8 * g) = (u32x4){ov[0], ov[1], ov[2], ov[3]};
    }
}

struct Launch32 : Block32 {
    using Args = BB32Args;
    static constexpr auto kernel = k_bblock2_32;
    static constexpr bool REACH = true;                  // the X tile has ~120 KB: a small tile's junk reads can pass W2's end
    static void diag(Args&) {}
};

}  // namespace

int pam_bb32_launch(void* stream, const void* in, const void* wpack, void* out, int N, int H, int W, int tile_rows, int tile_cols) {
    return resident_block_launch<Launch32>(stream, in, wpack, out, N, H, W, tile_rows, tile_cols);
}
