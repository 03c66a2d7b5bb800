// libpam_hip.so, conv stack
// ====================================================================================================================
// k_conv3x3s: the same convolution (Cin = 192 / 384, activation codes 0 / 1) with SPECIALISED waves.  In k_conv3x3 at 20 crops a
// workgroup is alone on its CU, so every wave pays for its own operand traffic in its own instruction stream: the burst of
// buffer_loads for the next chunk holds the MFMA stream for ~1.6 k cycles per chunk, the register -> LDS pass for another ~1 k, against
// 1.7-2.3 k cycles of MFMAs (tools/stamp_conv.py knock-outs).  Here waves 4-7 only move bytes -- LDS-DMA (global_load_lds_dwordx4: no
// registers, no ds_write pass) of 32-channel chunks into a ring of NBUF chunk buffers, NBUF - 1 chunks ahead -- and waves 0-3 only
// read fragments and multiply (one per SIMD, MT x NTW accumulator tiles each as before).  One raw s_barrier per chunk: the loaders
// arrive once chunk k has landed (counted vmcnt, younger chunks stay in flight), the multipliers once they are done with chunk
// k - 1, whose buffer the loaders then refill.
//   chunk buffer = [PMAX patch slots][64 B] + [9 taps][BN rows][64 B], both dense (a DMA piece is 1 KiB = 16 rows, lane-linear) with
//   the 16-B piece g of row r stored at position g ^ ((r >> 1) & 2): conflict-free ds_read_b128 for a 16-row window at ANY row offset
//   (tools/lds_sim.py).  Patch rows outside the image are fetched from a page of zeros; the weight images are host-packed in exactly
//   this layout (pam_conv3x3_layout() == 1).  The residual is added to the bias before the K loop (its loads run beside the first
//   chunk's DMA), so the epilogue is convert + ReLU + store.
// ====================================================================================================================
#include "pam_conv.hpp"

template <int CIN, int NTW, int MT, int PMAX, int NBUF, bool GEN = false>
__global__ __launch_bounds__(512, 1) void k_conv3x3s(C3Args a) {
    constexpr int BN = 16 * NTW, NCHUNK = CIN / 32;
    constexpr int PIMG = PMAX * 64, WIMG = 9 * BN * 64, BUF = PIMG + WIMG;
    constexpr int PPW = PMAX / 64, WPIECES = WIMG / 1024, WPW = (WPIECES + 3) / 4, NPER = PPW + WPW;   // DMA pieces per loader wave per chunk
    static_assert(PMAX % 64 == 0 && BUF % 512 == 0 && WIMG % 1024 == 0 && NPER * (NBUF - 1) <= 60 && NBUF >= 2 && NBUF <= 4, "ring shape");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = a.tiles_y * a.N;
    const int bx = xcd_order(blockIdx.x, ntiles);       // XCD-aware tile order (see k_conv3x3)
    const int n = bx / a.tiles_y, ty0 = (bx - n * a.tiles_y) * a.TH;
    const int PW = a.W + 2, npatch = (a.TH + 2) * PW;
    const int nslots = min(a.TH, a.H - ty0) * PW;
    const int n0 = blockIdx.y * BN;

    if (wave >= 4) {
        // ---- loader waves ---------------------------------------------------------------------------------------------------
        const int lw = wave - 4;
        const char* psrc[PPW];
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int s = (lw + 4 * i) * 16 + (lane >> 2);                               // slot this lane fills in piece lw + 4 i
            const int gsrc = (lane & 3) ^ ((s >> 1) & 2);
            const int py = fdiv_small(s, a.inv_pw), px = s - py * PW;
            const int iy = ty0 - 1 + py, ix = px - 1;
            const bool ok = s < npatch && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            psrc[i] = ok ? (const char*)a.in + (((size_t)n * a.H + iy) * a.W + ix) * (CIN * 2) + gsrc * 16 : (const char*)g_c3_zero + (lane & 3) * 16;
        }
        const char* wsrc = (const char*)a.wimg + (size_t)blockIdx.y * NCHUNK * WIMG + lane * 16;
        auto issue = [&](int c) {
            char* dst = smem + (size_t)((unsigned)c % (unsigned)NBUF) * BUF;
#pragma unroll
            for (int i = 0; i < (PPW > WPW ? PPW : WPW); ++i) {
                if (i < WPW) {
                    const int j = min(lw + 4 * i, WPIECES - 1);                          // a wave short of a piece re-sends the last one
                    __builtin_amdgcn_global_load_lds((glb_void*)(wsrc + (size_t)c * WIMG + j * 1024), (lds_void*)(dst + PIMG + j * 1024), 16, 0, 0);
                }
                if (i < PPW)
                    __builtin_amdgcn_global_load_lds((glb_void*)(psrc[i] + c * 64), (lds_void*)(dst + (lw + 4 * i) * 1024), 16, 0, 0);
            }
        };
#pragma unroll
        for (int c = 0; c < NBUF - 1; ++c)
            if (c < NCHUNK) issue(c);
        for (int k = 0; k < NCHUNK; ++k) {
            const int fly = min(NCHUNK - 1 - k, NBUF - 2);                               // younger chunks that may stay in flight
            dma_ring_wait<NPER, NBUF>(fly);
            asm volatile("s_barrier" ::: "memory");
            if (k + NBUF - 1 < NCHUNK) issue(k + NBUF - 1);
        }
        return;
    }

    // ---- multiplier waves ---------------------------------------------------------------------------------------------------
    C3_STAMP(0);
    f32x4 acc[MT][NTW];
    uint32_t gres[GEN ? MT : 1][2 * NTW];                 // GEN (Darknet activation codes): the residual rows stay in registers until the epilogue
    {
        f32x4 bias4[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) bias4[j] = a.bias ? *(const f32x4*)(a.bias + n0 + g * 4 * NTW + j * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (GEN && a.res) {
            const auto rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, (int)((size_t)a.N * a.H * a.W * a.Cout * 2), 0x00020000);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int p = wave * 16 * MT + i * 16 + (lane & 15);
                const int py = fdiv_small(p, a.inv_pw), px = p - py * PW;
                const bool ok = p < nslots && px < a.W;
                const unsigned o = ok ? (unsigned)(((((size_t)n * a.H + ty0 + py) * a.W + px) * a.Cout + n0 + g * 4 * NTW) * 2) : OOB_OFFSET;
                c3_row_load<NTW>(rs_res, o, g, gres[GEN ? i : 0]);
            }
        }
        if (!GEN && a.res) {
            const auto rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, (int)((size_t)a.N * a.H * a.W * a.Cout * 2), 0x00020000);
            uint32_t rres[MT][2 * NTW];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int p = wave * 16 * MT + i * 16 + (lane & 15);
                const int py = fdiv_small(p, a.inv_pw), px = p - py * PW;
                const bool ok = p < nslots && px < a.W;
                const unsigned o = ok ? (unsigned)(((((size_t)n * a.H + ty0 + py) * a.W + px) * a.Cout + n0 + g * 4 * NTW) * 2) : OOB_OFFSET;
                c3_row_load<NTW>(rs_res, o, g, rres[i]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) {
                    acc[i][j][0] = bias4[j][0] + __builtin_bit_cast(float, rres[i][2 * j] << 16);
                    acc[i][j][1] = bias4[j][1] + __builtin_bit_cast(float, rres[i][2 * j] & 0xffff0000u);
                    acc[i][j][2] = bias4[j][2] + __builtin_bit_cast(float, rres[i][2 * j + 1] << 16);
                    acc[i][j][3] = bias4[j][3] + __builtin_bit_cast(float, rres[i][2 * j + 1] & 0xffff0000u);
                }
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j) acc[i][j] = bias4[j];
        }
    }
    // LDS byte offsets (inside a chunk buffer) of this lane's patch fragment for M tile i and tap t, swizzle included
    // M tile i sits 16 slots = 1024 bytes behind tile 0 and has the same swizzle (it depends on bit 2 of the slot only): nine offsets
    // + immediates instead of MT x 9 registers
    unsigned aoff0[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int s = wave * 16 * MT + (lane & 15) + (t / 3) * PW + (t % 3);
        aoff0[t] = (unsigned)(s * 64 + ((g ^ ((s >> 1) & 2)) << 4));
    }
    const unsigned woff = (unsigned)(PIMG + (lane & 15) * 64 + ((g ^ ((lane >> 1) & 2)) << 4));   // row j*16 + (lane & 15): bit 2 of the row = bit 2 of the lane

    // One software pipeline over all NCHUNK * 9 k-steps: the fragments of step s + 1 are read while the MFMAs of step s issue, and a
    // chunk boundary (drain this wave's LDS reads, barrier, first reads of the next chunk) sits between the last tap's reads and its
    // MFMAs, so the barrier and the first read latency of a chunk hide under 12 MFMAs.  Fragment slots alternate with (k + t) & 1.
    bf16x8 af[2][MT], bfr[2][NTW];
    auto ldfrag = [&](int k, int t, bf16x8* af_, bf16x8* bf_) {
        const char* buf = smem + (size_t)((unsigned)k % (unsigned)NBUF) * BUF;
#pragma unroll
        for (int j = 0; j < NTW; ++j) bf_[j] = *(const bf16x8*)(buf + woff + (t * BN + j * 16) * 64);
#ifdef PAM_KO_PIXREADS                                     // timing knock-out (wrong results): pixel fragments read for the kx = 0 taps only
        if (t % 3 == 0)
#endif
#pragma unroll
        for (int i = 0; i < MT; ++i) af_[i] = *(const bf16x8*)(buf + aoff0[t] + i * 1024);
    };
    auto chunk = [&](int k, auto PARC) {
        constexpr int PAR = decltype(PARC)::value;
        C3_STAMP(3 + 3 * (k & 15));
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            constexpr int dummy = 0; (void)dummy;
            const int cur = (t + PAR) & 1, nxt = cur ^ 1;
            if (t + 1 < 9) ldfrag(k, t + 1, af[nxt], bfr[nxt]);
            else if (k + 1 < NCHUNK) {
                __builtin_amdgcn_s_waitcnt(0xC07F);                                       // lgkmcnt(0): this wave is done reading chunk k
                asm volatile("s_barrier" ::: "memory");                                   // chunk k + 1 has landed; chunk k's buffer is free
                ldfrag(k + 1, 0, af[nxt], bfr[nxt]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bfr[cur][j]),
                                                                       __builtin_bit_cast(bf16x8_t, af[cur][i]), acc[i][j], 0, 0, 0);
            // issue order inside the step: the next step's MT + NTW fragment reads spread between this step's MFMAs (a burst of reads
            // ahead of the MFMAs holds the wave's issue slot ~100 cycles per step with the matrix pipe idle)
            if constexpr (MT * NTW >= MT + NTW) spread<MT * NTW, MT + NTW>();   // (16-channel slabs: more reads than MFMAs, the compiler's order)
            __builtin_amdgcn_sched_barrier(0);
        }
        C3_STAMP(4 + 3 * (k & 15));
    };
    asm volatile("s_barrier" ::: "memory");                                              // chunk 0 has landed (and is visible)
    ldfrag(0, 0, af[0], bfr[0]);
    for (int k = 0; k < NCHUNK; k += 2) {
        chunk(k, std::integral_constant<int, 0>{});
        if (k + 1 < NCHUNK) chunk(k + 1, std::integral_constant<int, 1>{});
    }
    C3_STAMP(60);

    // ---- epilogue straight from the accumulators (row permutation of the slab as in k_conv3x3: 4*NTW contiguous channels per lane)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int p = wave * 16 * MT + i * 16 + (lane & 15);
        const int py = fdiv_small(p, a.inv_pw), px = p - py * PW;
        if (p < nslots && px < a.W) {
            uint32_t ov[2 * NTW];
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                if constexpr (GEN) {                     // epi_act's arithmetic: act & 3 = 0 linear / 1 ReLU / 2 leaky / 3 mish; act & 4: the residual is added after it
                    const uint32_t r01 = a.res ? gres[GEN ? i : 0][2 * j] : 0u, r23 = a.res ? gres[GEN ? i : 0][2 * j + 1] : 0u;
                    acc[i][j][0] = epi_act_gen(acc[i][j][0], __builtin_bit_cast(float, r01 << 16), a.relu);
                    acc[i][j][1] = epi_act_gen(acc[i][j][1], __builtin_bit_cast(float, r01 & 0xffff0000u), a.relu);
                    acc[i][j][2] = epi_act_gen(acc[i][j][2], __builtin_bit_cast(float, r23 << 16), a.relu);
                    acc[i][j][3] = epi_act_gen(acc[i][j][3], __builtin_bit_cast(float, r23 & 0xffff0000u), a.relu);
                }
                ov[2 * j] = pack_bf16x2_ew(acc[i][j][0], acc[i][j][1]); ov[2 * j + 1] = pack_bf16x2_ew(acc[i][j][2], acc[i][j][3]);
                if (!GEN && a.relu) {
                    ov[2 * j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j]), (s16x2){0, 0}));
                    ov[2 * j + 1] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j + 1]), (s16x2){0, 0}));
                }
            }
            row_store<NTW>(a.out + (((size_t)n * a.H + ty0 + py) * a.W + px) * a.Cout + n0 + g * 4 * NTW, g, ov);
        }
    }
    C3_STAMP(61);
}

template <int CIN, int NTW, int MT, int PMAX>
static int launch_c3s_gen_one(hipStream_t s, const C3Args& a) {
    constexpr size_t lds = (size_t)2 * (PMAX * 64 + 9 * 16 * NTW * 64);
    if (!pam_max_dynamic_lds((const void*)k_conv3x3s<CIN, NTW, MT, PMAX, 2, true>, (int)lds)) return PAM_E_HIP;
    CONV_KIND(PAM_CONV_KERNEL_3X3S, 100000 + CIN * 100 + NTW * 10 + MT);
    pam_launch(k_conv3x3s<CIN, NTW, MT, PMAX, 2, true>, dim3(a.tiles_y * a.N, a.Cout / (16 * NTW)), dim3(512), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
// the general-activation instantiations (tile_cfg -7)
static int launch_c3s_gen(hipStream_t s, const C3Args& a, int Cin, int mt) {
    switch (Cin * 10 + mt) {
        case 1284: return launch_c3s_gen_one<128, 4, 4, 320>(s, a);
        case 1285: return launch_c3s_gen_one<128, 4, 5, 384>(s, a);
        case 2564: return launch_c3s_gen_one<256, 2, 4, 320>(s, a);
        case 2565: return launch_c3s_gen_one<256, 2, 5, 384>(s, a);
        case 5124: return launch_c3s_gen_one<512, 2, 4, 320>(s, a);
        case 5125: return launch_c3s_gen_one<512, 2, 5, 384>(s, a);
    }
    return PAM_E_ARG;
}
template <int CIN, int NTW, int MT, int PMAX, int NBUF>
static int launch_c3s_one(hipStream_t s, const C3Args& a) {
    constexpr size_t lds = (size_t)NBUF * (PMAX * 64 + 9 * 16 * NTW * 64);
    static_assert(lds <= 160 * 1024, "LDS");
    if (!pam_max_dynamic_lds((const void*)k_conv3x3s<CIN, NTW, MT, PMAX, NBUF>, (int)lds)) return PAM_E_HIP;
    CONV_KIND(PAM_CONV_KERNEL_3X3S, CIN * 100 + NTW * 10 + MT);
    pam_launch(k_conv3x3s<CIN, NTW, MT, PMAX, NBUF>, dim3(a.tiles_y * a.N, a.Cout / (16 * NTW)), dim3(512), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
int launch_c3s(hipStream_t s, const C3Args& a, const ConvPlan& p) {
    const int Cin = p.cin, ntw = p.ntw, mt = p.mt, pmax = p.pmax;
    if (p.gen) return launch_c3s_gen(s, a, Cin, mt);
#ifdef PAM_DIAG
    static const int nbuf = getenv("PAM_C3S_NBUF") ? atoi(getenv("PAM_C3S_NBUF")) : 0;       // tuning hook
    if (Cin == 384 && ntw == 4 && mt == 3 && nbuf == 2) return launch_c3s_one<384, 4, 3, 192, 2>(s, a);
#endif
    if (Cin == 64 || Cin == 256) {                       // layer1 / transition1: every (M tiles, patch) shape the pick can return for them
        switch ((Cin == 64 ? 0 : 10) + (pmax == 448 ? 6 : mt)) {
            case 3: return launch_c3s_one<64, 4, 3, 192, 2>(s, a);
            case 4: return launch_c3s_one<64, 4, 4, 320, 2>(s, a);
            case 5: return launch_c3s_one<64, 4, 5, 384, 2>(s, a);
            case 6: return launch_c3s_one<64, 4, 5, 448, 2>(s, a);
            case 13: return launch_c3s_one<256, 3, 3, 192, 3>(s, a);
            case 14: return launch_c3s_one<256, 3, 4, 320, 2>(s, a);
            case 15: return launch_c3s_one<256, 3, 5, 384, 2>(s, a);
            case 16: return launch_c3s_one<256, 3, 5, 448, 2>(s, a);
        }
        return PAM_E_ARG;
    }
    if (pmax == 448) return PAM_E_ARG;
    switch (Cin * 100 + ntw * 10 + mt) {
        case 9633: return launch_c3s_one<96, 3, 3, 192, 2>(s, a);
        case 9634: return launch_c3s_one<96, 3, 4, 320, 2>(s, a);
        case 9635: return launch_c3s_one<96, 3, 5, 384, 2>(s, a);
        case 19243: return launch_c3s_one<192, 4, 3, 192, 3>(s, a);
        case 19244: return launch_c3s_one<192, 4, 4, 320, 2>(s, a);
        case 19245: return launch_c3s_one<192, 4, 5, 384, 2>(s, a);
        case 38443: return launch_c3s_one<384, 4, 3, 192, 3>(s, a);
        case 38444: return launch_c3s_one<384, 4, 4, 320, 2>(s, a);
        case 38445: return launch_c3s_one<384, 4, 5, 384, 2>(s, a);
        // 32-channel slabs (tile_cfg -8: forwards of a few crops, where a launch is as long as ONE workgroup): twice the workgroups, half
        // the MFMAs and 18 instead of 36 KB of weights per chunk each, three chunk buffers
        case 19223: return launch_c3s_one<192, 2, 3, 192, 3>(s, a);
        case 19224: return launch_c3s_one<192, 2, 4, 320, 3>(s, a);
        case 19225: return launch_c3s_one<192, 2, 5, 384, 3>(s, a);
        case 38423: return launch_c3s_one<384, 2, 3, 192, 3>(s, a);
        case 38424: return launch_c3s_one<384, 2, 4, 320, 3>(s, a);
        case 38425: return launch_c3s_one<384, 2, 5, 384, 3>(s, a);
    }
    return PAM_E_ARG;
}
