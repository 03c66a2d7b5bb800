// libpam_hip.so, conv stack
// ====================================================================================================================
// k_conv3x3: 3x3 / stride 1 / pad 1 convolutions (85 % of HRNet-W48's FLOPs) with the input rows resident in LDS.
//
// A workgroup owns TH full image rows of one image and one slab of BN = 16*NTW output channels.  Output "slots" are the
// positions of the PADDED row-major grid (PW = W + 2 columns): slot p <-> window corner at patch pixel p, so the MFMA A
// fragment of tap (ky,kx) is one ds_read_b128 at (p + ky*PW + kx) * PITCH_A -- linear in p, conflict-free at
// PITCH_A = 96 B -- and the two junk columns per row are simply not stored.  K is walked in chunks of CK input channels:
// the (TH+2) x PW x CK patch chunk and the [BN][9][CK] weight chunk (pre-packed on the host as an LDS image, so its load
// is a linear 16-B copy) go global -> registers -> LDS, the next chunk in flight under the current chunk's MFMAs.
// ====================================================================================================================
#include "pam_conv.hpp"

// the deep small-image layers run one workgroup per CU (one wave per SIMD): give those instantiations the whole register
// file, otherwise the scheduler, starved by the chunk-prefetch registers, reads each MFMA fragment right before its use
template <int CIN, int NTW, int MT, int NWAVES, int PMAX>
__global__ __launch_bounds__(64 * NWAVES, (c3_ck(CIN) == 64 ? 1 : 2)) void k_conv3x3(C3Args a) {
    constexpr int T = 64 * NWAVES, BN = 16 * NTW;
    constexpr int CK = c3_ck(CIN), NCHUNK = CIN / CK, PC8 = CK / 8;
    constexpr int PITCH_A = c3_pitch_a(CIN), PITCH_W = c3_pitch_w(CIN);
    constexpr int NPP = (PMAX * PC8 + T - 1) / T;                        // patch pieces per thread per chunk (PMAX >= patch pixels)
    constexpr int WIMG = BN * PITCH_W;                                    // bytes of one weight chunk image
    constexpr int NWP = (WIMG / 16 + T - 1) / T;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (C3_DBG(8)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    // XCD-aware tile order: workgroups b, b+8, b+16, ... share an XCD (and its L2), so give each XCD a contiguous run of
    // tiles -- vertically adjacent tiles re-read each other's halo rows, which then hit that L2 instead of the fabric
    // Single-chunk layers (Cin = 48) are PERSISTENT: the grid is capped at the resident workgroups and each one walks tiles
    // v = blockIdx.x, + gridDim.x, ... with the slab's weights staged once and the next tile's patch in flight (registers)
    // under the current tile's epilogue.  gridDim.x is a multiple of 8 then, so a workgroup stays on its XCD's run.
    const int ntiles = a.tiles_y * a.N;
    auto tile_of = [&](int v) { return xcd_order(v, ntiles); };
    int vtile = blockIdx.x;
    int bx = tile_of(vtile);
    int n = bx / a.tiles_y, ty0 = (bx - n * a.tiles_y) * a.TH;
    const int PW = a.W + 2, npatch = (a.TH + 2) * PW;   // full-height patch: rows below a ragged last tile load as zeros
    int nslots = min(a.TH, a.H - ty0) * PW;
    const int n0 = blockIdx.y * BN;
    char* Wsm = smem + ((((size_t)npatch + 2) * PITCH_A + 15) & ~(size_t)15);   // junk-slot reads past the patch land in the weights (in bounds)
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((size_t)a.N * a.H * a.W * CIN * 2), 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.wimg, 0, (int)((size_t)(a.Cout / BN) * NCHUNK * WIMG), 0x00020000);
    const auto rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(a.res ? a.res : a.out), 0, (int)((size_t)a.N * a.H * a.W * a.Cout * 2), 0x00020000);
    uint32_t rres[MT][2 * NTW];                         // residual row piece of this lane: 4*NTW contiguous channels
    char* zero_slot = Wsm + WIMG;                       // 64 zero bytes: K-tail A lanes (CIN = 48) + slack behind the last weight row
    if (tid < 4) *(u32x4*)(zero_slot + tid * 16) = (u32x4){0, 0, 0, 0};

    const unsigned wimg0 = (unsigned)((size_t)blockIdx.y * NCHUNK * WIMG);
    u32x4 ra[NPP], rw[NWP];
    auto gload_w = [&](int cc) {                        // weight chunk image: linear 16-byte copy, no descriptors
#pragma unroll
        for (int i = 0; i < NWP; ++i) {
            const int q = tid + i * T;
            rw[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, q < WIMG / 16 ? (unsigned)(q * 16) : OOB_OFFSET, wimg0 + (unsigned)cc * WIMG, 0);
        }
    };
    C3_STAMP(0);
    f32x4 bias4[NTW];                                   // lane group g ends with channels n0 + 4*NTW*g + 4*j + r (see the epilogue)
#pragma unroll
    for (int j = 0; j < NTW; ++j) bias4[j] = a.bias ? *(const f32x4*)(a.bias + n0 + g * 4 * NTW + j * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    if (!C3_DBG(1)) gload_w(0);                         // in flight while the patch descriptors are computed

    // ---- per-thread patch piece descriptors (fixed over the chunk loop) -------------------------------------------------
    unsigned goffA[NPP];
    int tid_v;
    auto descriptors = [&](int n_, int ty0_) {
#pragma unroll
        for (int i = 0; i < NPP; ++i) {
            const int q = tid_v + i * T;
            goffA[i] = OOB_OFFSET;
            if (q < npatch * PC8) {
                const int pp = q / PC8, c8 = q - pp * PC8;
                const int pyy = fdiv_small(pp, a.inv_pw), pxx = pp - pyy * PW;
                const int iy = ty0_ - 1 + pyy, ix = pxx - 1;
                if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                    goffA[i] = (unsigned)((((size_t)n_ * a.H + iy) * a.W + ix) * CIN * 2 + c8 * 16);
            }
        }
    };
    tid_v = tid;
    descriptors(n, ty0);
    auto gload_a = [&](int cc) {
        const unsigned so = (unsigned)(cc * CK * 2);
#pragma unroll
        for (int i = 0; i < NPP; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, goffA[i], goffA[i] == OOB_OFFSET ? 0 : so, 0);
    };
    auto gload = [&](int cc) { gload_w(cc); gload_a(cc); };
    auto lstore = [&](bool with_weights) {
#pragma unroll
        for (int i = 0; i < NPP; ++i) {
            const int q = tid_v + i * T;
            if (q < npatch * PC8) { const int pp = q / PC8, c8 = q - pp * PC8; *(u32x4*)(smem + (size_t)pp * PITCH_A + c8 * 16) = ra[i]; }
        }
        if (with_weights) {
#pragma unroll
            for (int i = 0; i < NWP; ++i) {
                const int q = tid + i * T;
                if (q < WIMG / 16) *(u32x4*)(Wsm + (size_t)q * 16) = rw[i];
            }
        }
    };

    f32x4 acc[MT][NTW];

    // slot of this lane in M tile i: p = wave*16*MT + i*16 + (lane & 15); A byte offset = p * PITCH_A (+ tap, + k slice)
    const int p_lane = wave * 16 * MT + (lane & 15);
    const char* al = smem + (size_t)p_lane * PITCH_A;
    const char* wl = Wsm + (size_t)(lane & 15) * PITCH_W;

    if (C3_DBG(16)) { if (goffA[0] == 12345u) a.out[0] = 1; return; }
    if (!C3_DBG(1)) gload_a(0);
    C3_STAMP(1);
    if constexpr (NCHUNK == 1) {                        // the slab's only weight chunk is staged once, outside the tile loop
#pragma unroll
        for (int i = 0; i < NWP; ++i) {
            const int q = tid + i * T;
            if (q < WIMG / 16) *(u32x4*)(Wsm + (size_t)q * 16) = rw[i];
        }
    }
    tid_v = tid;                                        // opaque per iteration: keeps per-piece addresses from being hoisted (VGPRs)
    for (bool first = true;; first = false) {           // tile loop (one pass unless persistent)
    if constexpr (NCHUNK == 1) asm volatile("" : "+v"(tid_v));
    const int vnext = vtile + (int)gridDim.x;
    const bool has_next = NCHUNK == 1 && vnext < ntiles;
    int n_nx = 0, ty0_nx = 0;
    // accumulators start from the bias (loaded first of all, so waiting for it never waits for the tile loads behind it)
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][j] = bias4[j];
    for (int cc = 0; cc < NCHUNK; ++cc) {
        if (cc > 0 || !first) __syncthreads();          // every wave is done reading the previous chunk / tile
        C3_STAMP(2 + 4 * cc);
        if (!C3_DBG(32)) lstore(NCHUNK > 1);
        C3_STAMP(3 + 4 * cc);
        __syncthreads();
        C3_STAMP(4 + 4 * cc);
        if (cc + 1 < NCHUNK && !C3_DBG(1)) gload(cc + 1);               // next chunk in flight under the MFMAs below
        if (cc == NCHUNK - 1 && a.res) {                                // residual tile in flight under the last chunk's MFMAs
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int p = wave * 16 * MT + i * 16 + (lane & 15);
                const int py = fdiv_small(p, a.inv_pw), px = p - py * PW;
                const bool ok = p < nslots && px < a.W;
                const unsigned o = ok ? (unsigned)(((((size_t)n * a.H + ty0 + py) * a.W + px) * a.Cout + n0 + g * 4 * NTW) * 2) : OOB_OFFSET;
                c3_row_load<NTW>(rs_res, o, g, rres[i]);
            }
        }
        if (C3_DBG(2)) continue;
        // K loop, software-pipelined by hand: the fragments of step s+1 are read from LDS while the MFMAs of step s issue
        // (with one wave per SIMD nothing else hides the ds_read latency)
        constexpr int NSTEP = (CIN == 48) ? 14 : 9 * (CK / 32);
        bf16x8 af[2][MT], bfr[2][NTW];
        auto ldfrag = [&](int st, bf16x8* af_, bf16x8* bf_) {
            if constexpr (CIN == 48) {
                const int k0 = 32 * st + 8 * g;                          // flattened (tap, c); an 8-slice never straddles taps
                const int t = k0 / 48, c = k0 - t * 48;
                const int ky = t / 3, kx = t - ky * 3;
                const bool zero = k0 >= 432;
                const unsigned aoff = (unsigned)((ky * PW + kx) * PITCH_A + c * 2);
#pragma unroll
                for (int j = 0; j < NTW; ++j) bf_[j] = *(const bf16x8*)(wl + (size_t)j * 16 * PITCH_W + k0 * 2);
#pragma unroll
                for (int i = 0; i < MT; ++i) af_[i] = *(const bf16x8*)(zero ? zero_slot : al + (size_t)i * 16 * PITCH_A + aoff);
            } else {
                constexpr int KS = CK / 32;
                const int t = st / KS, ks = st - t * KS;
                const int ky = t / 3, kx = t - ky * 3;
                const unsigned aoff = (unsigned)((ky * PW + kx) * PITCH_A + ks * 64 + g * 16);
#pragma unroll
                for (int j = 0; j < NTW; ++j) bf_[j] = *(const bf16x8*)(wl + (size_t)j * 16 * PITCH_W + st * 64 + g * 16);
#pragma unroll
                for (int i = 0; i < MT; ++i) af_[i] = *(const bf16x8*)(al + (size_t)i * 16 * PITCH_A + aoff);
            }
        };
        ldfrag(0, af[0], bfr[0]);
#pragma unroll
        for (int st = 0; st < NSTEP; ++st) {
            if (st + 1 < NSTEP) ldfrag(st + 1, af[(st + 1) & 1], bfr[(st + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);          // keep the next step's ds_reads ahead of this step's MFMAs (hipcc sinks them otherwise)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bfr[st & 1][j]),
                                                                       __builtin_bit_cast(bf16x8_t, af[st & 1][i]), acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        C3_STAMP(5 + 4 * cc);
    }

    // ---- epilogue straight from the accumulators.  With the weights as the MFMA A operand the D tile has channels on
    // its rows, and the host packs the slab's weight rows so that row j*16 + 4g + r is channel n0 + 4*NTW*g + 4j + r: this
    // lane then holds 4*NTW CONTIGUOUS channels of pixel slot i*16 + (lane & 15) -> residual loads and stores are 16 bytes
    // wide (the store tail is issue-bound), and the 4 lane groups of a pixel cover the slab's 32*NTW contiguous bytes.
    C3_STAMP(60);
    if (C3_DBG(4)) { if (tid == 0) a.out[(size_t)blockIdx.x * 8] = (uint16_t)acc[0][0][0]; return; }
    if (has_next) {     // next TILE's patch goes in flight under this tile's epilogue (the fragment registers are free again by now)
        const int b2 = tile_of(vnext);
        n_nx = b2 / a.tiles_y; ty0_nx = (b2 - n_nx * a.tiles_y) * a.TH;
        descriptors(n_nx, ty0_nx);
        gload_a(0);
    }
    // RES / RELU are compile-time in the HRNet instantiations (a uniform branch picks one of four copies): per 4 values the
    // epilogue is then 4 unpack + 4 add (residual only), 2 v_cvt_pk_bf16_f32 and ReLU as ONE packed integer max per dword
    // (bf16 is sign-magnitude: max(int16, 0) clears exactly the negative values) -- the tail is VALU-issue bound.
    auto epilogue = [&](auto RESC, auto RELUC, auto GENC) {
        constexpr bool RES = decltype(RESC)::value, RELU = decltype(RELUC)::value, GEN = decltype(GENC)::value;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int p = wave * 16 * MT + i * 16 + (lane & 15);
            const int py = fdiv_small(p, a.inv_pw), px = p - py * PW;
            if (p < nslots && px < a.W) {
                uint32_t ov[2 * NTW];
#pragma unroll
                for (int j = 0; j < NTW; ++j) {
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    float rr[4] = {0.f, 0.f, 0.f, 0.f};
                    if (GEN ? (a.res != nullptr) : RES) {
                        rr[0] = __builtin_bit_cast(float, rres[i][2 * j] << 16); rr[1] = __builtin_bit_cast(float, rres[i][2 * j] & 0xffff0000u);
                        rr[2] = __builtin_bit_cast(float, rres[i][2 * j + 1] << 16); rr[3] = __builtin_bit_cast(float, rres[i][2 * j + 1] & 0xffff0000u);
                    }
                    if constexpr (GEN) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = epi_act(v[r], rr[r], a.relu);
                        ov[2 * j] = pack_bf16x2_ew(v[0], v[1]); ov[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
                    } else {
                        if constexpr (RES) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] += rr[r];
                        }
                        ov[2 * j] = pack_bf16x2_ew(v[0], v[1]); ov[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
                        if constexpr (RELU) {
                            ov[2 * j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j]), (s16x2){0, 0}));
                            ov[2 * j + 1] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j + 1]), (s16x2){0, 0}));
                        }
                    }
                }
                row_store<NTW>(a.out + (((size_t)n * a.H + ty0 + py) * a.W + px) * a.Cout + n0 + g * 4 * NTW, g, ov);
            }
        }
    };
    typedef std::true_type T_; typedef std::false_type F_;
    if constexpr (c3_general_act(CIN)) {
        epilogue(F_{}, F_{}, T_{});
    } else if (a.res) {
        if (a.relu) epilogue(T_{}, T_{}, F_{}); else epilogue(T_{}, F_{}, F_{});
    } else {
        if (a.relu) epilogue(F_{}, T_{}, F_{}); else epilogue(F_{}, F_{}, F_{});
    }
    if (!has_next) break;
    vtile = vnext; n = n_nx; ty0 = ty0_nx; nslots = min(a.TH, a.H - ty0) * PW;
    }   // tile loop
    C3_STAMP(61);
}

template <int CIN, int NTW, int MT, int NWAVES, int PMAX>
static int launch_c3_one(hipStream_t s, const C3Args& a) {
    const int npatch = (a.TH + 2) * (a.W + 2);
    if (npatch > PMAX) return PAM_E_ARG;
    dim3 grid(a.tiles_y * a.N, a.Cout / (16 * NTW));
    const size_t lds = c3_lds_bytes(CIN, NTW, npatch);
    if (lds > 150 * 1024) return PAM_E_ARG;
    CONV_KIND(PAM_CONV_KERNEL_3X3, CIN * 10 + NTW);
    if (CIN / c3_ck(CIN) == 1 && !C3_DBG(128)) {        // single-chunk layers: persistent workgroups (see the kernel)
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_conv3x3<CIN, NTW, MT, NWAVES, PMAX>, 64 * NWAVES, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        // One workgroup per CU while a workgroup has only a few tiles to walk: the layer then leaves half of every CU's LDS and
        // registers to the kernels of the other branch streams (measured +2 % on the 20-crop forward; with two per CU the Cin-48
        // chain shuts the other branches out and they run after it).  Large batches fill the chip on their own: all resident slots.
#ifdef PAM_DIAG
        static const int cap = getenv("PAM_C3_PERSIST_SLOTS") ? atoi(getenv("PAM_C3_PERSIST_SLOTS")) : 0;     // tuning override
#else
        constexpr int cap = 0;
#endif
        int slots = 256 * per_cu / (int)grid.y / 8 * 8;
        const int few = cap > 0 ? cap : ((int)grid.x < 4 * 256 ? 256 : slots);
        if (slots > few) slots = few / 8 * 8;
        if (slots >= 8 && (int)grid.x > slots) grid.x = slots;
    }
    pam_launch(k_conv3x3<CIN, NTW, MT, NWAVES, PMAX>, grid, dim3(64 * NWAVES), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
// p.cfg = MT * 10 + NWAVES  (MT = 4; NWAVES in {2, 3, 4}); the patch bound PMAX is picked from the actual tile
template <int CIN, int NTW>
static int launch_c3_cfg(hipStream_t s, const C3Args& a, int cfg) {
    const int npatch = (a.TH + 2) * (a.W + 2);
    switch (cfg) {
        case 42: return npatch <= 160 ? launch_c3_one<CIN, NTW, 4, 2, 160>(s, a) : launch_c3_one<CIN, NTW, 4, 2, 288>(s, a);
        case 43: return npatch <= 160 ? launch_c3_one<CIN, NTW, 4, 3, 160>(s, a) : launch_c3_one<CIN, NTW, 4, 3, 352>(s, a);
        case 44: return npatch <= 288 ? launch_c3_one<CIN, NTW, 4, 4, 288>(s, a) : launch_c3_one<CIN, NTW, 4, 4, 416>(s, a);
        case 54:                                         // 5 M tiles per wave (320 slots): taller tiles -> a layer of <= 256 workgroups, each alone on its CU
            if constexpr (CIN == 96 || CIN == 192) return launch_c3_one<CIN, NTW, 5, 4, 416>(s, a);
            else return PAM_E_ARG;
    }
    return PAM_E_ARG;
}
int launch_c3(hipStream_t s, const C3Args& c, const ConvPlan& p) {
    const int cfg = p.cfg;
    switch (p.cin * 10 + p.ntw) {
        case 483: return launch_c3_cfg<48, 3>(s, c, cfg);
        case 643: return launch_c3_cfg<64, 3>(s, c, cfg);
        case 963: return launch_c3_cfg<96, 3>(s, c, cfg);
        case 1923: return launch_c3_cfg<192, 3>(s, c, cfg);
        case 3843: return launch_c3_cfg<384, 3>(s, c, cfg);
        case 484: return launch_c3_cfg<48, 4>(s, c, cfg);
        case 644: return launch_c3_cfg<64, 4>(s, c, cfg);
        case 964: return launch_c3_cfg<96, 4>(s, c, cfg);
        case 1924: return launch_c3_cfg<192, 4>(s, c, cfg);
        case 3844: return launch_c3_cfg<384, 4>(s, c, cfg);
        case 1922: return launch_c3_cfg<192, 2>(s, c, cfg);
        case 3842: return launch_c3_cfg<384, 2>(s, c, cfg);
        case 1921: return launch_c3_cfg<192, 1>(s, c, cfg);
        case 3841: return launch_c3_cfg<384, 1>(s, c, cfg);
        case 1284: return launch_c3_cfg<128, 4>(s, c, cfg);     // Darknet-53 widths
        case 2564: return launch_c3_cfg<256, 4>(s, c, cfg);
        case 2563: return launch_c3_cfg<256, 3>(s, c, cfg);     // HRNet transition1: 256 -> 48 at 96 x 72
        case 2562: return launch_c3_cfg<256, 2>(s, c, cfg);
        case 5124: return launch_c3_cfg<512, 4>(s, c, cfg);
        case 5122: return launch_c3_cfg<512, 2>(s, c, cfg);
        case 322: return launch_c3_cfg<32, 2>(s, c, cfg);       // HRNet-W32's 32-channel branch (unfused BasicBlocks)
    }
    return PAM_E_ARG;
}
