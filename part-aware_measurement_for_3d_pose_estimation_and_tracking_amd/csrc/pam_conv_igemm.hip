// libpam_hip.so, conv stack: k_conv_igemm, the generic NHWC bf16 convolution (1x1 / 3x3, stride 1 / 2) as an implicit GEMM
//     D[pixel][cout] = sum_k A[pixel][k] * Wt[cout][k],   k = (ky, kx, cin) flattened, cin fastest
// on v_mfma_f32_16x16x32_bf16 (wave64), with the whole epilogue fused: + bias (folded BatchNorm) [+ residual] [ReLU],
// fp32 accumulate, one bf16 rounding.  The A operand is gathered on the fly (no im2col buffer): each 16-byte piece is
// 8 consecutive input channels of one tap of one output pixel (Cin % 8 == 0), zero-filled outside the image.
#include "pam_conv.hpp"

constexpr int ROWB = KC * 2 + 16;    // LDS row pitch in bytes: 128 B of data + 16 B pad (spreads ds_read_b128 over banks)

// Block tile: BM = 64*WM output pixels x BN = 16*NTW*WN output channels; each wave owns 64 pixels x 16*NTW channels
// (4 x NTW accumulator tiles of 16x16).  K is walked in chunks of 64; chunk c+1 is fetched (buffer_load, zero-fill by the
// descriptor's range check, no branches) while chunk c is multiplied out of LDS.
template <int NTW, int WM, int WN, bool GEN>
__device__ __forceinline__ void conv_igemm_body(const ConvArgs& a, const int bx, const int by) {
    constexpr int T = 64 * WM * WN, BM = 64 * WM, BN = 16 * NTW * WN;
    constexpr int APT = (BM * 8 + T - 1) / T;          // A pieces (16 B) per thread per chunk (the last pass is partial when T does not divide BM * 8)
    constexpr int BPT = (BN * 8 + T - 1) / T;          // B pieces per thread per chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // two chunk buffers each -- or one when the whole K is a single chunk (1x1 layers with 64 input channels: half the LDS, twice
    // the workgroups per CU for layers that are one load -> multiply -> store chain per workgroup)
    const int nbuf = a.Kpad > KC ? 2 : 1;
    char* As = smem;                                   // [nbuf][BM][ROWB]
    char* Bs = smem + nbuf * BM * ROWB;                // [nbuf][BN][ROWB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = bx * BM, n0 = by * BN;
    const int kq = tid & 7;
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((size_t)a.N * a.H * a.W * a.in_cs * 2), 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, (int)((size_t)a.Cout * a.Kpad * 2), 0x00020000);

    // per-thread output-pixel rows of the A tile (fixed over the K loop): byte offset of the window corner and a
    // validity bit per tap
    unsigned rowoff[APT], tapmask[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
        const int row = (tid >> 3) + i * (T / 8);
        const int m = m0 + row;
        rowoff[i] = 0; tapmask[i] = 0;
        if (m < a.M && row < BM) {
            const int hw = a.Ho * a.Wo;
            const int n = m / hw, r = m - n * hw, oy = r / a.Wo, ox = r - oy * a.Wo;
            const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
            rowoff[i] = (unsigned)((((long)n * a.H + iy0) * a.W + ix0) * a.in_cs * 2); // may wrap; only used with valid taps
            unsigned mk = 0;
            for (int ky = 0; ky < a.KH; ++ky)
                for (int kx = 0; kx < a.KW; ++kx)
                    if ((unsigned)(iy0 + ky) < (unsigned)a.H && (unsigned)(ix0 + kx) < (unsigned)a.W) mk |= 1u << (ky * a.KW + kx);
            tapmask[i] = mk;
        }
    }
    int kc_c = kq * 8, kc_tap = 0;                      // channel / tap of this thread's piece in the current chunk
    while (kc_c >= a.Cin) { kc_c -= a.Cin; ++kc_tap; }
    unsigned woff[BPT];
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        const int p = tid + i * T;
        // LDS weight row wn*16*NTW + j*16 + q holds output channel wn*16*NTW + 4*NTW*(q >> 2) + 4*j + (q & 3): as the MFMA A operand
        // this leaves every lane with 4*NTW contiguous channels of its pixel (same scheme as k_conv3x3)
        const int row = p >> 3, wnb = row / (16 * NTW), rem = row - wnb * 16 * NTW, q = rem & 15;
        const int ch = wnb * 16 * NTW + 4 * NTW * (q >> 2) + 4 * (rem >> 4) + (q & 3);
        woff[i] = (p < BN * 8) ? (unsigned)(((size_t)(n0 + ch) * a.Kpad + (p & 7) * 8) * 2) : OOB_OFFSET;
    }

    u32x4 areg[APT], breg[BPT];
    auto load_chunk = [&]() {
        const int ky = kc_tap / a.KW, kx = kc_tap - ky * a.KW;
        const unsigned tapoff = (unsigned)(((ky * a.W + kx) * a.in_cs + kc_c) * 2);
        const unsigned tbit = (kc_tap < a.KH * a.KW) ? (1u << kc_tap) : 0u;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
            const unsigned off = (tapmask[i] & tbit) ? rowoff[i] + tapoff : OOB_OFFSET;
            areg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            breg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, woff[i], 0, 0);
            if (woff[i] != OOB_OFFSET) woff[i] += KC * 2;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < APT; ++i) {
            const int row = (tid >> 3) + i * (T / 8);
            if (BM * 8 % T == 0 || row < BM) *(u32x4*)(As + (size_t)buf * BM * ROWB + row * ROWB + kq * 16) = areg[i];
        }
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            const int p = tid + i * T;
            if (p < BN * 8) *(u32x4*)(Bs + (size_t)buf * BN * ROWB + (p >> 3) * ROWB + (p & 7) * 16) = breg[i];
        }
    };
    auto advance = [&]() {
        kc_c += KC;
        while (kc_c >= a.Cin) { kc_c -= a.Cin; ++kc_tap; }
    };

    const int g = lane >> 4, cw0 = n0 + wn * 16 * NTW;
    f32x4 acc[4][NTW];                                  // [pixel tile][channel tile], started from the bias
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const f32x4 b4 = a.bias ? *(const f32x4*)(a.bias + cw0 + g * 4 * NTW + j * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = b4;
    }

    // residual rows of this lane's 4 pixel tiles: issued BEFORE the K loop, so their latency runs under the operand loads and the
    // MFMAs instead of in front of the stores (the 1x1 64 -> 256 + residual layers of layer1 are one K chunk long: nothing else hides it)
    const auto rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(a.res ? a.res : a.out), 0, (int)((size_t)a.M * a.Cout * 2), 0x00020000);
    uint32_t rres[4][2 * NTW];
    if (a.res) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wm * 64 + i * 16 + (lane & 15);
            const size_t o = (size_t)m * a.Cout + cw0 + g * 4 * NTW;
            c3_row_load<NTW>(rs_res, m < a.M ? (unsigned)(o * 2) : OOB_OFFSET, g, rres[i]);
        }
    }

    const int nchunks = a.Kpad / KC;
    load_chunk();
    store_chunk(0);
    advance();
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk();             // loads in flight under the MFMAs below
        const char* Ab = As + (size_t)buf * BM * ROWB + (wm * 64 + (lane & 15)) * ROWB + (lane >> 4) * 16;
        const char* Bb = Bs + (size_t)buf * BN * ROWB + (wn * 16 * NTW + (lane & 15)) * ROWB + (lane >> 4) * 16;
        // both 32-deep steps of the chunk: all fragment reads first, pinned ahead of the MFMAs (hipcc otherwise sinks each
        // ds_read to just before its first use and the LDS latency is exposed every three MFMAs)
        bf16x8 af[2][4], bfr[2][NTW];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < 4; ++i) af[ks][i] = *(const bf16x8*)(Ab + i * 16 * ROWB + ks * 64);
#pragma unroll
            for (int j = 0; j < NTW; ++j) bfr[ks][j] = *(const bf16x8*)(Bb + j * 16 * ROWB + ks * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NTW; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bfr[ks][j]),
                                                                       __builtin_bit_cast(bf16x8_t, af[ks][i]), acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nchunks) { store_chunk(buf ^ 1); advance(); }
        __syncthreads();
    }

    // epilogue straight from the accumulators: with the weights as the A operand the D tile has channels on its rows, so this
    // lane holds channels cw0 + 4*NTW*g + 4*j + r of pixel mw0 + i*16 + (lane & 15): 4*NTW contiguous channels, 16-byte accesses
    const int mw0 = m0 + wm * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = mw0 + i * 16 + (lane & 15);
        if (m < a.M) {
            const size_t o = (size_t)m * a.Cout + cw0 + g * 4 * NTW;
            uint32_t ov[2 * NTW];
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
                float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                float rr[4] = {0.f, 0.f, 0.f, 0.f};
                if (a.res) {
                    rr[0] = __builtin_bit_cast(float, rres[i][2 * j] << 16); rr[1] = __builtin_bit_cast(float, rres[i][2 * j] & 0xffff0000u);
                    rr[2] = __builtin_bit_cast(float, rres[i][2 * j + 1] << 16); rr[3] = __builtin_bit_cast(float, rres[i][2 * j + 1] & 0xffff0000u);
                }
                const bool act_on = cw0 + g * 4 * NTW + j * 4 >= a.relu_from;   // merged fuse-layer convs: only the upper channels
                if constexpr (GEN) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = epi_act_gen(v[r], rr[r], act_on ? a.relu : (a.relu & 4));
                    ov[2 * j] = pack_bf16x2_ew(v[0], v[1]); ov[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
                } else {                                // HRNet's codes 0 / 1; ReLU as a packed int16 max on the bf16 pairs
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += rr[r];
                    ov[2 * j] = pack_bf16x2_ew(v[0], v[1]); ov[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
                    if (a.relu && act_on) {
                        ov[2 * j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j]), (s16x2){0, 0}));
                        ov[2 * j + 1] = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, ov[2 * j + 1]), (s16x2){0, 0}));
                    }
                }
            }
            row_store<NTW>(a.out + o, g, ov);
        }
    }
}

template <int NTW, int WM, int WN, bool GEN>
__global__ __launch_bounds__(64 * WM * WN) void k_conv_igemm(ConvArgs a) {
    conv_igemm_body<NTW, WM, WN, GEN>(a, blockIdx.x, blockIdx.y);
}

template <int NTW, int WM, int WN>
static int launch_conv(hipStream_t s, const ConvArgs& a) {
    constexpr int BM_ = 64 * WM, BN_ = 16 * NTW * WN;
    if (a.relu > 1) {                                   // Darknet activation codes: the general-epilogue instantiation
        CONV_KIND(PAM_CONV_KERNEL_IGEMM, 1000000 + BM_ * 1000 + BN_);
        dim3 grid((a.M + BM_ - 1) / BM_, a.Cout / BN_);
        const size_t lds = (a.Kpad > KC ? 2 : 1) * (size_t)(BM_ + BN_) * ROWB;
        pam_launch(k_conv_igemm<NTW, WM, WN, true>, grid, dim3(64 * WM * WN), lds, s, a);
        return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
    }
    constexpr int BM = 64 * WM, BN = 16 * NTW * WN;
    CONV_KIND(PAM_CONV_KERNEL_IGEMM, BM * 1000 + BN);
    dim3 grid((a.M + BM - 1) / BM, a.Cout / BN);
    const size_t lds = (a.Kpad > KC ? 2 : 1) * (size_t)(BM + BN) * ROWB;
    pam_launch(k_conv_igemm<NTW, WM, WN, false>, grid, dim3(64 * WM * WN), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// the plan's (NTW, WM, WN) -> the instantiation (tile_cfg 0 .. 7 of pam_conv2d_nhwc_bf16_ex; 32-channel N tiles: 64- and 128-pixel blocks only)
template <int NTW>
static int launch_igemm_n(hipStream_t s, const ConvArgs& a, const ConvPlan& p) {
    switch (p.WM * 10 + p.WN) {
        case 11: return launch_conv<NTW, 1, 1>(s, a);
        case 21: return launch_conv<NTW, 2, 1>(s, a);
    }
    if constexpr (NTW != 2) switch (p.WM * 10 + p.WN) {
        case 12: return launch_conv<NTW, 1, 2>(s, a);
        case 22: return launch_conv<NTW, 2, 2>(s, a);
        case 41: return launch_conv<NTW, 4, 1>(s, a);
        case 13: return launch_conv<NTW, 1, 3>(s, a);     // all of a 144- / 192-channel layer per pixel tile: input staged once
        case 14: return launch_conv<NTW, 1, 4>(s, a);
        case 23: return launch_conv<NTW, 2, 3>(s, a);
    }
    return PAM_E_ARG;
}
int launch_igemm(hipStream_t s, const ConvArgs& a, const ConvPlan& p) {
    switch (p.ntw) {
        case 2: return launch_igemm_n<2>(s, a, p);
        case 3: return launch_igemm_n<3>(s, a, p);
        case 4: return launch_igemm_n<4>(s, a, p);
    }
    return PAM_E_ARG;
}
