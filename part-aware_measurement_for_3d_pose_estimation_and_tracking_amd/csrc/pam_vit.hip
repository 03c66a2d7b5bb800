// Token kernels of the plain vision transformer (vitpose.py, hrnet_hip.HipViTPose): patch embedding, LayerNorm, linear layers
// (+ bias, + exact GELU or + residual) and multi-head attention over one crop's tokens.  A token tensor (M = B T rows of D channels,
// bf16) is the NHWC tensor (B, 16, 12, D), so the activation arena, k_deconv4x4s2 and the head pass read it as it stands.
//
// k_vit_gemm: out[m][n] = sum_k x[m][k] w[n][k] as v_mfma_f32_16x16x32_bf16 with the weights as the A operand (rows = output channels)
// and the tokens as the B operand (columns), so a lane ends with 16 contiguous output channels of one token (rows of an n-tile are
// permuted as in k_deconv4x4s2's image).  A wave owns MT token tiles x one 64-channel slab; a workgroup is 2 x 2 waves with no LDS and
// no barrier: the weight fragments are pre-packed per lane (packing.PackedLinear) and read as 16-byte global loads, a token's 32 K
// values of a k-step are four lanes' 16-byte pieces.  The next k-step's fragments are loaded while this one's MFMAs issue.
// PATCH form: the same loop over an implicit im2col of the crop kernel's (N, H, W, 8) output -- the patch embedding is packed for all 8
// channels of a pixel (a pixel IS one 16-byte B piece; picking the 3 real channels out would cost a shuffle per piece to save 0.2 of
// ViTPose-B's 17 GMAC).  K = (ky, kx, 8 channels), k-step c = (ky, kx = 4 (c & 3) + lane group); taps outside the crop are buffer
// loads beyond the range, which return zero.
//
// k_vit_layernorm: one wave per row, the row in registers as float32 (16-byte loads, up to 4 pieces a lane), the mean (rounded mean +
// the mean of the residues) and the variance of the centred values as wave reductions, one bf16 rounding at the store.
//
// k_vit_attention: one workgroup per (crop, head, strip of 64 queries), one wave per 16 queries.  K of the head sits in LDS row by row
// (pitch 72), V transposed (row = head channel in MFMA row order, column = key, pitch T' + 8).  S = K Q^T puts a query in a lane
// column and its keys 16 kt + 4 g + e in the four lanes g of that column: the row maximum and the sum are two xor-shuffles, every lane
// works on T / 4 scores.  The exponentials are rounded to bf16 straight into the B fragments of the P V product -- key order inside a
// k-step of 32 is (slot i of lane group g) = key 32 ks + 16 (i >> 2) + 4 g + (i & 3), which V's transposed image follows -- and the
// result is divided by the float32 sum of the unrounded exponentials.  The scores never leave registers.
// P goes into the product as TWO bf16 terms, the rounded exponential and the rounded remainder: one bf16 rounding has a relative error
// of up to 2^-8 (8 significant bits), twice the 2^-9 sum_j p_j |v_j| the kernel is held to, and rows that a few keys dominate reach it
// (measured with one term: 13 of 110592 elements outside that bound, by up to 1.15 x).  The second MFMA per fragment is 2 % of the
// network's work.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

struct VitGemmArgs {
    const uint16_t* x; const uint16_t* w; const float* bias; const uint16_t* res; uint16_t* out;
    int M, K, N, act;
    unsigned x_bytes;
    int H, W, T, TW;                     // PATCH: crop size, tokens per crop and per token row
};

template <int MT, bool PATCH>
__global__ __launch_bounds__(256) void k_vit_gemm(VitGemmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 2 + (wave & 1)) * (16 * MT);
    const int slab = blockIdx.y * 2 + (wave >> 1);
    if (m0 >= a.M || slab * 64 >= a.N) return;                                 // wave-uniform; the kernel has no barrier
    const int nk = a.K >> 5;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)a.x_bytes, 0x00020000);
    unsigned base[MT];
    int py0[MT], px0[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int tok = m0 + 16 * mt + col;
        if (PATCH) {
            const int n = tok / a.T, t = tok - n * a.T, ty = t / a.TW, tx = t - ty * a.TW;
            py0[mt] = tok < a.M ? 16 * ty - 2 : -(1 << 20);                    // a row outside every crop: all taps read zero
            px0[mt] = 16 * tx - 2 + g;
            base[mt] = (unsigned)n * (unsigned)a.H;
        } else {
            base[mt] = tok < a.M ? ((unsigned)tok * (unsigned)a.K + 8u * g) * 2u : OOB_OFFSET;
            py0[mt] = px0[mt] = 0;
        }
    }
    const uint16_t* wp = a.w + (size_t)slab * nk * 2048 + lane * 8;          // [slab][k-step][n-tile j][lane][8]
    auto load = [&](int c, bf16x8 (&af)[4], bf16x8 (&bf)[MT]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) af[j] = *(const bf16x8*)(wp + (size_t)(c * 4 + j) * 512);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            unsigned off;
            if (PATCH) {
                const int iy = py0[mt] + (c >> 2), ix = px0[mt] + 4 * (c & 3);
                const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                off = ok ? ((base[mt] + (unsigned)iy) * (unsigned)a.W + (unsigned)ix) * 16u : OOB_OFFSET;
            } else {
                off = base[mt] + 64u * (unsigned)c;
            }
            bf[mt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        }
    };
    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[mt][j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    auto mma = [&](const bf16x8 (&af)[4], const bf16x8 (&bf)[MT]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[j]), __builtin_bit_cast(bf16x8_t, bf[mt]),
                                                                     acc[mt][j], 0, 0, 0);
    };
    // Two sets of fragments in registers: the next k-step's loads are in flight while this one's MFMAs issue.  A ring of four steps
    // was measured and is slower: the loop is bound by the bytes its loads move through L1, not by their latency, and
    // the ring's registers cost a wave of occupancy.
    bf16x8 a0[4], b0[MT], a1[4], b1[MT];
    load(0, a0, b0);
    for (int c = 0; c < nk; c += 2) {                                          // K % 64 == 0: an even number of k-steps
        load(c + 1, a1, b1);
        mma(a0, b0);
        if (c + 2 < nk) load(c + 2, a0, b0);
        mma(a1, b1);
    }
    // epilogue: lane (col, g) of tile mt holds output channels 64 slab + 16 g .. + 15 of token m0 + 16 mt + col
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int tok = m0 + 16 * mt + col;
        if (tok >= a.M) continue;
        const int ch = 64 * slab + 16 * g;
        const float* bp = PATCH ? a.bias + (size_t)(tok % a.T) * a.N + ch : a.bias + ch;
        float v[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 b = *(const f32x4*)(bp + 4 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * j + e] = acc[mt][j][e] + b[e];
        }
        if (!PATCH && a.act == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678f));
        }
        uint16_t* o = a.out + (size_t)tok * a.N + ch;
        if (!PATCH && a.res != nullptr) {
            const uint16_t* r = a.res + (size_t)tok * a.N + ch;
            const bf16x8 r0 = *(const bf16x8*)r, r1 = *(const bf16x8*)(r + 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[e] += bf16_to_f32((uint16_t)r0[e]); v[8 + e] += bf16_to_f32((uint16_t)r1[e]); }
        }
        uint32_t d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = pack_bf16x2(v[2 * e], v[2 * e + 1]);
        *(u32x4*)o = (u32x4){d[0], d[1], d[2], d[3]};
        *(u32x4*)(o + 8) = (u32x4){d[4], d[5], d[6], d[7]};
    }
}

template <bool PATCH>
static int vit_gemm_launch(hipStream_t s, const VitGemmArgs& a) {
    const long long wg4 = (long long)((a.M + 127) / 128) * ((a.N + 127) / 128);
    const int gy = (a.N + 127) / 128;
    // MT = 4 from half a workgroup per CU on: at 20 crops it wins on every shape of -B, the 180-workgroup ones included;
    // a smaller grid takes the shorter workgroups.  Both forms give the same bits.
    if (2 * wg4 >= pam_cu_count()) pam_launch(k_vit_gemm<4, PATCH>, dim3((a.M + 127) / 128, gy), dim3(256), 0, s, a);
    else pam_launch(k_vit_gemm<2, PATCH>, dim3((a.M + 63) / 64, gy), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

extern "C" int pam_vit_linear_bf16(void* stream, const void* x, const void* w, const float* bias, const void* residual, void* out,
                                   int M, int K, int N, int act) {
    if (!x || !w || !bias || !out || M <= 0 || K <= 0 || N <= 0 || K % 64 != 0 || N % 64 != 0 || (act != 0 && act != 1) ||
        (residual && act != 0))
        return PAM_E_ARG;
    if ((size_t)M * K * 2 >= (1ull << 31) || (size_t)M * N * 2 >= (1ull << 31) || (N + 127) / 128 > 65535) return PAM_E_ARG;
    VitGemmArgs a = {};
    a.x = (const uint16_t*)x; a.w = (const uint16_t*)w; a.bias = bias; a.res = (const uint16_t*)residual; a.out = (uint16_t*)out;
    a.M = M; a.K = K; a.N = N; a.act = act; a.x_bytes = (unsigned)((size_t)M * K * 2);
    return vit_gemm_launch<false>((hipStream_t)stream, a);
}

extern "C" int pam_vit_patch_embed_bf16(void* stream, const void* x8, const void* w, const float* pos_bias, void* out, int N, int H, int W,
                                        int D) {
    if (!x8 || !w || !pos_bias || !out || N <= 0 || H <= 0 || W <= 0 || D <= 0 || H % 16 != 0 || W % 16 != 0 || D % 64 != 0) return PAM_E_ARG;
    const size_t T = (size_t)(H / 16) * (W / 16);
    if ((size_t)N * H * W * 16 >= (1ull << 31) || (size_t)N * T * D * 2 >= (1ull << 31) || (D + 127) / 128 > 65535) return PAM_E_ARG;
    VitGemmArgs a = {};
    a.x = (const uint16_t*)x8; a.w = (const uint16_t*)w; a.bias = pos_bias; a.res = nullptr; a.out = (uint16_t*)out;
    a.M = (int)(N * T); a.K = 2048; a.N = D; a.act = 0; a.x_bytes = (unsigned)((size_t)N * H * W * 16);
    a.H = H; a.W = W; a.T = (int)T; a.TW = W / 16;
    return vit_gemm_launch<true>((hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct VitLnArgs { const uint16_t* x; const float* gamma; const float* beta; uint16_t* out; int M, D; float eps; };

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(256) void k_vit_layernorm(VitLnArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= a.M) return;
    const int nch = a.D >> 3;                                                  // 16-byte pieces of a row: at most 256, four a lane
    const uint16_t* xr = a.x + (size_t)row * a.D;
    float v[4][8];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const bf16x8 t = *(const bf16x8*)(xr + 8 * ch);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = bf16_to_f32((uint16_t)t[e]); s += v[i][e]; }
        }
    }
    // the mean in two parts: a row of mean 100 and deviation 0.5 cannot hold its mean in ONE float32 to better than 4e-6, which is
    // 1e-5 deviations.  mean0 is the rounded mean, x - mean0 is exact for such rows (operands within a factor of two), and the mean of
    // those small residues is the correction; the variance is taken of the values centred by both.
    const float fd = (float)a.D;
    const float mean0 = wave_sum(s) / fd;
    float s1 = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] -= mean0; s1 += v[i][e]; }
        }
    const float mean1 = wave_sum(s1) / fd;
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] -= mean1; ss += v[i][e] * v[i][e]; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / fd + a.eps);
    uint16_t* orow = a.out + (size_t)row * a.D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const f32x4 g0 = *(const f32x4*)(a.gamma + 8 * ch), g1 = *(const f32x4*)(a.gamma + 8 * ch + 4);
            const f32x4 b0 = *(const f32x4*)(a.beta + 8 * ch), b1 = *(const f32x4*)(a.beta + 8 * ch + 4);
            float y[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { y[e] = v[i][e] * rstd * g0[e] + b0[e]; y[4 + e] = v[i][4 + e] * rstd * g1[e] + b1[e]; }
            *(u32x4*)(orow + 8 * ch) = (u32x4){pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7])};
        }
    }
}

extern "C" int pam_vit_layernorm_bf16(void* stream, const void* x, const float* gamma, const float* beta, void* out, int M, int D, float eps) {
    if (!x || !gamma || !beta || !out || M <= 0 || D <= 0 || D % 64 != 0 || D > 2048 || !(eps >= 0.0f)) return PAM_E_ARG;
    VitLnArgs a;
    a.x = (const uint16_t*)x; a.gamma = gamma; a.beta = beta; a.out = (uint16_t*)out; a.M = M; a.D = D; a.eps = eps;
    pam_launch(k_vit_layernorm, dim3((unsigned)(((long long)M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct VitAttnArgs { const uint16_t* qkv; uint16_t* out; int B, T, heads; };
constexpr int AT_KP = 72;                // K row pitch in LDS (64 + 8 bf16: 36 dwords, 16 rows of a fragment fall on distinct banks)
constexpr int AT_KT = 12;                // key tiles of 16: T <= 192

// LDS row of head channel d in V's transposed image: n-tile dt = (d >> 2) & 3 holds row 4 (d >> 4) + (d & 3), so a lane of the P V
// product ends with channels 16 g .. 16 g + 15;  column of key k: the k-step's slot order of the P fragments (see the head of the file)
__device__ __forceinline__ int at_vrow(int d) { return 16 * ((d >> 2) & 3) + 4 * (d >> 4) + (d & 3); }
__device__ __forceinline__ int at_vcol(int k) { return (k & ~31) + 8 * ((k >> 2) & 3) + 4 * ((k >> 4) & 1) + (k & 3); }

__global__ __launch_bounds__(256) void k_vit_attention(VitAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t at_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
    const int T = a.T, KT = T >> 4, KS = (KT + 1) >> 1, TP = 32 * KS, VP = TP + 8;
    uint16_t* Ks = at_lds;                                                     // [T keys][AT_KP]
    uint16_t* Vt = at_lds + T * AT_KP;                                         // [64 rows][VP]
    const int b = blockIdx.z, h = blockIdx.y;
    const size_t tok_stride = (size_t)3 * a.heads * 64;
    const uint16_t* base = a.qkv + (size_t)b * T * tok_stride + (size_t)h * 64;
    for (int idx = tid; idx < T * 8; idx += 256) {
        const int key = idx >> 3, p = idx & 7;
        const uint16_t* src = base + (size_t)key * tok_stride + 8 * p;
        *(bf16x8*)(Ks + key * AT_KP + 8 * p) = *(const bf16x8*)(src + (size_t)a.heads * 64);
        const bf16x8 v = *(const bf16x8*)(src + (size_t)2 * a.heads * 64);
        const int kc = at_vcol(key);
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[at_vrow(8 * p + e) * VP + kc] = (uint16_t)v[e];
    }
    for (int idx = tid; idx < (TP - T) * 64; idx += 256)                      // an odd number of key tiles: the last k-step's other half is zero
        Vt[at_vrow(idx & 63) * VP + at_vcol(T + (idx >> 6))] = 0;
    __syncthreads();
    const int qt = blockIdx.x * 4 + wave;
    if (qt >= KT) return;
    const int qrow = 16 * qt + col;
    bf16x8 bq[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) bq[c] = *(const bf16x8*)(base + (size_t)qrow * tok_stride + 32 * c + 8 * g);
    f32x4 s[AT_KT];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int kt = 0; kt < AT_KT; ++kt) {
        s[kt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        if (kt < KT) {                                                         // wave-uniform
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bf16x8 ak = *(const bf16x8*)(Ks + (16 * kt + col) * AT_KP + 32 * c + 8 * g);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ak), __builtin_bit_cast(bf16x8_t, bq[c]), s[kt], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[kt][e] *= 0.125f; mx = fmaxf(mx, s[kt][e]); }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < AT_KT; ++kt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float p = kt < KT ? expf(s[kt][e] - mx) : 0.0f;
            s[kt][e] = p;
            sum += p;
        }
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < AT_KT / 2; ++ks) {
        if (ks < KS) {                                                         // wave-uniform
            const u32x4 pd = (u32x4){pack_bf16x2(s[2 * ks][0], s[2 * ks][1]), pack_bf16x2(s[2 * ks][2], s[2 * ks][3]),
                                     pack_bf16x2(s[2 * ks + 1][0], s[2 * ks + 1][1]), pack_bf16x2(s[2 * ks + 1][2], s[2 * ks + 1][3])};
            // what the rounding dropped (exact in float32), rounded to bf16 in its turn: the second term of P
            u32x4 pl;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                pl[i] = pack_bf16x2(s[2 * ks + (i >> 1)][2 * (i & 1)] - bf16_lo(pd[i]), s[2 * ks + (i >> 1)][2 * (i & 1) + 1] - bf16_hi(pd[i]));
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 av = *(const bf16x8*)(Vt + (16 * dt + col) * VP + 32 * ks + 8 * g);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, pd), o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, pl), o[dt], 0, 0, 0);
            }
        }
    }
    uint32_t d[8];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        d[2 * dt] = pack_bf16x2(o[dt][0] / sum, o[dt][1] / sum);
        d[2 * dt + 1] = pack_bf16x2(o[dt][2] / sum, o[dt][3] / sum);
    }
    uint16_t* op = a.out + ((size_t)((size_t)b * T + qrow) * a.heads + h) * 64 + 16 * g;
    *(u32x4*)op = (u32x4){d[0], d[1], d[2], d[3]};
    *(u32x4*)(op + 8) = (u32x4){d[4], d[5], d[6], d[7]};
}

extern "C" int pam_vit_attention_bf16(void* stream, const void* qkv, void* out, int B, int T, int heads) {
    if (!qkv || !out || B <= 0 || heads <= 0 || T < 16 || T > 16 * AT_KT || T % 16 != 0 || B > 65535 || heads > 65535) return PAM_E_ARG;
    VitAttnArgs a;
    a.qkv = (const uint16_t*)qkv; a.out = (uint16_t*)out; a.B = B; a.T = T; a.heads = heads;
    const int KT = T / 16, TP = 32 * ((KT + 1) / 2);
    const int lds = (T * AT_KP + 64 * (TP + 8)) * 2;
    constexpr int lds_max = (16 * AT_KT * AT_KP + 64 * (16 * AT_KT + 8)) * 2;  // the attribute is set once per device: for the largest T
    if (!pam_max_dynamic_lds((const void*)k_vit_attention, lds_max)) return PAM_E_HIP;
    pam_launch(k_vit_attention, dim3((KT + 3) / 4, heads, B), dim3(256), lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
