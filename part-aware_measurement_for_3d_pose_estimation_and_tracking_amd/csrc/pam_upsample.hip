// libpam_hip.so, conv stack: k_upsample_add, the HRNet fuse-layer sum  out = [ReLU](base + sum_t nearest_upsample(term_t))
// (also the detector's shortcut adds that no convolution absorbs).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

// out[n,y,x,c] = [relu](base[n,y,x,c] + sum_t term_t[n, y >> sh_t, x >> sh_t, c]); 8 channels (16 B) per thread
struct UpArgs { const uint16_t* base; const uint16_t* term[3]; int sh[3]; int tcs[3]; int nterms; uint16_t* out; int N, H, W, C, relu; };
__global__ __launch_bounds__(256) void k_upsample_add(UpArgs a) {
    const unsigned C8 = (unsigned)a.C >> 3, total = (unsigned)a.N * a.H * a.W * C8;       // host checks total < 2^31: 32-bit index math
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const unsigned pix = e / C8, c8 = e - pix * C8;
        const unsigned t2 = pix / (unsigned)a.W, x = pix - t2 * a.W;
        const unsigned n = t2 / (unsigned)a.H, y = t2 - n * a.H;
        const bf16x8 b = *(const bf16x8*)(a.base + (size_t)pix * a.C + c8 * 8);
        bf16x8 q[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {                   // all term loads issued together (independent addresses)
            q[t] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (t < a.nterms) {
                const unsigned hs = (unsigned)a.H >> a.sh[t], ws = (unsigned)a.W >> a.sh[t];
                q[t] = *(const bf16x8*)(a.term[t] + ((size_t)(n * hs + (y >> a.sh[t])) * ws + (x >> a.sh[t])) * a.tcs[t] + c8 * 8);
            }
        }
        float v[8];
        sum8_start(v, b);
#pragma unroll
        for (int t = 0; t < 3; ++t)                     // same summation order as before: base, then terms in order
            if (t < a.nterms) sum8_add(v, q[t]);
        bf16x8 o;
        sum8_finish(v, a.relu, o);
        *(bf16x8*)(a.out + (size_t)pix * a.C + c8 * 8) = o;
    }
}

extern "C" int pam_upsample_add_nhwc_bf16_ex(void* stream, const void* base, int n_terms, const void* const* terms,
                                             const int32_t* shifts, const int32_t* term_cstrides, void* out, int N, int H, int W, int C, int relu);
extern "C" int pam_upsample_add_nhwc_bf16(void* stream, const void* base, int n_terms, const void* const* terms,
                                          const int32_t* shifts, void* out, int N, int H, int W, int C, int relu) {
    return pam_upsample_add_nhwc_bf16_ex(stream, base, n_terms, terms, shifts, nullptr, out, N, H, W, C, relu);
}
extern "C" int pam_upsample_add_nhwc_bf16_ex(void* stream, const void* base, int n_terms, const void* const* terms,
                                             const int32_t* shifts, const int32_t* term_cstrides, void* out, int N, int H, int W, int C, int relu) {
    if (!base || !out || n_terms < 0 || n_terms > 3 || C % 8 != 0 || (size_t)N * H * W * (C / 8) >= (1ull << 31)) return PAM_E_ARG;
    UpArgs a;
    a.base = (const uint16_t*)base; a.out = (uint16_t*)out; a.nterms = n_terms;
    for (int t = 0; t < 3; ++t) {
        a.term[t] = t < n_terms ? (const uint16_t*)terms[t] : nullptr; a.sh[t] = t < n_terms ? shifts[t] : 0;
        a.tcs[t] = (t < n_terms && term_cstrides && term_cstrides[t] > 0) ? term_cstrides[t] : C;
        if (a.tcs[t] < C || a.tcs[t] % 8 != 0) return PAM_E_ARG;
    }
    a.N = N; a.H = H; a.W = W; a.C = C; a.relu = relu;
    const size_t total = (size_t)N * H * W * (C / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    pam_launch(k_upsample_add, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
