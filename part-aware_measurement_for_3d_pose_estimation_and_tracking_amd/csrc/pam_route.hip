// libpam_hip.so, person-detector side: Darknet's general `[route]` as one launch (YOLOv4 / YOLOv4-tiny; the contract is in include/pam.h).
// ====================================================================================================================
// k_route: out[n, y, x, :] = the channel slices of up to four source layers side by side, then +0 up to the output's padded channel
// count.  A slice is `count` channels from channel `offset` of a source whose pixels are `cstride` channels apart (a group route, or the
// real channels of a channel-padded layer); a source flagged "nearest x2" is an (H/2, W/2) map read at (y/2, x/2).  A pure copy: one
// 16-byte piece (8 channels) per lane and step, consecutive lanes along the channels of a pixel and on into the next pixel, so a
// wave stores 1 KiB of consecutive output bytes and loads runs of whole slices; a grid-stride loop sized from the output, no LDS.  The
// piece index is 32-bit (three unsigned divisions per piece at most, where the 64-bit ones of a size_t index would cost more than the
// copy); byte offsets are size_t.
// ====================================================================================================================
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pam.h"
#include "pam_kernel.hpp"

struct RouteArgs {
    const uint16_t* src[PAM_ROUTE_MAX_SRC];
    int cs[PAM_ROUTE_MAX_SRC], off[PAM_ROUTE_MAX_SRC], up[PAM_ROUTE_MAX_SRC];
    int end8[PAM_ROUTE_MAX_SRC];     // where source k's slice ends in the output, in 8-channel pieces (sources past n_src: real8)
    uint16_t* out;
    int H, W, C8, real8, any_up;
    unsigned total;                  // N * H * W * C8 pieces, < 2^31
};

__global__ __launch_bounds__(256) void k_route(RouteArgs a) {
    const unsigned step = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < a.total; i += step) {
        const unsigned p = i / (unsigned)a.C8;
        const int c8 = (int)(i - p * (unsigned)a.C8);
        u32x4 v = {0u, 0u, 0u, 0u};                     // the padded tail: +0
        if (c8 < a.real8) {
            // which slice: selects, not indexed reads of the argument struct
            const int k = (c8 >= a.end8[0]) + (c8 >= a.end8[1]) + (c8 >= a.end8[2]);
            const int first8 = k == 0 ? 0 : (k == 1 ? a.end8[0] : (k == 2 ? a.end8[1] : a.end8[2]));
            const uint16_t* sp = k == 0 ? a.src[0] : (k == 1 ? a.src[1] : (k == 2 ? a.src[2] : a.src[3]));
            const int cs = k == 0 ? a.cs[0] : (k == 1 ? a.cs[1] : (k == 2 ? a.cs[2] : a.cs[3]));
            const int off = k == 0 ? a.off[0] : (k == 1 ? a.off[1] : (k == 2 ? a.off[2] : a.off[3]));
            size_t pix = p;
            if (a.any_up) {                             // uniform
                const int up = k == 0 ? a.up[0] : (k == 1 ? a.up[1] : (k == 2 ? a.up[2] : a.up[3]));
                if (up) {
                    const unsigned q = p / (unsigned)a.W, x = p - q * (unsigned)a.W;
                    const unsigned n = q / (unsigned)a.H, y = q - n * (unsigned)a.H;
                    pix = ((size_t)n * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1);
                }
            }
            v = *(const u32x4*)(sp + pix * (size_t)cs + off + (c8 - first8) * 8);
        }
        *(u32x4*)(a.out + (size_t)i * 8) = v;
    }
}

extern "C" int pam_route_concat_nhwc_bf16(void* stream, int n_src, const void* const* src, const int32_t* src_cstride, const int32_t* src_offset,
                                          const int32_t* src_count, const int32_t* src_up2, void* out, int N, int H, int W, int C_out) {
    if (n_src < 1 || n_src > PAM_ROUTE_MAX_SRC || !src || !src_cstride || !src_offset || !src_count || !src_up2 || !out || ((uintptr_t)out & 15) ||
        N <= 0 || H <= 0 || W <= 0 || C_out <= 0 || C_out % 8 != 0)
        return PAM_E_ARG;
    RouteArgs a = {};
    long long real = 0;
    for (int k = 0; k < n_src; ++k) {
        if (!src[k] || ((uintptr_t)src[k] & 15) || src_cstride[k] <= 0 || src_cstride[k] % 8 != 0 || src_offset[k] < 0 || src_offset[k] % 8 != 0 ||
            src_count[k] <= 0 || src_count[k] % 8 != 0 || (long long)src_offset[k] + src_count[k] > src_cstride[k])
            return PAM_E_ARG;                           // a slice that is no whole number of 16-byte pieces, or leaves its source
        if (src_up2[k] && ((H & 1) || (W & 1))) return PAM_E_ARG;
        real += src_count[k];
        if (real > C_out) return PAM_E_ARG;             // the padded output count is smaller than the real one
        a.src[k] = (const uint16_t*)src[k]; a.cs[k] = src_cstride[k]; a.off[k] = src_offset[k]; a.up[k] = src_up2[k] ? 1 : 0;
        a.end8[k] = (int)(real / 8);
        a.any_up |= a.up[k];
    }
    for (int k = n_src; k < PAM_ROUTE_MAX_SRC; ++k) a.end8[k] = (int)(real / 8);
    const unsigned long long total = (unsigned long long)N * H * W * (C_out / 8);
    if (total >= (1ull << 31)) return PAM_E_ARG;        // the piece index is 32-bit
    a.out = (uint16_t*)out; a.H = H; a.W = W; a.C8 = C_out / 8; a.real8 = (int)(real / 8); a.total = (unsigned)total;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(k_route, dim3(blocks < 2048u ? blocks : 2048u), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
