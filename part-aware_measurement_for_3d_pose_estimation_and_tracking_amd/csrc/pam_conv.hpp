// Private to the convolution sources (pam_conv.hip and one pam_conv_*.hip per kernel family): the argument structs, the record of
// what was launched, the family launchers' prototypes and the device helpers more than one family uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/pam.h"
#include "pam_kernel.hpp"
#include "pam_conv_plan.hpp"

struct ConvArgs {
    const uint16_t* in; const uint16_t* w; const float* bias; const uint16_t* res; uint16_t* out;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, relu, Ktot, Kpad, M;
    int in_cs;        // channel stride of the input pixels (= Cin unless the input is a channel slice of a wider tensor)
    int relu_from;    // the activation applies to output channels >= relu_from (0 = all); multiple of 16
};

// k_conv3x3 / k_conv3x3s
struct C3Args {
    const uint16_t* in; const uint16_t* wimg; const float* bias; const uint16_t* res; uint16_t* out;
    int N, H, W, Cout, TH, tiles_y, relu;
    float inv_pw;
#ifdef PAM_DIAG
    int dbg;                         // phase knock-outs / stamps for tools/stamp_conv.py
    unsigned long long* stamps;      // (dbg & 64): per-workgroup s_memtime stamps, never read by the kernel
#endif
};
// Diagnostic build only (make DIAG=1): phase knock-outs, in-kernel stamps and environment tuning overrides.  The shipped library is
// compiled without them -- C3_DBG folds to false, C3_STAMP to nothing, no getenv on the launch path.
#ifdef PAM_DIAG
#define C3_DBG(bit) (a.dbg & (bit))
#define C3_STAMP(k) do { if ((a.dbg & 64) && tid == 0) a.stamps[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define C3_DBG(bit) false
#define C3_STAMP(k) do { } while (0)
#endif

// which kernel (PAM_CONV_KERNEL_*) and which instantiation of it (the form: include/pam.h) the calling thread's last
// pam_conv2d_nhwc_bf16[_ex] call launched.  Both are recorded by ONE statement inside each launcher, from the template parameters of
// the kernel it launches, so the two cannot disagree with each other or with the launch (profiling labels, tests of the tile choice).
// Defined in pam_conv.hip.
extern __thread int g_last_conv_kernel;
extern __thread int g_last_conv_form;
#define CONV_KIND(k, form) (g_last_conv_kernel = (k), g_last_conv_form = (form))

// One launcher per family: maps the plan's parameters to the instantiation, records CONV_KIND from its template parameters, launches.
int launch_igemm(hipStream_t s, const ConvArgs& a, const ConvPlan& p);          // pam_conv_igemm.hip
int launch_gs(hipStream_t s, const ConvArgs& a, const ConvPlan& p);             // pam_conv_gs.hip
int launch_stem(hipStream_t s, const ConvArgs& a, const void* wfrag);           // pam_conv_stem.hip
int launch_c3(hipStream_t s, const C3Args& a, const ConvPlan& p);               // pam_conv3x3.hip
int launch_c3s(hipStream_t s, const C3Args& a, const ConvPlan& p);              // pam_conv3x3s.hip

// fused epilogue activation.  act & 3: 0 linear, 1 ReLU, 2 leaky ReLU (slope 0.1); act & 4: the residual is added AFTER the
// activation (Darknet shortcut layers) instead of before it (ResNet / HRNet blocks)
__device__ __forceinline__ float epi_act1(float v, int kind) {
    return kind == 1 ? fmaxf(v, 0.0f) : (kind == 2 ? (v > 0.0f ? v : 0.1f * v) : v);
}
__device__ __forceinline__ float epi_act(float v, float r, int act) {
    return (act & 4) ? epi_act1(v, act & 3) + r : epi_act1(v + r, act & 3);
}

// Code 3 of act & 3: mish, x * tanh(softplus(x)), in the division form of Darknet's GPU code (no log, no tanh; finite for every finite x:
// e = inf gives x, e = 0 gives -0; within 3 float32 ulp of the float64 value).  Only the Darknet-only instantiations carry it -- the
// general-activation (GEN) forms of k_conv_igemm / k_conv3x3s and the mish forms of k_conv_stem / k_conv_gs --, through epi_act_gen;
// epi_act1 / epi_act above, which the pose networks' instantiations compile, never see code 3.
__device__ __forceinline__ float epi_mish(float x) {
    const float e = expf(x), n = e * e + 2.0f * e;
    return x <= -0.6f ? x * (n / (n + 2.0f)) : x - 2.0f * (x / (n + 2.0f));
}
__device__ __forceinline__ float epi_act1_gen(float v, int kind) { return kind == 3 ? epi_mish(v) : epi_act1(v, kind); }
__device__ __forceinline__ float epi_act_gen(float v, float r, int act) {
    return (act & 4) ? epi_act1_gen(v, act & 3) + r : epi_act1_gen(v + r, act & 3);
}

// the element-wise pack (two converts + a permute); the shared pack_bf16x2 changes these kernels' code and is left to a measured change
__device__ __forceinline__ uint32_t pack_bf16x2_ew(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

// One lane's row piece of 4*NTW contiguous bf16 channels (8*NTW bytes at byte offset o, 8-byte aligned; 16-byte aligned
// when NTW is even or the lane group g is even) as 16-byte accesses where possible.  NTW = 3 (24 bytes) splits 16 + 8 for
// even g and 8 + 16 for odd g, so the 16-byte half is always aligned.
template <int NTW>
__device__ __forceinline__ void c3_row_load(__amdgpu_buffer_rsrc_t rs, unsigned o, int g, uint32_t* d) {
    if constexpr (NTW == 1) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, o, 0, 0); d[0] = v[0]; d[1] = v[1];
    } else if constexpr (NTW == 2) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0); d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    } else if constexpr (NTW == 4) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0), w = __builtin_amdgcn_raw_buffer_load_b128(rs, o + 16, 0, 0);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3]; d[4] = w[0]; d[5] = w[1]; d[6] = w[2]; d[7] = w[3];
    } else if constexpr (NTW == 6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o + 16 * k, 0, 0);
            d[4 * k] = v[0]; d[4 * k + 1] = v[1]; d[4 * k + 2] = v[2]; d[4 * k + 3] = v[3];
        }
    } else {
        static_assert(NTW == 3, "slab width");
        const bool odd = g & 1;
        const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(rs, o + (odd ? 8u : 0u), 0, 0);
        const u32x2 h = __builtin_amdgcn_raw_buffer_load_b64(rs, o + (odd ? 0u : 16u), 0, 0);
        d[0] = odd ? h[0] : q[0]; d[1] = odd ? h[1] : q[1]; d[2] = odd ? q[0] : q[2];
        d[3] = odd ? q[1] : q[3]; d[4] = odd ? q[2] : h[0]; d[5] = odd ? q[3] : h[1];
    }
}

// a page of zeros for the LDS-DMA loaders of k_conv3x3s and k_conv_gs (rows outside the image, K tail, rows past M): 64 B + the largest
// chunk offset (Cin = 512); one copy per source file that reads it
__device__ __attribute__((aligned(64))) const uint32_t g_c3_zero[16 + 16 * 16] = {0};
