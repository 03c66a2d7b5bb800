// libpam_hip.so, conv part of a1: the entry points of the HRNet / Darknet convolution stack.  pam_conv2d_nhwc_bf16_ex asks
// pam_conv_plan.hpp which kernel and instantiation a layer runs on and hands the launch to that family's source file:
//   pam_conv_igemm.hip  k_conv_igemm   the generic implicit GEMM            pam_conv_gs.hip    k_conv_gs    the streamed implicit GEMM
//   pam_conv3x3.hip     k_conv3x3      3x3 / stride 1, rows resident in LDS  pam_conv3x3s.hip   k_conv3x3s   the same with specialised waves
//   pam_conv_stem.hip   k_conv_stem    the 8-channel first layer
#include "pam_conv.hpp"

__thread int g_last_conv_kernel = 0;
__thread int g_last_conv_form = 0;
// profiling labels (bench.py's per-family roofline) and the tests' record of the tile choice: see CONV_KIND
extern "C" int pam_conv_last_kernel(void) { return g_last_conv_kernel; }
extern "C" int pam_conv_last_form(void) { return g_last_conv_form; }

// the weight-image layout queries (include/pam.h)
extern "C" int pam_conv3x3_slab(int H, int W, int Cin, int Cout) { return c3_slab(H, W, Cin, Cout); }
extern "C" int pam_conv3x3_layout_ex(int H, int W, int Cin, int Cout, int c96_slab) { return c3s_layout(H, W, Cin, Cout, c96_slab); }
extern "C" int pam_conv3x3_layout(int H, int W, int Cin, int Cout) { return c3s_layout(H, W, Cin, Cout, 0); }
extern "C" int pam_conv3x3_layout_gen(int H, int W, int Cin, int Cout) { return c3s_layout_gen(H, W, Cin, Cout); }
extern "C" int pam_conv3x3_layout_small(int H, int W, int Cin, int Cout) { return c3s_layout_small(H, W, Cin, Cout); }

// Diagnostic build only (make DIAG=1): the stamp buffer of k_conv3x3 / k_conv3x3s.  Kept in the ABI; only the diagnostic build records stamps.
#ifdef PAM_DIAG
static unsigned long long* g_c3_stamps = nullptr;
extern "C" int pam_conv_debug_stamps(void* dev_buf) { g_c3_stamps = (unsigned long long*)dev_buf; return PAM_OK; }
#else
extern "C" int pam_conv_debug_stamps(void*) { return PAM_E_ARG; }
#endif

static ConvQuery conv_query(bool in, bool w_packed, bool w_img, bool residual, bool out, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                            int stride, int pad, int relu, int tile_cfg, int in_cstride, int relu_from) {
    ConvQuery q;
    q.N = N; q.H = H; q.W = W; q.Cin = Cin; q.Cout = Cout; q.KH = KH; q.KW = KW; q.stride = stride; q.pad = pad; q.relu = relu;
    q.tile_cfg = tile_cfg; q.in_cstride = in_cstride; q.relu_from = relu_from;
    q.in = in; q.w_packed = w_packed; q.w_img = w_img; q.residual = residual; q.out = out;
    return q;
}

extern "C" int pam_conv_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu, int tile_cfg,
                             int in_cstride, int relu_from, int has_in, int has_w_packed, int has_w_img, int has_residual, int has_out,
                             int32_t* kernel, int32_t* form) {
    if (!kernel || !form) return PAM_E_ARG;
    const ConvPlan p = conv_plan(conv_query(has_in, has_w_packed, has_w_img, has_residual, has_out, N, H, W, Cin, Cout, KH, KW, stride, pad,
                                            relu, tile_cfg, in_cstride, relu_from));
    if (p.rc == PAM_OK) { *kernel = p.kernel; *form = p.form; }
    return p.rc;
}

extern "C" int pam_conv2d_nhwc_bf16_ex(void* stream, const void* in, const void* w_packed, const void* w_img, const float* bias,
                                       const void* residual, void* out, int N, int H, int W, int Cin, int Cout,
                                       int KH, int KW, int stride, int pad, int relu, int tile_cfg, int in_cstride, int relu_from) {
    const ConvPlan p = conv_plan(conv_query(in, w_packed, w_img, residual, out, N, H, W, Cin, Cout, KH, KW, stride, pad, relu, tile_cfg,
                                            in_cstride, relu_from));     // pointers as presence flags
    if (p.rc != PAM_OK) return p.rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.kernel == PAM_CONV_KERNEL_3X3 || p.kernel == PAM_CONV_KERNEL_3X3S) {          // rows in LDS: TH output rows per tile, weights from w_img
        C3Args c;
        c.in = (const uint16_t*)in; c.wimg = (const uint16_t*)w_img; c.bias = bias; c.res = (const uint16_t*)residual; c.out = (uint16_t*)out;
        c.N = N; c.H = H; c.W = W; c.Cout = Cout; c.TH = p.TH; c.tiles_y = (H + p.TH - 1) / p.TH; c.relu = relu; c.inv_pw = 1.0f / (float)(W + 2);
#ifdef PAM_DIAG
        c.stamps = g_c3_stamps; c.dbg = p.dbg | ((p.stamped && g_c3_stamps) ? 64 : 0);
#endif
        return p.kernel == PAM_CONV_KERNEL_3X3 ? launch_c3(s, c, p) : launch_c3s(s, c, p);
    }
    ConvArgs a;
    a.in = (const uint16_t*)in; a.w = (const uint16_t*)w_packed; a.bias = bias; a.res = (const uint16_t*)residual;
    a.out = (uint16_t*)out;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.relu = relu;
    a.in_cs = in_cstride > 0 ? in_cstride : Cin; a.relu_from = relu_from;
    a.Ho = (H + 2 * pad - KH) / stride + 1; a.Wo = (W + 2 * pad - KW) / stride + 1;
    a.Ktot = KH * KW * Cin; a.Kpad = (a.Ktot + KC - 1) / KC * KC; a.M = N * a.Ho * a.Wo;
    switch (p.kernel) {
        case PAM_CONV_KERNEL_STEM: return launch_stem(s, a, w_img);
        case PAM_CONV_KERNEL_GS: return launch_gs(s, a, p);
        case PAM_CONV_KERNEL_IGEMM: return launch_igemm(s, a, p);
    }
    return PAM_E_ARG;
}
extern "C" int pam_conv2d_nhwc_bf16(void* stream, const void* in, const void* w_packed, const void* w_img, const float* bias,
                                    const void* residual, void* out, int N, int H, int W, int Cin, int Cout,
                                    int KH, int KW, int stride, int pad, int relu, int tile_cfg) {
    return pam_conv2d_nhwc_bf16_ex(stream, in, w_packed, w_img, bias, residual, out, N, H, W, Cin, Cout, KH, KW, stride, pad, relu,
                                   tile_cfg, Cin, 0);
}
