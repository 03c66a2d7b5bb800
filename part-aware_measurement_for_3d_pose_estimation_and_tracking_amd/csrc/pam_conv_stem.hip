// libpam_hip.so, conv stack
// ====================================================================================================================
// k_conv_stem: the first convolution of both networks' stems -- 3x3 / stride 1 or 2 / pad 1 from the 8-channel (RGB + zeros)
// input to 32 or 64 channels.  K per tap ROW is 3 taps x 8 channels = 24 <= 32, so one v_mfma_f32_16x16x32_bf16 covers a whole tap row:
// lane (pixel l & 15, k-group g = l >> 4) supplies as its B fragment the 16-byte input pixel (2y + ky - 1, 2x + g - 1)
// straight from global memory (g = 3 and the zero padding come from the buffer bounds check), 3 loads and 12 MFMAs per
// 16 output pixels x 64 channels.  The weights (A operand, 12 fragments) live in registers for the wave's whole row; their
// rows are permuted like k_conv3x3's so a lane ends with 16 contiguous channels: each pixel's 128 output bytes are written
// by 4 lanes x 2 x 16 B.  Pure streaming: ~35 MB in, ~71 MB out at 20 crops.  One wave per output row.
// ====================================================================================================================
#include "pam_conv.hpp"

struct StemArgs { const uint16_t* in; const uint16_t* wfrag; const float* bias; uint16_t* out; int N, H, W, Ho, Wo, relu; };
#define STEM_KERNEL k_conv_stem
#define STEM_MISH 0
#include "pam_conv_stem_kernel.inc"
#undef STEM_KERNEL
#undef STEM_MISH
#define STEM_KERNEL k_conv_stem_mish
#define STEM_MISH 1
#include "pam_conv_stem_kernel.inc"
#undef STEM_KERNEL
#undef STEM_MISH

template <int S, int NT>
static void launch_stem_one(hipStream_t s, const StemArgs& t) {
    CONV_KIND(PAM_CONV_KERNEL_STEM, S * 100 + 16 * NT);
    pam_launch(k_conv_stem<S, NT>, dim3((t.N * t.Ho + 3) / 4), dim3(256), 0, s, t);
}
template <int NT>                                       // YOLOv4's layer 0 (3 -> 32, stride 1): the mish form, stride 1 only
static void launch_stem_mish(hipStream_t s, const StemArgs& t) {
    CONV_KIND(PAM_CONV_KERNEL_STEM, 1000 + 100 + 16 * NT);
    pam_launch(k_conv_stem_mish<1, NT>, dim3((t.N * t.Ho + 3) / 4), dim3(256), 0, s, t);
}
int launch_stem(hipStream_t s, const ConvArgs& a, const void* wfrag) {
    StemArgs t;                                          // wfrag = the pre-permuted A fragments (see pam.h)
    t.in = a.in; t.wfrag = (const uint16_t*)wfrag; t.bias = a.bias; t.out = a.out;
    t.N = a.N; t.H = a.H; t.W = a.W; t.Ho = a.Ho; t.Wo = a.Wo; t.relu = a.relu;
    if ((a.relu & 3) == 3) {
        if (a.stride != 1) return PAM_E_ARG;
        if (a.Cout == 64) launch_stem_mish<4>(s, t); else launch_stem_mish<2>(s, t);
    } else if (a.stride == 2 && a.Cout == 64) launch_stem_one<2, 4>(s, t);
    else if (a.stride == 2) launch_stem_one<2, 2>(s, t);
    else if (a.Cout == 64) launch_stem_one<1, 4>(s, t);
    else launch_stem_one<1, 2>(s, t);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
