// libpam_hip.so, conv stack
// ====================================================================================================================
// k_conv_gs: the implicit GEMM (1x1 and strided 3x3 layers) with the wave roles of k_conv3x3s.  Waves 4-7 gather the im2col tile
// -- 256 output pixels x 64 K values per chunk, every 16-byte piece fetched from its own address (or from a page of zeros: padding,
// K tail, rows past M) -- and the slab's weight rows straight from the packed [Cout][Kpad] matrix, by LDS-DMA into a ring of NBUF chunk
// buffers; waves 0-3 read fragments and multiply (64 pixels x 16*NTW channels each).  Rows are dense 128 bytes with the 16-byte
// piece q of row r at position q ^ ((r >> 1) & 7): conflict-free ds_read_b128 for a 16-row window x 4 k-groups, and a lane's
// fragment addresses are constants + immediates.  One s_barrier per chunk (loaders: chunk k has landed; multipliers: chunk k - 1 is
// consumed), residual folded into the bias before the K loop, epilogue = convert + ReLU (channels >= relu_from) + 16-byte stores.
// ====================================================================================================================
#include "pam_conv.hpp"

#define GS_KERNEL k_conv_gs
#define GS_MISH 0
#include "pam_conv_gs_kernel.inc"
#undef GS_KERNEL
#undef GS_MISH
#define GS_KERNEL k_conv_gs_mish
#define GS_MISH 1
#include "pam_conv_gs_kernel.inc"
#undef GS_KERNEL
#undef GS_MISH

// the mish forms: 64-channel slabs, ring of 3, no residual (a mish layer's shortcut is added after the activation, by the GEN kernels)
template <int BM>
static int launch_conv_gs_mish(hipStream_t s, const ConvArgs& a) {
    constexpr int NTW = 4, NBUF = 3;
    constexpr size_t lds = (size_t)NBUF * (BM + 16 * NTW) * 128;
    if (!pam_max_dynamic_lds((const void*)k_conv_gs_mish<NTW, NBUF, false, BM>, (int)lds)) return PAM_E_HIP;
    CONV_KIND(PAM_CONV_KERNEL_GS, NBUF * 1000000 + BM * 1000 + 500 + 16 * NTW);
    const int ntile = ((a.M + BM - 1) / BM) * (a.Cout / (16 * NTW));
    pam_launch(k_conv_gs_mish<NTW, NBUF, false, BM>, dim3(ntile < 256 ? ntile : 256), dim3(512), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
template <int NTW, bool RES, int BM = 256, int NBUF = 3>
static int launch_conv_gs_r(hipStream_t s, const ConvArgs& a) {
    constexpr size_t lds = (size_t)NBUF * (BM + 16 * NTW) * 128;
    static_assert(lds <= 160 * 1024, "LDS");
    if (!pam_max_dynamic_lds((const void*)k_conv_gs<NTW, NBUF, RES, BM>, (int)lds)) return PAM_E_HIP;
    CONV_KIND(PAM_CONV_KERNEL_GS, NBUF * 1000000 + BM * 1000 + 16 * NTW);
    const int ntile = ((a.M + BM - 1) / BM) * (a.Cout / (16 * NTW));
    pam_launch(k_conv_gs<NTW, NBUF, RES, BM>, dim3(ntile < 256 ? ntile : 256), dim3(512), lds, s, a);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
// the plan's (slab, pixel tile, ring depth, residual) -> the instantiation
int launch_gs(hipStream_t s, const ConvArgs& a, const ConvPlan& p) {
    if (p.mish) {                                          // the forms plan_gs hands a code-3 layer
        if (p.res || p.ntw != 4 || p.NBUF != 3) return PAM_E_ARG;
        switch (p.BM) {
            case 64: return launch_conv_gs_mish<64>(s, a);
            case 128: return launch_conv_gs_mish<128>(s, a);
            case 256: return launch_conv_gs_mish<256>(s, a);
        }
        return PAM_E_ARG;
    }
    switch (p.ntw * 10000 + p.BM * 10 + p.NBUF) {
        case 32563: return p.res ? launch_conv_gs_r<3, true>(s, a) : launch_conv_gs_r<3, false>(s, a);
        case 42563: return p.res ? launch_conv_gs_r<4, true>(s, a) : launch_conv_gs_r<4, false>(s, a);
        case 62563: return p.res ? PAM_E_ARG : launch_conv_gs_r<6, false>(s, a);    // the wide slab has no registers left for the residual rows
    }
    if (p.res) return PAM_E_ARG;
    switch (p.ntw * 10000 + p.BM * 10 + p.NBUF) {
        case 30643: return launch_conv_gs_r<3, false, 64, 3>(s, a);
        case 31283: return launch_conv_gs_r<3, false, 128, 3>(s, a);
        case 31285: return launch_conv_gs_r<3, false, 128, 5>(s, a);
        case 40643: return launch_conv_gs_r<4, false, 64, 3>(s, a);
        case 41283: return launch_conv_gs_r<4, false, 128, 3>(s, a);
    }
    return PAM_E_ARG;
}
