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
template <int S, int NT>                                // S = stride (1: Darknet's first layer, 2: HRNet's), NT = Cout / 16 (2 or 4)
__global__ __launch_bounds__(256) void k_conv_stem(StemArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_id = blockIdx.x * 4 + wave;
    if (row_id >= a.N * a.Ho) return;
    const int n = row_id / a.Ho, oy = row_id - n * a.Ho;
    const int px = lane & 15, g = lane >> 4;
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((size_t)a.N * a.H * a.W * 16), 0x00020000);
    bf16x8 wf[NT][3];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) wf[j][ky] = *(const bf16x8*)(a.wfrag + ((size_t)(j * 3 + ky) * 64 + lane) * 8);
    f32x4 bias4[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bias4[j] = a.bias ? *(const f32x4*)(a.bias + g * 4 * NT + j * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    unsigned rowoff[3];                                  // byte offset of input row S*oy + ky - 1, or OOB
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = S * oy + ky - 1;
        rowoff[ky] = (iy >= 0 && iy < a.H && g < 3) ? (unsigned)((((size_t)n * a.H + iy) * a.W) * 16) : OOB_OFFSET;
    }
    const int ntiles = (a.Wo + 15) >> 4;
    auto load_tile = [&](int t, bf16x8* b) {
        const int ix = S * (t * 16 + px) + g - 1;
        const bool ok = ix >= 0 && ix < a.W;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
            b[ky] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_in, (ok && rowoff[ky] != OOB_OFFSET) ? rowoff[ky] + (unsigned)ix * 16u : OOB_OFFSET, 0, 0));
    };
    bf16x8 cur[3], nxt[3];
    load_tile(0, cur);
    uint16_t* orow = a.out + (((size_t)n * a.Ho + oy) * a.Wo) * (16 * NT) + g * 4 * NT;
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) load_tile(t + 1, nxt);
        f32x4 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = bias4[j];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[j][ky]), __builtin_bit_cast(bf16x8_t, cur[ky]), acc[j], 0, 0, 0);
        const int ox = t * 16 + px;
        if (ox < a.Wo) {
            uint32_t d[2 * NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = epi_act1(acc[j][r], a.relu & 3);
                d[2 * j] = pack_bf16x2_ew(v[0], v[1]); d[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
            }
            row_store<NT>(orow + (size_t)ox * (16 * NT), g, d);
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) cur[ky] = nxt[ky];
    }
}

template <int S, int NT>
static void launch_stem_one(hipStream_t s, const StemArgs& t) {
    CONV_KIND(PAM_CONV_KERNEL_STEM, S * 100 + 16 * NT);
    pam_launch(k_conv_stem<S, NT>, dim3((t.N * t.Ho + 3) / 4), dim3(256), 0, s, t);
}
int launch_stem(hipStream_t s, const ConvArgs& a, const void* wfrag) {
    StemArgs t;                                          // wfrag = the pre-permuted A fragments (see pam.h)
    t.in = a.in; t.wfrag = (const uint16_t*)wfrag; t.bias = a.bias; t.out = a.out;
    t.N = a.N; t.H = a.H; t.W = a.W; t.Ho = a.Ho; t.Wo = a.Wo; t.relu = a.relu;
    if (a.stride == 2 && a.Cout == 64) launch_stem_one<2, 4>(s, t);
    else if (a.stride == 2) launch_stem_one<2, 2>(s, t);
    else if (a.Cout == 64) launch_stem_one<1, 4>(s, t);
    else launch_stem_one<1, 2>(s, t);
    return hipGetLastError() == hipSuccess ? PAM_OK : PAM_E_HIP;
}
