// The text of k_conv_stem (csrc/pam_conv_stem.hip), compiled twice: as k_conv_stem (STEM_MISH 0: activation codes 0 / 1 / 2, the kernels
// every network launches, whose code this file must not change) and as k_conv_stem_mish (STEM_MISH 1: mish, code 3; YOLOv4's layer 0).
// The includer defines STEM_KERNEL and STEM_MISH.
template <int S, int NT>                                // S = stride (1: Darknet's first layer, 2: HRNet's), NT = Cout / 16 (2 or 4)
__global__ __launch_bounds__(256) void STEM_KERNEL(StemArgs a) {
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
#if STEM_MISH
                for (int r = 0; r < 4; ++r) v[r] = epi_mish(acc[j][r]);
#else
                for (int r = 0; r < 4; ++r) v[r] = epi_act1(acc[j][r], a.relu & 3);
#endif
                d[2 * j] = pack_bf16x2_ew(v[0], v[1]); d[2 * j + 1] = pack_bf16x2_ew(v[2], v[3]);
            }
            row_store<NT>(orow + (size_t)ox * (16 * NT), g, d);
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) cur[ky] = nxt[ky];
    }
}

