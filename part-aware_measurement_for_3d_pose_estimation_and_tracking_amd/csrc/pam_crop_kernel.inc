// The crop kernel's text, included once per form by pam_image.hip with CROP_KERNEL (the kernel's name) and CROP_FLIP defined.
// CROP_FLIP 0: k_preprocess_crops, rows n_src .. (grid) repeat row n_src - 1.
// CROP_FLIP 1: the crops of one flip-test forward in one buffer -- rows [0, n_src) plain, rows [n_src, 2 n_src) the column reversal of
// row r - n_src, rows from 2 n_src on repeat row 2 n_src - 1 (bucket padding).  A mirrored row is the SAME sample stored at column
// ow - 1 - ox (the official input.flip(3)): bit-equal to the reversal of the plain row on both resize paths, never a resample of a
// mirrored box.  One text for both forms keeps the plain form's instructions what they were and the float operations the same.
__global__ __launch_bounds__(256) void CROP_KERNEL(int n_src, const uint8_t* const* __restrict__ frames, int H, int W,
                                                          const int* __restrict__ view_of, const float* __restrict__ boxes,
                                                          int oh, int ow, int oc, uint16_t* __restrict__ out, int antialias) {
#if CROP_FLIP
    const int crop = blockIdx.y, mirror = crop >= n_src, src = min(mirror ? crop - n_src : crop, n_src - 1);
#else
    const int crop = blockIdx.y, src = min(crop, n_src - 1);
#endif
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= oh * ow) return;
    const int oy = px / ow, ox = px % ow;
    const uint8_t* __restrict__ img = frames[view_of[src]];
    const float bx = boxes[src * 4 + 0], by = boxes[src * 4 + 1], bw = boxes[src * 4 + 2], bh = boxes[src * 4 + 3];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, istd[3] = {1.0f / 0.229f, 1.0f / 0.224f, 1.0f / 0.225f};
    uint16_t o[3];
    if (!antialias) {
        float sx = bx + (ox + 0.5f) * (bw / (float)ow) - 0.5f;
        float sy = by + (oy + 0.5f) * (bh / (float)oh) - 0.5f;
        sx = fminf(fmaxf(sx, 0.0f), (float)(W - 1));
        sy = fminf(fmaxf(sy, 0.0f), (float)(H - 1));
        const int x0 = (int)sx, y0 = (int)sy;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float fx = sx - (float)x0, fy = sy - (float)y0;
        const uint8_t* r0 = img + ((size_t)y0 * W) * 3;
        const uint8_t* r1 = img + ((size_t)y1 * W) * 3;
        // the two pixels of a row are 6 consecutive bytes: ONE unaligned 8-byte load per row instead of six byte loads (the kernel was bound by
        // the texture-address unit: 12 one-byte gathers per output pixel); not for the last two columns (x1 is clamped there / the load would
        // leave the row)
        uint8_t t0[6], t1[6];
        if (x0 + 2 < W) {
            struct __attribute__((packed)) U8 { uint32_t x, y; };              // alignment 1: the backend emits one dwordx2 load (unaligned access is on)
            const U8 q0 = *(const U8*)(r0 + x0 * 3), q1 = *(const U8*)(r1 + x0 * 3);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                t0[k] = (uint8_t)((k < 4 ? q0.x >> (8 * k) : q0.y >> (8 * (k - 4))) & 0xff);
                t1[k] = (uint8_t)((k < 4 ? q1.x >> (8 * k) : q1.y >> (8 * (k - 4))) & 0xff);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { t0[k] = r0[x0 * 3 + k]; t0[3 + k] = r0[x1 * 3 + k]; t1[k] = r1[x0 * 3 + k]; t1[3 + k] = r1[x1 * 3 + k]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {          // c indexes RGB; source is BGR
            const int sc = 2 - c;
            const float a = (float)t0[sc], b = (float)t0[3 + sc];
            const float cc = (float)t1[sc], d = (float)t1[3 + sc];
            const float top = a + (b - a) * fx, bot = cc + (d - cc) * fx;
            const float v = (top + (bot - top) * fy) * (1.0f / 255.0f);
            o[c] = f32_to_bf16((v - mean[c]) * istd[c]);
        }
    } else {
        const float scx = bw / (float)ow, scy = bh / (float)oh, supx = fmaxf(scx, 1.0f), supy = fmaxf(scy, 1.0f);
        const float cx = bx + (ox + 0.5f) * scx, cy = by + (oy + 0.5f) * scy;
        // (a box wholly right of / below the frame: the window is the last column / row, whose weight is 0 there -- a black pixel, never a read past the frame)
        const int xlo = min(max(0, (int)floorf(bx)), W - 1), xhi = max(xlo + 1, min(W, (int)ceilf(bx + bw)));
        const int ylo = min(max(0, (int)floorf(by)), H - 1), yhi = max(ylo + 1, min(H, (int)ceilf(by + bh)));
        int x0 = max(xlo, (int)(cx - supx + 0.5f)), x1 = min(xhi, (int)(cx + supx + 0.5f));
        int y0 = max(ylo, (int)(cy - supy + 0.5f)), y1 = min(yhi, (int)(cy + supy + 0.5f));
        if (x1 <= x0) { x0 = min(max((int)cx, xlo), xhi - 1); x1 = x0 + 1; }
        if (y1 <= y0) { y0 = min(max((int)cy, ylo), yhi - 1); y1 = y0 + 1; }
        // beyond the limit the window is cut to the AA_MAXT taps nearest the centre (symmetric: no shift of the sampled position)
        if (x1 - x0 > AA_MAXT) { x0 = min(max((int)floorf(cx - 0.5f * AA_MAXT + 0.5f), x0), x1 - AA_MAXT); x1 = x0 + AA_MAXT; }
        if (y1 - y0 > AA_MAXT) { y0 = min(max((int)floorf(cy - 0.5f * AA_MAXT + 0.5f), y0), y1 - AA_MAXT); y1 = y0 + AA_MAXT; }
        const float isx = 1.0f / supx, isy = 1.0f / supy;
        float acc[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
        for (int y = y0; y < y1; ++y) {
            const float wy = fmaxf(0.0f, 1.0f - fabsf(((float)y + 0.5f - cy) * isy));
            const uint8_t* r = img + ((size_t)y * W) * 3;
            float row[3] = {0.f, 0.f, 0.f}, wr = 0.f;
            for (int x = x0; x < x1; ++x) {
                const float wx = fmaxf(0.0f, 1.0f - fabsf(((float)x + 0.5f - cx) * isx));
                row[0] += wx * (float)r[x * 3 + 2]; row[1] += wx * (float)r[x * 3 + 1]; row[2] += wx * (float)r[x * 3 + 0];
                wr += wx;
            }
            acc[0] += wy * row[0]; acc[1] += wy * row[1]; acc[2] += wy * row[2];
            wsum += wy * wr;
        }
        const float inv = wsum > 0.f ? 1.0f / (wsum * 255.0f) : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = f32_to_bf16((acc[c] * inv - mean[c]) * istd[c]);
    }
#if CROP_FLIP
    const int st = mirror ? ow - 1 - ox : ox;      // the store column
#else
    const int st = ox;
#endif
    if (oc == 3) {
        uint16_t* dst = out + (((size_t)crop * oh + oy) * ow + st) * 3;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    } else {            // 8-channel form for the MFMA conv kernel (Cin % 8 == 0): RGB + 5 zero channels, one 16-B store
        uint4 v;
        v.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16); v.y = (uint32_t)o[2]; v.z = 0; v.w = 0;
        *(uint4*)(out + (((size_t)crop * oh + oy) * ow + st) * 8) = v;
    }
}
