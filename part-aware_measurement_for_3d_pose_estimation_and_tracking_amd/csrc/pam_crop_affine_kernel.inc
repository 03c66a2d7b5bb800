// The affine crop kernel's text, included once per form by pam_crop.hip with CROP_KERNEL (the kernel's name) and CROP_FLIP defined.
// CROP_FLIP 0: rows n_src .. (grid) repeat row n_src - 1.  CROP_FLIP 1: rows [0, n_src) plain, rows [n_src, 2 n_src) the same samples stored
// at column ow - 1 - ox, rows from 2 n_src on repeat row 2 n_src - 1 (crop_row / store_pixel of pam_crop.hip, in this file's own statements).
// It is no template behind two wrappers as the stretch form is: behind one, the same text compiled to another prologue and the launch
// at 20 crops measured 0.4 % above the range of the parent's own rounds (DESIGN.md, section 10p).
// The box each row samples is the EFFECTIVE box of pam_box_cs.hpp, computed inline from the raw box (uniform per workgroup); thread 0 of
// a plain row's first workgroup stores it to eff[row] for the decode and the OKS-NMS.  Rows >= n_src of eff are never written.
// Sampling is warpAffine's convention: integer coordinates are pixel centres, output pixel (u, v) reads the frame at
// sx = xe + u * (We / ow), sy = ye + v * (He / oh) (float32, no half-pixel terms), bilinear over the four neighbours, and a tap outside
// the frame contributes 0 (BORDER_CONSTANT), it is not the replicated edge.  A box with We == 0 (pam_box_cs.hpp) is all zero.
// CROP_UDP 1 (Unbiased Data Processing, Huang et al., CVPR 2020): the same box on an align-corners grid, pitch We / (ow - 1), He / (oh - 1):
// pixel 0 reads the box's left edge and pixel ow - 1 its right edge (the entry point refuses ow < 2 and oh < 2).  Nothing else differs; the
// antialias branch takes the pitch as its scale.  CROP_UDP 0 leaves the text of the affine kernels as it was.
__global__ __launch_bounds__(256) void CROP_KERNEL(int n_src, const uint8_t* const* __restrict__ frames, int H, int W,
                                                   const int* __restrict__ view_of, const float* __restrict__ boxes, float box_scale,
                                                   int oh, int ow, int oc, uint16_t* __restrict__ out, int antialias,
                                                   float* __restrict__ eff) {
#if CROP_FLIP
    const int crop = blockIdx.y, mirror = crop >= n_src, src = min(mirror ? crop - n_src : crop, n_src - 1);
#else
    const int crop = blockIdx.y, src = min(crop, n_src - 1);
#endif
    const PamBoxCs e = pam_box_cs_fn(boxes[src * 4 + 0], boxes[src * 4 + 1], boxes[src * 4 + 2], boxes[src * 4 + 3], ow, oh, box_scale);
    if (blockIdx.x == 0 && threadIdx.x == 0 && crop < n_src) {
        eff[crop * 4 + 0] = e.x; eff[crop * 4 + 1] = e.y; eff[crop * 4 + 2] = e.w; eff[crop * 4 + 3] = e.h;
    }
    const int px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= oh * ow) return;
    const int oy = px / ow, ox = px % ow;
    const uint8_t* __restrict__ img = frames[view_of[src]];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, istd[3] = {1.0f / 0.229f, 1.0f / 0.224f, 1.0f / 0.225f};
#if CROP_UDP
    const float scx = e.w / (float)(ow - 1), scy = e.h / (float)(oh - 1);
#else
    const float scx = e.w / (float)ow, scy = e.h / (float)oh;
#endif
    const float sx = e.x + (float)ox * scx, sy = e.y + (float)oy * scy;
    const bool live = e.w > 0.0f;
    float val[3] = {0.f, 0.f, 0.f};                // RGB, 0 .. 255, before the normalisation
    if (!(antialias && (scx > 1.0f || scy > 1.0f))) {
        // the comparisons are false for a NaN coordinate and keep the int conversion inside [-1, W - 1] x [-1, H - 1]
        if (live && sx > -1.0f && sx < (float)W && sy > -1.0f && sy < (float)H) {
            const float flx = floorf(sx), fly = floorf(sy);
            const int x0 = (int)flx, y0 = (int)fly;
            const float fx = sx - flx, fy = sy - fly;
            uint8_t t[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int y = y0 + k;
                if (y < 0 || y >= H) continue;     // a row outside the frame: its two taps stay 0
                const uint8_t* r = img + ((size_t)y * W) * 3;
                // both pixels and the two bytes behind them inside the row: ONE unaligned 8-byte load (load_two_pixels in pam_crop.hip); else byte
                // loads of the pixels that exist
                if (x0 >= 0 && x0 + 2 < W) {
                    struct __attribute__((packed)) U8 { uint32_t x, y; };
                    const U8 q = *(const U8*)(r + x0 * 3);
#pragma unroll
                    for (int b = 0; b < 6; ++b) t[k][b] = (uint8_t)((b < 4 ? q.x >> (8 * b) : q.y >> (8 * (b - 4))) & 0xff);
                } else {
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        if (x0 >= 0) t[k][b] = r[x0 * 3 + b];
                        if (x0 + 1 < W) t[k][3 + b] = r[(x0 + 1) * 3 + b];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {          // c indexes RGB; source is BGR
                const int sc = 2 - c;
                const float a = (float)t[0][sc], b = (float)t[0][3 + sc];
                const float cc = (float)t[1][sc], d = (float)t[1][3 + sc];
                const float top = a + (b - a) * fx, bot = cc + (d - cc) * fx;
                val[c] = top + (bot - top) * fy;
            }
        }
    } else {
        // down-scaling: triangle weights of support max(scale, 1) about the sample position, taps = the integer positions inside the
        // support, at most AA_MAXT per axis (the ones nearest the centre).  A tap outside the frame carries colour 0 but COUNTS in the
        // normaliser, so a border fades to black as the zero border of the plain form does.  No window of a sample further than
        // AA_MAXT + 1 from the frame reaches it (half a window is at most AA_MAXT / 2 + 1): black, and no int conversion of a huge value.
        const float supx = fmaxf(scx, 1.0f), supy = fmaxf(scy, 1.0f);
        if (live && sx > -(float)(AA_MAXT + 1) && sx < (float)(W + AA_MAXT) && sy > -(float)(AA_MAXT + 1) && sy < (float)(H + AA_MAXT)) {
            const float ax0 = ceilf(sx - supx), ax1 = floorf(sx + supx), ay0 = ceilf(sy - supy), ay1 = floorf(sy + supy);
            int x0, x1, y0, y1;                      // [x0, x1) x [y0, y1)
            if (ax1 - ax0 + 1.0f > (float)AA_MAXT) { x0 = (int)floorf(sx - 0.5f * AA_MAXT) + 1; x1 = x0 + AA_MAXT; }
            else { x0 = (int)ax0; x1 = (int)ax1 + 1; }
            if (ay1 - ay0 + 1.0f > (float)AA_MAXT) { y0 = (int)floorf(sy - 0.5f * AA_MAXT) + 1; y1 = y0 + AA_MAXT; }
            else { y0 = (int)ay0; y1 = (int)ay1 + 1; }
            const float isx = 1.0f / supx, isy = 1.0f / supy;
            float wr = 0.f;                          // the row normaliser: every tap of the window, inside the frame or not
            for (int x = x0; x < x1; ++x) wr += fmaxf(0.0f, 1.0f - fabsf(((float)x - sx) * isx));
            const int xa = max(x0, 0), xb = min(x1, W);
            float acc[3] = {0.f, 0.f, 0.f}, wc = 0.f;
            for (int y = y0; y < y1; ++y) {
                const float wy = fmaxf(0.0f, 1.0f - fabsf(((float)y - sy) * isy));
                wc += wy;
                if (y < 0 || y >= H) continue;
                const uint8_t* r = img + ((size_t)y * W) * 3;
                float row[3] = {0.f, 0.f, 0.f};
                for (int x = xa; x < xb; ++x) {
                    const float wx = fmaxf(0.0f, 1.0f - fabsf(((float)x - sx) * isx));
                    row[0] += wx * (float)r[x * 3 + 2]; row[1] += wx * (float)r[x * 3 + 1]; row[2] += wx * (float)r[x * 3 + 0];
                }
                acc[0] += wy * row[0]; acc[1] += wy * row[1]; acc[2] += wy * row[2];
            }
            const float wsum = wc * wr, inv = wsum > 0.f ? 1.0f / wsum : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) val[c] = acc[c] * inv;
        }
    }
    uint16_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = f32_to_bf16((val[c] * (1.0f / 255.0f) - mean[c]) * istd[c]);
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
