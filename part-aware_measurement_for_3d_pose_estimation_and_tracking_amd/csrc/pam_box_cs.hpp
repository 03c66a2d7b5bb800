// The pose checkpoints' box transform, ONE definition for the crop kernel, the table kernel and the host entry (pam_crop.hip).
// Official HRNet / Simple Baselines / DARK test code: _box2cs (centre + scale from the box: the box widened to the input's aspect ratio
// about its centre, then enlarged by 1.25), get_affine_transform without rotation (a uniform scale about the centre) and transform_preds
// (heat-map cells back through the same enlarged box).  All three are this function: the EFFECTIVE box (xe, ye, We, He) is what the crop
// samples and what the decode maps a heat-map cell through (px / hm_w * We + xe).
// float64 from the float32 inputs, in exactly the order written below, each result rounded once to float32.  The library is built with
// -ffp-contract=off, so host, device and a NumPy float64 restatement give the same bits.
// The official code compares w > aspect * h with a float `aspect` = out_w / out_h; the integer-ratio form w * out_h > h * out_w used here
// differs from it only on exact ties (a box exactly at the aspect, where a rounded `aspect` may fall on either side and the official code
// then grows one extent by a rounding error; here such a box keeps both extents).
// A box whose effective width is not > 0 (a zero or negative extent, NaN) gives (x, y, 0, 0): its crop is all zero before normalisation.
#pragma once
#include <hip/hip_runtime.h>

struct PamBoxCs { float x, y, w, h; };

__host__ __device__ inline PamBoxCs pam_box_cs_fn(float x, float y, float w, float h, int out_w, int out_h, float scale) {
    const double ow = (double)out_w, oh = (double)out_h;
    double wd = (double)w, hd = (double)h;
    const double cx = (double)x + wd * 0.5, cy = (double)y + hd * 0.5;
    if (wd * oh > hd * ow) hd = wd * oh / ow;             // too wide: grow the height
    else if (wd * oh < hd * ow) wd = hd * ow / oh;        // too tall: grow the width
    const double We = wd * (double)scale, He = We * oh / ow;
    PamBoxCs r;
    r.w = (float)We;
    if (!(r.w > 0.0f)) { r.x = x; r.y = y; r.w = 0.0f; r.h = 0.0f; return r; }
    r.h = (float)He;
    r.x = (float)(cx - We * 0.5);
    r.y = (float)(cy - He * 0.5);
    return r;
}
