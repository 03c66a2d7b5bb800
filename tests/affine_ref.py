"""Float64 restatement of the pose checkpoints' centre/scale box transform (csrc/pam_box_cs.hpp) and of the affine crop kernel
(csrc/pam_crop_affine_kernel.inc) with a DERIVED per-element tolerance, NumPy only, no GPU -- the companion of image_ref.preprocess64,
built the same way.  Nothing in a tolerance here is tuned against the kernel: each term is a rounding bound of a number format or the
sensitivity of the float64 reference itself to the roundings the float32 kernel may make.  tests/test_affine_ref.py checks the
restatement against known answers and shows that the tolerance rejects each deliberately wrong restatement on the case inputs;
tests/test_gpu_affine_crop.py takes its inputs from the case builders at the end of this file, so both see the same data."""
import functools

import numpy as np

from image_ref import AA_MAXT, MEAN, STD, U32, bf16_ulp, f32, noise_frames, ulp32

BOX_SCALE = 1.25


def box_cs64(boxes, out_w, out_h, scale=BOX_SCALE, aspect_fix=True):
    """The effective boxes of (n, 4) xywh boxes: the expressions of include/pam.h in float64 from the float32 inputs, in that order, each
    result rounded once to float32.  A box whose We is not > 0 (NaN included) gives (x, y, 0, 0).  aspect_fix=False is for
    tests/test_affine_ref.py only (a deliberately wrong restatement).  -> (n, 4) float32."""
    b = f32(boxes).reshape(-1, 4)
    out = np.empty_like(b)
    ow, oh, s = float(out_w), float(out_h), float(np.float32(scale))
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(len(b)):
            x, y, w, h = [np.float64(v) for v in b[i]]
            cx = x + w * 0.5
            cy = y + h * 0.5
            if aspect_fix:
                if w * oh > h * ow:
                    h = w * oh / ow
                elif w * oh < h * ow:
                    w = h * ow / oh
            We = w * s
            He = We * oh / ow if aspect_fix else h * s
            if not np.float32(We) > 0:
                out[i] = (b[i, 0], b[i, 1], 0.0, 0.0)
                continue
            out[i] = (np.float32(cx - We * 0.5), np.float32(cy - He * 0.5), np.float32(We), np.float32(He))
    return out


def _coords(b0, ext, o, half=0.0):
    """Sample coordinates of one axis as the kernel forms them, b0 + i * (ext / o), every operation rounded to float32 (no FMA), and
    delta: 4 float32 ulps of the largest term -- the sum has one rounding after the product's, each at most half an ulp of the
    largest term, and the scale's own rounding moves the product by at most half an ulp more; 4 leaves room for a contracted or
    reordered form.  half: the stretch form's half-pixel convention, b0 + (i + half) * sc - half (a wrong restatement here)."""
    with np.errstate(invalid='ignore', over='ignore'):
        sc = f32(ext) / f32(o)
        t = (np.arange(o, dtype=np.float32) + f32(half)) * sc
        c = f32(b0) + t
        if half:
            c = c - f32(half)
    big = max(abs(float(b0)), float(np.abs(t).max()), 0.5)
    delta = 4.0 * float(ulp32(big)) if np.isfinite(big) else 0.0
    return c.astype(np.float64), float(sc), delta


def _bilinear_rows(s, size, replicate=False):
    """(o, size) weights of the 2-tap sample at coordinates s, integer coordinates = pixel centres.  A tap outside [0, size) is dropped
    (it contributes 0: a constant border); a coordinate that is not finite, or not inside (-1, size), has no tap at all.
    replicate=True: the coordinate clamped to the frame instead (the edge replicated: a wrong restatement here)."""
    s = np.asarray(s, dtype=np.float64)
    w = np.zeros((s.size, size))
    if replicate:
        s = np.clip(np.where(np.isfinite(s), s, 0.0), 0.0, size - 1.0)
    ok = np.isfinite(s) & (s > -1.0) & (s < size)
    sv = np.where(ok, s, 0.0)
    i0 = np.floor(sv).astype(np.int64)
    f = sv - i0
    r = np.arange(s.size)
    a = ok & (i0 >= 0)
    b = ok & (i0 + 1 < size)
    np.add.at(w, (r[a], i0[a]), (1.0 - f)[a])
    np.add.at(w, (r[b], i0[b] + 1), f[b])
    return w


def _triangle_rows(s, sc, size, max_taps=AA_MAXT, count_outside=True):
    """(o, size) weights of the antialias form: taps = the integer positions within sup = max(sc, 1) of s, weight 1 - |i - s| / sup, at
    most max_taps (the ones nearest s), divided by the sum over ALL taps of the window -- a tap outside the frame carries colour 0 but
    counts in the normaliser (count_outside=False: only the taps inside count, a wrong restatement here).  -> weights, most taps."""
    s = np.asarray(s, dtype=np.float64)
    sup = max(sc, 1.0) if np.isfinite(sc) else np.inf
    w = np.zeros((s.size, size))
    most = 0
    for r in range(s.size):
        c = s[r]
        if not np.isfinite(c) or not (-(max_taps + 1) < c < size + max_taps):
            continue
        lo, hi = np.ceil(c - sup), np.floor(c + sup)
        if hi - lo + 1 > max_taps:
            lo = np.floor(c - 0.5 * max_taps) + 1
            hi = lo + max_taps - 1
        i = np.arange(int(lo), int(hi) + 1)
        wt = np.maximum(0.0, 1.0 - np.abs(i - c) / sup)
        inside = (i >= 0) & (i < size)
        tot = wt.sum() if count_outside else wt[inside].sum()
        if tot > 0:
            w[r, i[inside]] = wt[inside] / tot
        most = max(most, i.size)
    return w, most


def warp64(frames, view_of, boxes, resolution, scale=BOX_SCALE, antialias=False, half=0.0, replicate=False, aspect_fix=True,
           count_outside=True):
    """k_preprocess_crops_affine restated: the effective box of every box (box_cs64), per output pixel (u, v) the bilinear sample at
    sx = xe + u * (We / W), sy = ye + v * (He / H) (integer coordinates = pixel centres, a tap outside the frame = 0) from the BGR uint8
    frame -- with antialias, where the scale exceeds 1, the triangle filter of _triangle_rows -- then BGR->RGB, /255, (v - mean) / std.
    Coordinates come from the float32 effective box in float32; interpolation and normalisation are float64.
    -> (value, tol), both (n, 3, H, W) float64.  tol per element, built as image_ref.preprocess64 builds its own:
       the change of the reference when its sample coordinate moves by +-delta along x, plus the same along y (delta: _coords -- 4
       float32 ulps of the coordinate expression's largest term; evaluated at the moved coordinate, so a cell edge, the frame's edge
       or the end of a filter window within delta is covered)
     + 8 float32 ulps for the interpolation and normalisation, at the magnitude the float32 chain works at, |value| + (v/255 + mean) /
       std, and with the triangle filter one more per tap of the row and of the column accumulation
     + half a bf16 ulp at |value| + the terms above (the float32 number that is rounded may sit that far from the reference).
    half / replicate / aspect_fix / count_outside exist for tests/test_affine_ref.py only (deliberately wrong restatements)."""
    frames = np.asarray(frames); boxes = f32(boxes).reshape(-1, 4); view_of = np.asarray(view_of)
    H, W = resolution
    fh, fw = frames.shape[1], frames.shape[2]
    n = view_of.size
    eff = box_cs64(boxes, W, H, scale, aspect_fix=aspect_fix)
    val = np.empty((n, 3, H, W)); tol = np.empty((n, 3, H, W))
    for i in range(n):
        xe, ye, We, He = [float(v) for v in eff[i]]
        cx, scx, dx = _coords(xe, We, W, half)
        cy, scy, dy = _coords(ye, He, H, half)
        taps = 0
        if not We > 0.0:
            wx, wy = np.zeros((W, fw)), np.zeros((H, fh))
            wxs, wys = [wx], [wy]
        elif antialias and (scx > 1.0 or scy > 1.0):
            (wx, tx), (wy, ty) = _triangle_rows(cx, scx, fw, count_outside=count_outside), _triangle_rows(cy, scy, fh, count_outside=count_outside)
            taps = tx + ty
            wxs = [_triangle_rows(cx + d, scx, fw, count_outside=count_outside)[0] for d in (-dx, dx)]
            wys = [_triangle_rows(cy + d, scy, fh, count_outside=count_outside)[0] for d in (-dy, dy)]
        else:
            wx, wy = _bilinear_rows(cx, fw, replicate), _bilinear_rows(cy, fh, replicate)
            wxs = [_bilinear_rows(cx + d, fw, replicate) for d in (-dx, dx)]
            wys = [_bilinear_rows(cy + d, fh, replicate) for d in (-dy, dy)]
        sub = frames[int(view_of[i])].astype(np.float64)                       # (fh, fw, 3) BGR
        along_y = lambda w_, m: (w_ @ m.reshape(fh, -1)).reshape(H, -1, 3)                         # (fh, X, 3) -> (H, X, 3)
        along_x = lambda w_, m: np.tensordot(m, w_, axes=([1], [1])).transpose(1, 0, 2)            # (Y, fw, 3) -> (3, Y, W)
        rowsum, colsum = along_y(wy, sub), along_x(wx, sub)                    # (H, fw, 3), (3, fh, W)
        v = along_x(wx, rowsum)                                                # (3, H, W) BGR
        slack = np.zeros_like(v)
        part = np.zeros_like(v)
        for w_ in wxs:
            part = np.maximum(part, np.abs(along_x(w_, rowsum) - v))
        slack += part
        part = np.zeros_like(v)
        for w_ in wys:
            part = np.maximum(part, np.abs(np.tensordot(w_, colsum, axes=([1], [1])).transpose(1, 0, 2) - v))
        slack += part
        v, slack = v[::-1], slack[::-1]                                        # BGR -> RGB
        out = (v / 255.0 - MEAN[:, None, None]) / STD[:, None, None]
        slack = slack / 255.0 / STD[:, None, None]
        mag = np.abs(out) + (v / 255.0 + MEAN[:, None, None]) / STD[:, None, None]
        t = slack + (8 + taps) * 2.0 * U32 * mag                               # float32 ulp = 2 * U32 relative
        val[i] = out
        tol[i] = 0.5 * bf16_ulp(np.abs(out) + t) + t
    return val, tol


def kernel_f32_identity(pix_rgb):
    """The float32 expression the kernel writes for a sample that falls on a pixel (both fractions 0): (p * (1/255) - mean) * (1/std), every
    constant and operation float32 -> float32 array; pix_rgb (..., 3) uint8 values in RGB order, 0 for a tap outside the frame."""
    p = f32(pix_rgb)
    mean = f32([0.485, 0.456, 0.406])
    istd = f32(1.0) / f32([0.229, 0.224, 0.225])
    return (p * (f32(1.0) / f32(255.0)) - mean) * istd


# ---- the inputs of the GPU tests (and of the CPU tests that show the checks reject wrong code on them) --------------------------------
FRAME_SIZES = ((47, 61), (131, 97))                  # (h, w), 2 views each
SMALL_OUTPUTS = ((16, 12), (64, 48))                 # every box
LARGE_OUTPUTS = ((256, 192), (384, 288))             # 3 crops only
CROP_COUNTS = (1, 3, 5)
NAN = float('nan')


def case_boxes(frame_hw, resolution):
    """The boxes of one (frame, output) case, xywh, with names: wider / taller than the output's aspect and exactly at it, up-scaled (a
    9 x 7 box) and down-scaled about 3 x (We = 3 out_w), hanging over each of the four frame edges, wholly outside the frame, w = 0 and
    h = 0 (the aspect fix gives both an extent), both 0 (We = 0: an all-zero crop), and a NaN extent (w: We is NaN, all zero; h: We is
    valid and the rows' coordinates are NaN)."""
    fh, fw = frame_hw
    H, W = resolution
    return [('wider', [5, 10, 30, 12]), ('taller', [12.5, 3.25, 8, 30]), ('at the aspect', [10, 8, 12, 16]),
            ('up-scaled 9 x 7', [20.25, 15.5, 9, 7]), ('down-scaled 3 x', [fw * 0.5 - 1.2 * W, fh * 0.5 - 1.2 * H, 2.4 * W, 3.2 * H]),
            ('over the left edge', [-6.5, 10, 14, 20]), ('over the top edge', [10, -7.25, 15, 18]),
            ('over the right edge', [fw - 8, 12, 16, 20]), ('over the bottom edge', [15, fh - 9, 14, 20]),
            ('outside, right', [fw + 40, 5, 10, 14]), ('outside, above left', [-300, -300, 20, 30]),
            ('w = 0', [10, 10, 0, 20]), ('h = 0', [10, 10, 20, 0]), ('w = h = 0', [10, 10, 0, 0]),
            ('NaN width', [10, 10, NAN, 20]), ('NaN height', [10, 10, 12, NAN])]


LARGE_PICK = ('taller', 'down-scaled 3 x', 'over the right edge')        # the 3 crops of the large outputs
OUTSIDE = ('outside, right', 'outside, above left', 'w = h = 0', 'NaN width', 'NaN height')     # crops that must be all zero


def case_list():
    """(frame (h, w), resolution, names, boxes (n, 4) float32) for every value case of the GPU test."""
    out = []
    for hw in FRAME_SIZES:
        for res in SMALL_OUTPUTS:
            nb = case_boxes(hw, res)
            out.append((hw, res, tuple(k for k, _ in nb), np.asarray([b for _, b in nb], dtype=np.float32)))
        for res in LARGE_OUTPUTS:
            nb = [kb for kb in case_boxes(hw, res) if kb[0] in LARGE_PICK]
            out.append((hw, res, tuple(k for k, _ in nb), np.asarray([b for _, b in nb], dtype=np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def case_frames(frame_hw, seed=11):
    fr = noise_frames(2, frame_hw[0], frame_hw[1], seed)
    fr.setflags(write=False)
    return fr


def case_view_of(n):
    return (np.arange(n) % 2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case_reference(k, antialias):
    """(val, tol) of case_list()[k], computed once and shared (read-only)."""
    hw, res, _, boxes = case_list()[k]
    val, tol = warp64(case_frames(hw), case_view_of(len(boxes)), boxes, res, antialias=antialias)
    val.setflags(write=False); tol.setflags(write=False)
    return val, tol
