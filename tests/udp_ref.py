"""Float64 restatement of the UDP protocol (Huang et al., CVPR 2020; contract in include/pam.h at pam_preprocess_crops_udp and
pam_head_decode_udp), NumPy only: crop_udp64 (the align-corners crop, csrc/pam_crop_affine_kernel.inc under CROP_UDP, with
affine_ref.warp64's derived tolerance), udp64 (the UDP form of DARK at given arg-max cells, csrc/pam_head.hip: k_udp_finish, with a
per-case bound and a `decided` mask), map64 (UDP's transform_preds), official_udp (an independent statement of mmpose's post_dark_udp
on scipy.ndimage, sharing no code with udp64) and the inputs of tests/test_gpu_udp.py, so that the CPU tests (tests/test_udp_ref.py)
judge the same data the GPU tests run on.

The bound of a case is derived the way dark_ref.dark64 derives its own, never measured on a kernel.  The kernel's float32 map lies
within image_ref.head64's per-cell bound (plus the merge's rounding, flip_ref.merge64) of the float64 one.  The blur is linear with
positive taps and a reflected cell is a cell of the map, so the blurred map lies within bB = blur(bound) (the same reflection) of B.
Where a sample is clear of both clamps (B - bB > 0.001 and B + bB < 50) the logarithm turns that into e = bB / (B - bB); where the
clamp certainly acts (B + bB <= 0.001 or B - bB >= 50) the logarithm is the clamp's own on both sides and e = 0.  The derivatives take
e by the triangle inequality with the UDP stencil's weights (samples c, x+, x-, y+, y-, ++, --):
    dg  = max((e[x+] + e[x-]) / 2, (e[y+] + e[y-]) / 2)
    exx = e[x+] + 2 e[c] + e[x-],  eyy alike,  exy = (e[++] + e[x+] + e[y+] + 2 e[c] + e[x-] + e[y-] + e[--]) / 2
    dH  = max(exx + exy, exy + eyy)
and the solve, with H' = H + 2^-23 I on both sides (the e of the contract is exact, it adds no error),
    |do|_inf <= |H'^-1|_inf (dg + dH |o|_inf) / (1 - |H'^-1|_inf dH).
A border winner's clamped samples coincide with others (L[x-1] = L[c] at px = 0); the triangle inequality holds all the same.
A case is UNDECIDED when its arg-max is (dark_ref.argmax_decided), when a sample lies within its bound of 0.001 or of 50, when the
denominator is <= 0, or when the bound exceeds dark_ref.CAP.  The float64 roundings of the blur, the logarithm and the solve (1e-16
relative) are not counted."""
import functools

import numpy as np

import affine_ref as A
import dark_ref as D
import flip_ref as FR
import image_ref as R
from image_ref import MEAN, STD, U32, bf16_ulp, f32, ulp32

J = R.J
CAP = D.CAP
LO, HI = 1.0e-3, 50.0
EPS = float(np.finfo(np.float32).eps)          # 2^-23 on the Hessian's diagonal
# (dy, dx) of the 7 sampled cells: centre, x + 1, x - 1, y + 1, y - 1, (+1, +1), (-1, -1)
SAMPLES = ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1))
# udp_inputs' seed of the random-blob cases, chosen on the CPU with the float64 reference alone.  Seeds 1 and 2 leave no case undecided in
# any (C, map, crops, flags) case (derived bounds up to 1.9e-3 cell, the largest on the 7 x 5 map at 256 channels); seed 3 leaves one
# of the 51 cases of C = 256, 7 x 5, 3 crops, merged with the shift undecided (bound 2.07e-3), more than the 1 % the tests allow.  The
# first of them is taken.  tests/test_udp_ref.py asserts the share for this seed.
SEED = 1
UDP_CHANNELS = D.DARK_CHANNELS
UDP_MAPS = D.DARK_MAPS
UDP_CROPS = D.DARK_CROPS
UDP_FLAGS = D.DARK_FLAGS


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    """BORDER_REFLECT_101 of indices i into [0, n), n >= 2, however far outside: m = i mod 2 (n - 1) >= 0, m < n ? m : 2 (n - 1) - m."""
    p = 2 * (n - 1)
    m = np.mod(np.asarray(i), p)
    return np.where(m < n, m, p - m)


def blur_reflect64(M, g):
    """Separable blur of (..., h, w) maps, rows first then columns, float64 sums in ascending tap order, cells outside the map read the
    reflected cell (reflect101; more than one bounce where (k - 1) / 2 >= the map's size)."""
    k = g.size; r = (k - 1) // 2
    h, w = M.shape[-2:]
    with np.errstate(invalid='ignore'):
        P = M[..., reflect101(np.arange(-r, w + r), w)]
        H = np.zeros_like(M)
        for t in range(k):
            H = H + g[t] * P[..., :, t:t + w]
        P = H[..., reflect101(np.arange(-r, h + r), h), :]
        B = np.zeros_like(M)
        for t in range(k):
            B = B + g[t] * P[..., t:t + h, :]
    return B


def _taylor(L):
    """L (7, ...) logs at SAMPLES -> gx, gy, dxx, dyy, dxy."""
    return (0.5 * (L[1] - L[2]), 0.5 * (L[3] - L[4]), L[1] - 2.0 * L[0] + L[2], L[3] - 2.0 * L[0] + L[4],
            0.5 * (L[5] - L[1] - L[3] + 2.0 * L[0] - L[2] - L[4] + L[6]))


def udp64(M, bound, idx, k, variant='ok'):
    """M, bound (n, 17, h, w) float64 (image_ref.head64 / flip_ref.merge64), idx (n, 17) flat arg-max cells, k the blur size or 0 ->
    dict(inside, ox, oy (cells), bound (cells, infinity norm; inf where it cannot be formed), decided).  `inside` marks the cases that
    take the step: every case when k != 0 (there is no inside rule), none at k == 0 (offset 0, bound 0, decided) -- the key keeps
    dark_ref.judge usable.  `decided` does not include the arg-max (dark_ref.argmax_decided: the caller knows which cells it passes).
    variant (tests, deliberately wrong): 'zero_pad' (DARK's zero frame), 'stencil2' (DARK's +-2 second derivatives with 0.25 and its
    four-corner dxy), 'inside_rule' (DARK's 1 < px < w - 2, 1 < py < h - 2), 'no_eps', 'clamp_dark' (max(B, 1e-10), no upper clamp)."""
    n, j, h, w = M.shape
    zero = np.zeros((n, j))
    if k == 0:
        return dict(inside=np.zeros((n, j), dtype=bool), ox=zero, oy=zero.copy(), bound=zero.copy(), decided=np.ones((n, j), dtype=bool))
    g = D.taps(k)
    B = D.blur64(M, g, 'zero') if variant == 'zero_pad' else blur_reflect64(M, g)
    bB = blur_reflect64(bound, g)
    a, c = np.arange(n)[:, None], np.arange(j)[None, :]
    py, px = idx // w, idx % w
    cl = lambda v, hi: np.clip(v, 0, hi - 1)
    samples = SAMPLES
    if variant == 'stencil2':
        samples = SAMPLES + ((0, 2), (0, -2), (2, 0), (-2, 0), (-1, 1), (1, -1))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        Bs = np.stack([B[a, c, cl(py + dy, h), cl(px + dx, w)] for dy, dx in samples])
        bs = np.stack([bB[a, c, cl(py + dy, h), cl(px + dx, w)] for dy, dx in samples])
        if variant == 'clamp_dark':
            L = np.log(np.where(Bs > 1e-10, Bs, 1e-10))
        else:
            L = np.log(np.where(Bs > LO, np.where(Bs < HI, Bs, HI), LO))          # (a NaN clamps to 0.001)
        free = (Bs - bs > LO) & (Bs + bs < HI)
        held = (Bs + bs <= LO) | (Bs - bs >= HI)
        e = np.where(free, bs / np.where(free, Bs - bs, 1.0), np.where(held, 0.0, np.inf))
        gx, gy, dxx, dyy, dxy = _taylor(L)
        if variant == 'stencil2':
            dxx, dyy = 0.25 * (L[7] - 2.0 * L[0] + L[8]), 0.25 * (L[9] - 2.0 * L[0] + L[10])
            dxy = 0.25 * (L[5] - L[11] - L[12] + L[6])
        eps = 0.0 if variant == 'no_eps' else EPS
        hxx, hyy = dxx + eps, dyy + eps
        det = hxx * hyy - dxy * dxy
        ok = (det != 0) & np.isfinite(det)
        if variant == 'inside_rule':
            ok = ok & D.inside_of(idx, h, w)
        sdet = np.where(ok, det, 1.0)
        ox = np.where(ok, -(hyy * gx - dxy * gy) / sdet, 0.0)
        oy = np.where(ok, -(hxx * gy - dxy * gx) / sdet, 0.0)
        e = e[:7]
        dg = np.maximum(0.5 * (e[1] + e[2]), 0.5 * (e[3] + e[4]))
        exx, eyy = e[1] + 2.0 * e[0] + e[2], e[3] + 2.0 * e[0] + e[4]
        exy = 0.5 * (e[5] + e[1] + e[3] + 2.0 * e[0] + e[2] + e[4] + e[6])
        dH = np.maximum(exx + exy, exy + eyy)
        inv = np.maximum(np.abs(hyy) + np.abs(dxy), np.abs(dxy) + np.abs(hxx)) / np.abs(sdet)
        den = 1.0 - inv * dH
        good = ok & np.isfinite(dH) & (den > 0)
        bd = np.where(good, inv * (dg + dH * np.maximum(np.abs(ox), np.abs(oy))) / np.where(good, den, 1.0), np.inf)
    decided = good & (bd <= CAP)
    return dict(inside=np.ones((n, j), dtype=bool), ox=ox, oy=oy, bound=bd, decided=decided)


def map64(py, px, eff, h, w, variant='ok'):
    """UDP's transform_preds: fractional cells (n, m) through the effective boxes eff (n, 4) float32, float64 arithmetic with one float32
    rounding: x = xe + px * (We / (w - 1)), y = ye + py * (He / (h - 1)) -> (y, x) float64.  variant 'hm_w' (tests): the affine pitch."""
    b = np.asarray(f32(eff), dtype=np.float64)
    dh, dw = (h, w) if variant == 'hm_w' else (h - 1, w - 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = f32(b[:, 1:2] + np.asarray(py, dtype=np.float64) * (b[:, 3:4] / dh)).astype(np.float64)
        x = f32(b[:, 0:1] + np.asarray(px, dtype=np.float64) * (b[:, 2:3] / dw)).astype(np.float64)
    return y, x


def cells_of(rows, eff, h, w):
    """det rows (n, 17, 3) (y, x, score) -> positions in cells (py, px) through the inverse of map64, and the float32 rounding of the
    mapping in cells (half a float32 ulp of the stored coordinate; + 1e-9 cell for the float64 roundings of this inversion itself)."""
    b = np.asarray(eff, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        py = (rows[:, :, 0] - b[:, 1:2]) / b[:, 3:4] * (h - 1)
        px = (rows[:, :, 1] - b[:, 0:1]) / b[:, 2:3] * (w - 1)
        return py, px, 0.5 * ulp32(rows[:, :, 0]) * (h - 1) / b[:, 3:4] + 1e-9, 0.5 * ulp32(rows[:, :, 1]) * (w - 1) / b[:, 2:3] + 1e-9


# ---- mmpose's steps, stated independently ---------------------------------------------------------------------------------------------------
def official_udp(M, k):
    """mmpose 0.x post_dark_udp on float64 maps (n, 17, h, w), one map at a time: cv2.GaussianBlur(map, (k, k), 0) with its default
    border (here scipy.ndimage.correlate1d with the kernel getGaussianKernel(k, 0) would return, mode='mirror', rows then columns),
    np.clip(., 0.001, 50), np.log, the whole map framed with np.pad(mode='edge'), and at the arg-max cell of the UNBLURRED map the
    step -inv(H + eps I) g with np.linalg.inv.  -> coords (n, 17, 2) float64 (x, y) in cells."""
    from scipy.ndimage import correlate1d
    n, j, h, w = M.shape
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k) - (k - 1) / 2.0
    kern = np.exp(-x ** 2 / (2 * sigma ** 2))
    kern = kern / kern.sum()
    coords = np.zeros((n, j, 2))
    for a in range(n):
        for p in range(j):
            hm = M[a, p]
            flat = int(np.argmax(hm))
            coords[a, p] = (flat % w, flat // w)
            bl = correlate1d(correlate1d(hm, kern, axis=1, mode='mirror'), kern, axis=0, mode='mirror')
            lg = np.pad(np.log(np.clip(bl, 0.001, 50)), ((1, 1), (1, 1)), mode='edge')
            cx, cy = flat % w + 1, flat // w + 1
            i_ = lg[cy][cx]
            ix1, ix1_ = lg[cy][cx + 1], lg[cy][cx - 1]
            iy1, iy1_ = lg[cy + 1][cx], lg[cy - 1][cx]
            ix1y1, ix1_y1_ = lg[cy + 1][cx + 1], lg[cy - 1][cx - 1]
            derivative = np.array([[0.5 * (ix1 - ix1_)], [0.5 * (iy1 - iy1_)]])
            dxx = ix1 - 2 * i_ + ix1_
            dyy = iy1 - 2 * i_ + iy1_
            dxy = 0.5 * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_)
            hessian = np.array([[dxx, dxy], [dxy, dyy]]) + np.finfo(np.float32).eps * np.eye(2)
            coords[a, p] -= (np.linalg.inv(hessian) @ derivative)[:, 0]
    return coords


# ---- crop ------------------------------------------------------------------------------------------------------------------------------
def _coords(b0, ext, o, pitch='udp'):
    """Sample coordinates of one axis as the kernel forms them, b0 + i * (ext / (o - 1)), every operation rounded to float32 (no FMA),
    and delta as affine_ref._coords: 4 float32 ulps of the largest term.  pitch='out_w' (tests): the affine form's ext / o."""
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        sc = f32(ext) / f32(o if pitch == 'out_w' else o - 1)
        t = np.arange(o, dtype=np.float32) * sc
        c = f32(b0) + t
    big = max(abs(float(b0)), float(np.abs(t).max()), 0.5)
    delta = 4.0 * float(ulp32(big)) if np.isfinite(big) else 0.0
    return c.astype(np.float64), float(sc), delta


def crop_udp64(frames, view_of, boxes, resolution, scale=A.BOX_SCALE, antialias=False, pitch='udp'):
    """k_preprocess_crops_udp restated: affine_ref.warp64 with the align-corners pitch -- the effective box of every box
    (affine_ref.box_cs64), per output pixel (u, v) the bilinear sample at sx = xe + u * (We / (W - 1)), sy = ye + v * (He / (H - 1))
    (integer coordinates = pixel centres, a tap outside the frame = 0), with antialias, where the pitch exceeds 1, the triangle filter
    of affine_ref._triangle_rows with the pitch as its scale; then BGR->RGB, /255, (v - mean) / std.  -> (value, tol), both
    (n, 3, H, W) float64; tol per element is warp64's, term by term (the coordinate's +-delta sensitivity along x and y, 8 float32
    ulps + one per tap for interpolation and normalisation, half a bf16 ulp)."""
    frames = np.asarray(frames); boxes = f32(boxes).reshape(-1, 4); view_of = np.asarray(view_of)
    H, W = resolution
    fh, fw = frames.shape[1], frames.shape[2]
    n = view_of.size
    eff = A.box_cs64(boxes, W, H, scale)
    val = np.empty((n, 3, H, W)); tol = np.empty((n, 3, H, W))
    for i in range(n):
        xe, ye, We, He = [float(v) for v in eff[i]]
        cx, scx, dx = _coords(xe, We, W, pitch)
        cy, scy, dy = _coords(ye, He, H, pitch)
        taps = 0
        if not We > 0.0:
            wx, wy = np.zeros((W, fw)), np.zeros((H, fh))
            wxs, wys = [wx], [wy]
        elif antialias and (scx > 1.0 or scy > 1.0):
            (wx, tx), (wy, ty) = A._triangle_rows(cx, scx, fw), A._triangle_rows(cy, scy, fh)
            taps = tx + ty
            wxs = [A._triangle_rows(cx + d, scx, fw)[0] for d in (-dx, dx)]
            wys = [A._triangle_rows(cy + d, scy, fh)[0] for d in (-dy, dy)]
        else:
            wx, wy = A._bilinear_rows(cx, fw), A._bilinear_rows(cy, fh)
            wxs = [A._bilinear_rows(cx + d, fw) for d in (-dx, dx)]
            wys = [A._bilinear_rows(cy + d, fh) for d in (-dy, dy)]
        sub = frames[int(view_of[i])].astype(np.float64)                       # (fh, fw, 3) BGR
        along_y = lambda w_, m: (w_ @ m.reshape(fh, -1)).reshape(H, -1, 3)
        along_x = lambda w_, m: np.tensordot(m, w_, axes=([1], [1])).transpose(1, 0, 2)
        rowsum, colsum = along_y(wy, sub), along_x(wx, sub)
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
        t = slack + (8 + taps) * 2.0 * U32 * mag
        val[i] = out
        tol[i] = 0.5 * bf16_ulp(np.abs(out) + t) + t
    return val, tol


# ---- inputs of the GPU tests: decode --------------------------------------------------------------------------------------------------------
NOISE, FLOOR, GAIN, BLOB_SIGMA = 0.001, 0.05, 16.0, 0.6


def _vectors(wt):
    """(17, C) float64: the feature vector that raises joint j's map by 1 and no other joint's (the rows of pinv(wt)^T).  Its products
    with wt[j] are nearly all positive, so the head bound's sum of magnitudes is about the signal itself."""
    return np.linalg.pinv(wt.astype(np.float64)).T


def _centres(rng, size, r, count):
    """`count` blob centres along an axis of `size` cells under a blur of radius r: uniform over the cells further than r from both
    borders where there are such cells, else ON a border cell (0 or size - 1, drawn evenly).  Within reach of a border the blur's
    reflection adds a mirror image that drags the blurred peak to the border; one Newton step from the arg-max cell is then a cell or
    more long and its derived bound, which grows with the step, passes dark_ref.CAP at 256 channels whatever the seed.  On a border
    cell the image coincides with the blob and the step is the half cell of the edge-replicated stencil.  Winners on every border and
    in every corner of the larger maps are the planted cases' part (planted_inputs)."""
    lo, hi = r + 1.0, size - 2.0 - r
    if hi > lo:
        return lo + rng.random(count) * (hi - lo)
    return np.where(rng.random(count) < 0.5, 0.0, size - 1.0)


def udp_inputs(C, h, w, n, k, shift=False, seed=SEED):
    """A feature batch of 2n + 1 rows for n crops decoded with blur size k, shaped like a pose network's output under UDP: maps in
    (0, 50), a low floor and one peak per joint.  image_ref.head_inputs features scaled to NOISE, biases FLOOR + 0.05 b, and for each
    (crop, joint) a Gaussian blob (BLOB_SIGMA cells, GAIN in the joint's own map and in no other: _vectors) at a seeded fractional
    centre (_centres); the mirrored row n + i carries crop i's blobs mirrored, joint pair(j), at the column the merge reads them back
    from: w - 1 - cx, or with `shift` w - cx, as a network's map of the mirrored crop lies one column off before the official shift
    aligns it (a centre on column 0 then lies at w, outside the map: merged column 0 keeps the mirrored map's own edge value, as the
    official code's does).  A batch built for one setting and merged under the other is a blob pair one column apart: wider, flatter,
    and on the 7 x 5 map past dark_ref.CAP at 256 channels.  Rounded to bf16.
    The spare row 2n holds 1e30 everywhere: a call that reads it into a result shows.
    (dark_ref.dark_inputs does not serve: its biases of 30 and 60 put the blurred peaks at or above the clamp at 50, and a floor that
    high flattens the logarithm until the +-1 stencil's bound, four times DARK's, passes dark_ref.CAP.)
    -> feat (2n + 1, h, w, C) float32, wt, b, boxes (n, 4), centres (n, 17, 2) (cy, cx)."""
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    rng = np.random.default_rng([seed, C, h, w, n, 78])
    r = (k - 1) // 2
    centres = np.stack([_centres(rng, h, r, n * J), _centres(rng, w, r, n * J)], axis=1).reshape(n, J, 2)
    f = NOISE * feat.astype(np.float64)
    vec = GAIN * _vectors(wt)
    for i in range(n):
        for j in range(J):
            cy, cx = centres[i, j]
            f[i] += D._blob(h, w, cy, cx, BLOB_SIGMA)[:, :, None] * vec[j][None, None, :]
            f[n + i] += D._blob(h, w, cy, (w if shift else w - 1.0) - cx, BLOB_SIGMA)[:, :, None] * vec[FR.PAIR[j]][None, None, :]
    feat = R.bf16_rne(f).astype(np.float32)
    spare = np.full((1, h, w, C), R.bf16_rne(1.0e30), dtype=np.float32)
    b = (np.float32(FLOOR) + np.float32(0.05) * b).astype(np.float32)
    return np.concatenate([feat, spare]), wt, b, boxes[:n], centres


def reference(feat, wt, b, n, flags):
    """(M, bound) (n, 17, h, w) float64 of a call with `flags` on a batch of udp_inputs / planted_inputs."""
    return D.reference(feat, wt, b, n, flags)


def plant_cells(h, w):
    """The nine planted winners of an (h, w) map: the four corners, the middle of each edge, the centre (fewer where they coincide)."""
    ys, xs = sorted({0, h // 2, h - 1}), sorted({0, w // 2, w - 1})
    return [(y, x) for y in ys for x in xs]


def planted_inputs(h, w, flags, C=D.PLANT_C, seed=SEED):
    """One crop per cell of plant_cells, built as udp_inputs builds its crops, with joint 5's blob centred ON the cell: the winner is
    that border or corner cell -- where DARK's inside rule decodes nothing -- and takes the step, about half a cell outwards along each
    axis the cell lies on the border of (the edge-replicated stencil's answer for a peak on the edge).  The other joints carry no blob
    (floor and noise: flat maps, mostly undecided).  Joint 7's bias is -inf: a map of -inf, cell 0, which takes the step like any
    other cell (every sample clamps to 0.001: the offset is exactly 0).  The mirrored rows carry the blob of joint 6 = pair(5) at the
    column the merge reads it back from under `flags`.  Rows [0, n) plain, [n, 2n) mirrored, one spare at 1e30.
    -> feat, wt, b, boxes, cases [(crop, (y, x))]."""
    cells = plant_cells(h, w)
    n = len(cells)
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    f = NOISE * feat.astype(np.float64)
    vec = GAIN * _vectors(wt)
    for i, (y, x) in enumerate(cells):
        f[i] += D._blob(h, w, y, x, BLOB_SIGMA)[:, :, None] * vec[5]
        f[n + i] += D._blob(h, w, y, (w if flags & 2 else w - 1.0) - x, BLOB_SIGMA)[:, :, None] * vec[6]
    feat = R.bf16_rne(f).astype(np.float32)
    spare = np.full((1, h, w, C), R.bf16_rne(1.0e30), dtype=np.float32)
    b = (np.float32(FLOOR) + np.float32(0.05) * b).astype(np.float32)
    b[7] = -np.inf
    return np.concatenate([feat, spare]), wt, b, boxes[:n], list(enumerate(cells))


PLANTS = (((96, 72), 17), ((64, 48), 11), ((33, 17), 11), ((33, 17), 17), ((7, 5), 11), ((2, 2), 11), ((2, 2), 17))


# ---- inputs of the GPU tests: crop ----------------------------------------------------------------------------------------------------------
FRAME_SIZES = ((131, 97), (30, 40))                  # (h, w), 2 views each
OUTPUTS = ((16, 12), (64, 48), (2, 2))               # (H, W); at 2 x 2 the pitch divides by 1: pixel 1 reads the box's far edge
NAN = float('nan')


def case_boxes(frame_hw, resolution):
    """The boxes of one (frame, output) case, xywh, with names: inside the frame (up-scaled), down-scaled about 3 x (the antialias
    branch), half outside over each of two edges, fully outside, zero width and height (We = 0: an all-zero crop), NaN."""
    fh, fw = frame_hw
    H, W = resolution
    return [('inside', [6.25, 4.5, 9, 7]), ('inside, taller', [12.5, 3.25, 8, 20]),
            ('down-scaled 3 x', [fw * 0.5 - 1.2 * W, fh * 0.5 - 1.2 * H, 2.4 * W, 3.2 * H]),
            ('half outside, left', [-7.0, 5, 14, 18]), ('half outside, bottom', [8, fh - 9.0, 14, 18]),
            ('outside', [fw + 40, 5, 10, 14]), ('w = h = 0', [10, 10, 0, 0]), ('NaN width', [10, 10, NAN, 20]), ('NaN height', [10, 10, 12, NAN])]


ALL_ZERO = ('outside', 'w = h = 0', 'NaN width', 'NaN height')      # crops that must be the normalised zero everywhere


def case_list():
    """(frame (h, w), resolution, names, boxes (n, 4) float32) for every value case of the GPU crop test."""
    out = []
    for hw in FRAME_SIZES:
        for res in OUTPUTS:
            nb = case_boxes(hw, res)
            out.append((hw, res, tuple(k for k, _ in nb), np.asarray([b for _, b in nb], dtype=np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def case_frames(frame_hw, seed=13):
    fr = R.noise_frames(2, frame_hw[0], frame_hw[1], seed)
    fr.setflags(write=False)
    return fr


case_view_of = A.case_view_of


@functools.lru_cache(maxsize=None)
def case_reference(k, antialias):
    """(val, tol) of case_list()[k], computed once and shared (read-only)."""
    hw, res, _, boxes = case_list()[k]
    val, tol = crop_udp64(case_frames(hw), case_view_of(len(boxes)), boxes, res, antialias=antialias)
    val.setflags(write=False); tol.setflags(write=False)
    return val, tol
