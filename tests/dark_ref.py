"""Float64 restatement of the DARK decode (csrc/pam_head.hip: k_dark_finish; contract in include/pam.h, pam_head_decode_dark) with
derived bounds, NumPy only: dark64 (the offsets at given arg-max cells, a per-case bound and a `decided` mask), official_dark (an
independent statement of the published steps on scipy.ndimage, sharing no code with dark64) and the inputs of tests/test_gpu_dark.py,
so that the CPU tests (tests/test_dark_ref.py) judge the same data the GPU tests run on.

The bound of a case is derived, never measured on a kernel.  The kernel's float32 map lies within image_ref.head64's per-cell bound
(plus the merge's rounding, flip_ref.merge64) of the float64 one.  The blur is linear with positive taps, so the blurred map lies within
bB = blur(bound) of B; the logarithm turns that into e = bB / (B - bB) (|log(B') - log(B)| <= -log(1 - bB / B) <= bB / (B - bB)); the five
derivatives take it by the triangle inequality (dg for the gradient, dH for the Hessian, both in the infinity norm); and the solve by
    |do|_inf <= |H^-1|_inf (dg + dH |o|_inf) / (1 - |H^-1|_inf dH).
A case is UNDECIDED when the arg-max is (image_ref.argmax_check's rule), when a sampled B - bB <= 1e-10 (the clamp may or may not act),
when the denominator is <= 0, or when the bound exceeds CAP = 2e-3 cell: a decided case may not be excused by more than 1/125 of the
quarter-cell step this option replaces.  One case is decided although clamped: every one of the 13 samples has B + bB <= 1e-10, so
every logarithm is log(1e-10) in the kernel and here alike and the offset is exactly 0 (the scale-free definition's answer for a lone
spike on a negative map).  The float64 roundings of the blur, the logarithm and the solve (1e-16 relative) are not counted."""
import numpy as np

import flip_ref as FR
import image_ref as R

J = R.J
CAP = 2.0e-3
CLAMP = 1.0e-10
# image_ref.head_inputs seed of the random-blob cases, chosen on the CPU with the float64 reference alone.  Seed 0 leaves one of the 48
# inside cases of C = 256, 96 x 72, 3 crops, merged without the shift undecided (its arg-max: two cells within the float32 bound of
# each other), more than the 1 % the tests allow.  Seed 1 leaves no inside case undecided in any (C, map, crops, flags) case; its derived
# bounds run from 3e-5 to 1.9e-3 cell.  tests/test_dark_ref.py asserts the share for this seed.
SEED = 1
DARK_CHANNELS = (32, 48, 256)
DARK_MAPS = (((96, 72), 17), ((64, 48), 11), ((33, 17), 11), ((7, 5), 11))        # (map, blur size)
DARK_CROPS = (1, 3)
DARK_FLAGS = (0, 1, 3)
PLANT_C = 48
# (dy, dx) of the 13 sampled cells: centre, the cross at 1 and 2, the diagonals
SAMPLES = ((0, 0), (0, 1), (0, -1), (0, 2), (0, -2), (1, 0), (-1, 0), (2, 0), (-2, 0), (1, 1), (-1, 1), (1, -1), (-1, -1))


def sigma_of(k):
    """OpenCV's rule for GaussianBlur(.., (k, k), 0)."""
    return 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8


def taps(k, sigma=None):
    """g[i] = exp(-(i - R)^2 / (2 sigma^2)), normalised to sum 1, float64; 9 <= k <= 17, odd."""
    assert k % 2 == 1 and 9 <= k <= 17, k
    s = sigma_of(k) if sigma is None else sigma
    i = np.arange(k, dtype=np.float64) - (k - 1) // 2
    g = np.exp(-(i * i) / (2.0 * s * s))
    return g / g.sum()


def blur64(M, g, pad='zero'):
    """Separable blur of (..., h, w) maps, rows first then columns, float64 sums in ascending tap order, cells outside the map 0
    (pad='reflect', tests: the wrong border, cv2's default BORDER_REFLECT_101)."""
    k = g.size; r = (k - 1) // 2
    h, w = M.shape[-2:]
    width = [(0, 0)] * (M.ndim - 2)
    with np.errstate(invalid='ignore'):
        P = np.pad(M, width + [(0, 0), (r, r)], mode='reflect') if pad == 'reflect' else np.pad(M, width + [(0, 0), (r, r)])
        H = np.zeros_like(M)
        for t in range(k):
            H = H + g[t] * P[..., :, t:t + w]
        P = np.pad(H, width + [(r, r), (0, 0)], mode='reflect') if pad == 'reflect' else np.pad(H, width + [(r, r), (0, 0)])
        B = np.zeros_like(M)
        for t in range(k):
            B = B + g[t] * P[..., t:t + h, :]
    return B


def inside_of(idx, h, w, loose=False):
    """The cells the offset applies to: 1 < px < w - 2 and 1 < py < h - 2 (loose, tests: the quarter rule's px < w - 1)."""
    py, px = idx // w, idx % w
    e = 1 if loose else 2
    return (1 < px) & (px < w - e) & (1 < py) & (py < h - e)


def argmax_decided(M, bound):
    """(n, 17) bool: the arg-max of the map is decided in the sense of image_ref.argmax_check -- no cell but the float64 maximum (and
    cells exactly equal to it) can hold the float32 maximum.  A map with no finite maximum counts as decided (cell 0)."""
    n, j = M.shape[:2]
    m, b = M.reshape(n, j, -1), bound.reshape(n, j, -1)
    out = np.ones((n, j), dtype=bool)
    for a in range(n):
        for c in range(j):
            top = int(np.argmax(m[a, c]))
            if not np.isfinite(m[a, c, top]):
                continue
            cand = np.nonzero(m[a, c, top] - m[a, c] <= b[a, c, top] + b[a, c])[0]
            out[a, c] = bool(np.all(m[a, c, cand] == m[a, c, top]))
    return out


def _taylor(L):
    """L (13, ...) logs at SAMPLES -> gx, gy, dxx, dyy, dxy."""
    return (0.5 * (L[1] - L[2]), 0.5 * (L[5] - L[6]), 0.25 * (L[3] - 2.0 * L[0] + L[4]), 0.25 * (L[7] - 2.0 * L[0] + L[8]),
            0.25 * (L[9] - L[10] - L[11] + L[12]))


def dark64(M, bound, idx, k, variant='ok'):
    """M, bound (n, 17, h, w) float64 (image_ref.head64 / flip_ref.merge64), idx (n, 17) flat arg-max cells, k the blur size ->
    dict(inside, ox, oy (cells; 0 outside), bound (cells, infinity norm; 0 outside, inf where it cannot be formed), decided).
    `decided` does not include the arg-max (argmax_decided: the caller knows which cells it passes).
    variant (tests, deliberately wrong): 'no_blur', 'loose_border' (the quarter rule's border test), 'reflect' (padding), 'taps17' (the
    middle k of k = 17's taps, renormalised: 17's sigma at size k), 'no_log', 'dxy_sign'."""
    n, j, h, w = M.shape
    g = taps(k)
    if variant == 'taps17':
        g17 = taps(17); c = 8; r = (k - 1) // 2
        g = g17[c - r:c + r + 1] / g17[c - r:c + r + 1].sum()
    inside = inside_of(idx, h, w, loose=(variant == 'loose_border'))
    if variant == 'no_blur':
        B, bB = M, bound
    else:
        B, bB = blur64(M, g, 'reflect' if variant == 'reflect' else 'zero'), blur64(bound, g)
    a, c = np.arange(n)[:, None], np.arange(j)[None, :]
    py, px = idx // w, idx % w
    cl = lambda v, hi: np.clip(v, 0, hi - 1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        Bs = np.stack([B[a, c, cl(py + dy, h), cl(px + dx, w)] for dy, dx in SAMPLES])
        bs = np.stack([bB[a, c, cl(py + dy, h), cl(px + dx, w)] for dy, dx in SAMPLES])
        all_clamped = np.all(Bs + bs <= CLAMP, axis=0)
        none_clamped = np.all(Bs - bs > CLAMP, axis=0)
        L = Bs if variant == 'no_log' else np.log(np.maximum(Bs, CLAMP))
        e = np.where(Bs - bs > CLAMP, bs / np.where(Bs - bs > CLAMP, Bs - bs, 1.0), np.inf)
        gx, gy, dxx, dyy, dxy = _taylor(L)
        if variant == 'dxy_sign':
            dxy = -dxy
        det = dxx * dyy - dxy * dxy
        ok = inside & (det != 0) & np.isfinite(det)
        sdet = np.where(ok, det, 1.0)
        ox = np.where(ok, -(dyy * gx - dxy * gy) / sdet, 0.0)
        oy = np.where(ok, -(dxx * gy - dxy * gx) / sdet, 0.0)
        dg = np.maximum(0.5 * (e[1] + e[2]), 0.5 * (e[5] + e[6]))
        exx, eyy = 0.25 * (e[3] + 2.0 * e[0] + e[4]), 0.25 * (e[7] + 2.0 * e[0] + e[8])
        exy = 0.25 * (e[9] + e[10] + e[11] + e[12])
        dH = np.maximum(exx + exy, exy + eyy)
        inv = np.maximum(np.abs(dyy) + np.abs(dxy), np.abs(dxy) + np.abs(dxx)) / np.abs(sdet)
        den = 1.0 - inv * dH
        good = ok & none_clamped & (den > 0)
        bd = np.where(good, inv * (dg + dH * np.maximum(np.abs(ox), np.abs(oy))) / np.where(good, den, 1.0), np.inf)
    bd = np.where(~inside | (inside & all_clamped), 0.0, bd)
    decided = ~inside | (inside & all_clamped) | (good & (bd <= CAP))
    return dict(inside=inside, ox=ox, oy=oy, bound=bd, decided=decided)


# ---- the published steps, stated independently ----------------------------------------------------------------------------------------------
def official_dark(M, k):
    """The DARK post-processing as published (gaussian_blur + taylor of the authors' inference code) on float64 maps (n, 17, h, w): each
    map embedded in a zero frame of width (k - 1) / 2, blurred with OpenCV's Gaussian of size k and sigma 0 (here
    scipy.ndimage.correlate1d with the kernel getGaussianKernel(k, 0) would return, mode='constant'), cut back, rescaled by
    max(M) / max(B); then max(., 1e-10), log, and at the arg-max cell of the UNBLURRED map, where 1 < px < w - 2 and 1 < py < h - 2, the
    step -H^-1 g through a matrix inverse when dxx dyy - dxy^2 != 0.  -> coords (n, 17, 2) float64 (x, y) in cells."""
    from scipy.ndimage import correlate1d
    n, j, h, w = M.shape
    border = (k - 1) // 2
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
            origin_max = np.max(hm)
            dr = np.zeros((h + 2 * border, w + 2 * border))
            dr[border:-border, border:-border] = hm
            dr = correlate1d(correlate1d(dr, kern, axis=1, mode='constant', cval=0.0), kern, axis=0, mode='constant', cval=0.0)
            bl = dr[border:-border, border:-border].copy()
            bl *= origin_max / np.max(bl)
            lg = np.log(np.maximum(bl, 1e-10))
            px, py = int(coords[a, p, 0]), int(coords[a, p, 1])
            if 1 < px < w - 2 and 1 < py < h - 2:
                dx = 0.5 * (lg[py][px + 1] - lg[py][px - 1])
                dy = 0.5 * (lg[py + 1][px] - lg[py - 1][px])
                dxx = 0.25 * (lg[py][px + 2] - 2 * lg[py][px] + lg[py][px - 2])
                dxy = 0.25 * (lg[py + 1][px + 1] - lg[py - 1][px + 1] - lg[py + 1][px - 1] + lg[py - 1][px - 1])
                dyy = 0.25 * (lg[py + 2 * 1][px] - 2 * lg[py][px] + lg[py - 2 * 1][px])
                derivative = np.array([[dx], [dy]])
                hessian = np.array([[dxx, dxy], [dxy, dyy]])
                if dxx * dyy - dxy ** 2 != 0:
                    offset = -np.linalg.inv(hessian) @ derivative
                    coords[a, p] += offset[:, 0]
    return coords


# ---- inputs of the GPU tests --------------------------------------------------------------------------------------------------------------
def bias_lift(C):
    return 60.0 if C == 256 else 30.0


def _blob(h, w, cy, cx, sigma=2.0):
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma))


def dark_inputs(C, h, w, n, seed=SEED):
    """A feature batch of 2n + 1 rows for n crops: image_ref.head_inputs features scaled to 0.25, biases raised by bias_lift(C) so that
    every blurred sample is positive, and for each (crop, joint) a Gaussian blob (sigma 2 cells, gain 3) of sign(w[joint]) vectors at a
    seeded fractional centre anywhere in the map; the mirrored row n + i carries crop i's blobs mirrored (column w - 1 - cx, joint
    pair(j)), as the network's map of a mirrored crop would.  Rounded to bf16.  The spare row 2n holds 1e30 everywhere: a call that
    reads it into a result shows.  (N(0, 1) maps are useless here: their blurred values straddle 0 and their Hessians are near-singular.)
    -> feat (2n + 1, h, w, C) float32, wt, b, boxes (n, 4), centres (n, 17, 2) (cy, cx)."""
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    rng = np.random.default_rng([seed, C, h, w, n, 77])
    centres = rng.random((n, J, 2)) * np.array([h - 1.0, w - 1.0])
    f = 0.25 * feat.astype(np.float64)
    sg = np.sign(wt).astype(np.float64)
    for i in range(n):
        for j in range(J):
            cy, cx = centres[i, j]
            f[i] += 3.0 * _blob(h, w, cy, cx)[:, :, None] * sg[j][None, None, :]
            f[n + i] += 3.0 * _blob(h, w, cy, w - 1.0 - cx)[:, :, None] * sg[FR.PAIR[j]][None, None, :]
    feat = R.bf16_rne(f).astype(np.float32)
    spare = np.full((1, h, w, C), R.bf16_rne(1.0e30), dtype=np.float32)
    b = (b + np.float32(bias_lift(C))).astype(np.float32)
    return np.concatenate([feat, spare]), wt, b, boxes[:n], centres


def reference(feat, wt, b, n, flags, variant='ok'):
    """(M, bound) (n, 17, h, w) float64 of a call with `flags` on the batch of dark_inputs / planted_inputs."""
    hmP, bdP, hmF, bdF = FR.maps64(feat, wt, b, n)
    if not flags & 1:
        return hmP, bdP
    return FR.merge64(hmP, bdP, hmF, bdF, bool(flags & 2), variant)


def judge(pos_y, pos_x, idx, D, w, slack_y=0.0, slack_x=0.0):
    """The check of the GPU test, in cells: positions (n, 17) a decoder returned against dark64's result D at the cells idx.  Every
    decided case (outside cases included: offset 0, bound 0) must lie within its bound plus `slack` (the float32 rounding of the box
    mapping, when the positions come back through it); an undecided case with a finite bound within that bound -- the widest answer the
    derivation allows -- and with none, anywhere.  -> dict(cases, inside, undecided (inside cases), worst (error / allowance over the
    decided inside cases), wrong [(crop, joint, err_y, err_x, allowed)])."""
    ey = np.abs(pos_y - (idx // w + D['oy'])); ex = np.abs(pos_x - (idx % w + D['ox']))
    fin = np.isfinite(D['bound'])
    ay, ax = np.where(fin, D['bound'], np.inf) + slack_y, np.where(fin, D['bound'], np.inf) + slack_x
    with np.errstate(invalid='ignore', divide='ignore'):
        bad = ~((ey <= ay) & (ex <= ax))
        ins = D['inside'] & D['decided'] & (D['bound'] > 0)
        worst = float(np.maximum(ey / ay, ex / ax)[ins].max()) if ins.any() else 0.0
    wrong = [(int(a), int(c), float(ey[a, c]), float(ex[a, c]), float(D['bound'][a, c])) for a, c in zip(*np.nonzero(bad))]
    return dict(cases=int(idx.size), inside=int(D['inside'].sum()), undecided=int((D['inside'] & ~D['decided']).sum()), worst=worst, wrong=wrong)


def planted_inputs(h, w, k, flags, C=PLANT_C, seed=SEED):
    """One crop per single-purpose case of an (h, w) map decoded with blur size k and `flags`; rows [0, n) plain, [n, 2n) mirrored, one
    spare.  Background: head_inputs features scaled to 0.25, every bias + 30 except joint 7 (-inf: a map of -inf) and joints 9 and 10 (-30:
    strongly negative maps, merged or not).  Each case plants joint 5 (joint 9 for the spike) and stores what it pins:
      'px=K' / 'py=K'  a blob centred on the cell, K in {1, 2, w - 3, w - 2} / {1, 2, h - 3, h - 2}: both sides of the inside rule
      'centre'         a blob off the grid in the middle: the window spans a 256-pixel tile seam wherever the map has more than one tile,
                       and hangs over both map edges at once where 2 R + 5 exceeds the map (7 x 5 at k = 11; 33 x 17 at k = 17 -- at
                       k = 11 the window is 15 columns wide and fits into 17, so that map gets its two-sided case from k = 17)
      'last tile'      a blob two rows from the bottom: the winner lies in the last tile
      'plateau'        a square of identical feature vectors round the middle, large enough to hold the whole window of its centre.
                       The first maximum is the square's FIRST cell, so the decode runs there, on the square's corner (the tie rule
                       under the new finish kernel).  A flat window round the winner itself cannot be built: every cell of such a
                       window that precedes the winner in flat order would tie with it and win.  Exact zeros, determinant 0 and no
                       offset are pinned by the spike case instead.
      'spike'          joint 9: one cell far above 0 (about + 90, + 30 merged) on a map of about - 30: every blurred sample is negative, every logarithm is
                       log(1e-10), the determinant is 0 and there is no offset (the scale-free definition; the official rescaling
                       would turn the map's sign).  Pinned exactly.
      'mirror only'    (MERGE) a blob of joint 5 that only the mirrored crop carries: it shows in joint 6 at the column that reads it,
                       with or without the shift
    -> feat, wt, b, boxes, cases [(crop, name, expect)]."""
    R_ = (k - 1) // 2
    xs = FR.source_columns(w, bool(flags & 2))
    r, c = h // 2, w // 2
    names = (['px=%d' % v for v in sorted({1, 2, w - 3, w - 2})] + ['py=%d' % v for v in sorted({1, 2, h - 3, h - 2})] +
             ['centre', 'last tile', 'plateau', 'spike'] + (['mirror only'] if flags & 1 else []))
    n = len(names)
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    f = 0.25 * feat.astype(np.float64)
    sg = np.sign(wt).astype(np.float64)
    b = (b + np.float32(30.0)).astype(np.float32)
    b[7] = -np.inf
    b[9] = b[10] = np.float32(-30.0)                                   # (10 = pair(9): the merged map of joint 9 is negative as well)
    cases = []
    for i, name in enumerate(names):
        e = dict(joint=5)
        if name[:3] in ('px=', 'py='):
            v = int(name[3:])
            y, x = (r, v) if name[1] == 'x' else (v, c)
            f[i] += 3.0 * _blob(h, w, y, x)[:, :, None] * sg[5]
            e.update(cell=y * w + x, inside=bool(1 < x < w - 2 and 1 < y < h - 2))
        elif name == 'centre':
            cy, cx = r + 0.2, c - 0.2                                  # (gain 6: half of it is left after a merge with a blank mirror)
            f[i] += 6.0 * _blob(h, w, cy, cx)[:, :, None] * sg[5]
            e.update(cell=r * w + c, inside=bool(1 < c < w - 2 and 1 < r < h - 2), centre=(cy, cx))
        elif name == 'last tile':
            y = h - 3
            f[i] += 6.0 * _blob(h, w, y, c + 0.2)[:, :, None] * sg[5]
            e.update(cell=y * w + c, inside=bool(1 < c < w - 2 and 1 < y < h - 2), tile=(h * w - 1) // R.HEAD_TILE)
        elif name == 'plateau':
            half = min(R_ + 2, r - 2, c - 2)
            f[i, r - half:r + half + 1, c - half:c + half + 1] = 4.0 * sg[5]
            if flags & 1:                                              # the mirrored halves of the square's cells identical as well
                f[n + i, r - half:r + half + 1, xs[c - half:c + half + 1]] = 4.0 * sg[6]
            e.update(cell=(r - half) * w + (c - half), inside=bool(1 < c - half < w - 2 and 1 < r - half < h - 2))
        elif name == 'spike':
            f[i, r, c] = 16.0 * sg[9]
            e.update(joint=9, cell=r * w + c, inside=bool(1 < c < w - 2 and 1 < r < h - 2), zero=True)
        elif name == 'mirror only':
            kx = c - 1
            f[n + i] += 3.0 * _blob(h, w, r, kx)[:, :, None] * sg[5]
            cols = [x for x in range(w) if int(xs[x]) == kx]
            e.update(joint=6, among=[r * w + x for x in cols])
        cases.append((i, name, e))
    feat = R.bf16_rne(f).astype(np.float32)
    spare = np.full((1, h, w, C), R.bf16_rne(1.0e30), dtype=np.float32)
    return np.concatenate([feat, spare]), wt, b, boxes[:n], cases
