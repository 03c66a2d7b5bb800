"""Float64 restatements of the image-side kernels (csrc/pam_crop.hip, csrc/pam_head.hip) with DERIVED per-element tolerances, NumPy only, no GPU:
the crop kernel (preprocess64 / crop_check), the final 1x1 convolution (head64), the hard and soft arg-max decodes (argmax_check,
soft64) and the box mapping (decode64).  Nothing in a tolerance here is tuned against the kernels: each term is a rounding bound of a
number format or the sensitivity of the float64 reference itself to the roundings the float32 kernel may make.  tests/test_image_ref.py
checks the restatements against the older ones and shows that each tolerance rejects a deliberately wrong restatement; the GPU tests
(tests/test_gpu_image_shapes.py) take their inputs from the case builders at the end of this file, so both see the same data."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
J = 17
U32 = 2.0 ** -24                 # unit round-off of float32
HEAD_TILE = 256                  # pixels per workgroup of k_head / k_head_argmax
FINISH_GROUP = 8                 # tiles k_argmax_finish loads at a time
DECODE_TILE = 1024               # pixels per staging tile of k_decode_nhwc
AA_MAXT = 24                     # taps per axis of the antialias path


def f32(x):
    return np.asarray(x, dtype=np.float32)


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def bf16_ulp(x):
    """Spacing of bfloat16 (8 significant bits) at |x|."""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 7)


def bf16_bits_to_f64(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_rne(x):
    """float -> bfloat16 by round-to-nearest-even, returned as float64 (finite inputs)."""
    u = f32(x).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    return bf16_bits_to_f64(u.astype(np.uint32))


def bf16_trunc(x):
    """The wrong conversion: the low 16 bits dropped."""
    return bf16_bits_to_f64(f32(x).view(np.uint32) >> 16)


# ---- crop kernel ---------------------------------------------------------------------------------------------------------------------
def _axis_coords(b0, ext, o, half):
    """Sample coordinates of one axis as the kernel forms them, b0 + (i + 0.5) * (ext / o) - half, every operation rounded to float32
    (no FMA), and delta: 4 float32 ulps of the largest term -- the expression has two roundings after the product (one if the compiler
    contracts it into an FMA), each at most half an ulp of the largest term; 4 leaves room for the rounding of the scale itself."""
    sc = f32(ext) / f32(o)
    t = (np.arange(o, dtype=np.float32) + f32(0.5)) * sc
    c = f32(b0) + t
    if half:
        c = c - f32(half)
    delta = 4.0 * float(ulp32(max(abs(float(b0)), float(np.abs(t).max()), 0.5)))
    return c.astype(np.float64), float(sc), delta


def _bilinear_rows(s, size):
    """(o, size) weights of the 2-tap bilinear sample at coordinates s: clamp to the frame, border replicate."""
    s = np.clip(s, 0.0, size - 1.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, size - 1)
    f = s - i0
    w = np.zeros((s.size, size))
    r = np.arange(s.size)
    np.add.at(w, (r, i0), 1.0 - f)
    np.add.at(w, (r, i1), f)
    return w


def _triangle_rows(c, sc, b0, ext, size, max_taps=AA_MAXT, centred=True):
    """(o, size) normalised weights of the antialias path: frame pixels i inside the box rounded outwards (box arithmetic in float32),
    weight 1 - |i + 0.5 - c| / max(sc, 1); at most max_taps taps -- the ones nearest the centre (centred=False: the first max_taps,
    the one-sided cut the kernel once made).  A pixel with no positive tap gets an all-zero row (black)."""
    sup = max(sc, 1.0)
    lo = min(max(0, int(np.floor(f32(b0)))), size - 1)         # a box wholly outside keeps the nearest frame column / row (often at weight 0)
    hi = max(lo + 1, min(size, int(np.ceil(f32(b0) + f32(ext)))))
    i = np.arange(size)
    w = np.maximum(0.0, 1.0 - np.abs(i[None, :] + 0.5 - c[:, None]) / sup)
    w[:, :lo] = 0.0
    w[:, hi:] = 0.0
    pos = w > 0
    cnt = pos.sum(1)
    for r in np.nonzero(cnt > max_taps)[0]:
        x0 = int(np.argmax(pos[r])); x1 = size - int(np.argmax(pos[r][::-1]))
        s = min(max(int(np.floor(c[r] - 0.5 * max_taps + 0.5)), x0), x1 - max_taps) if centred else x0
        w[r, :s] = 0.0
        w[r, s + max_taps:] = 0.0
    tot = w.sum(1, keepdims=True)
    return np.where(tot > 0, w / np.where(tot > 0, tot, 1.0), 0.0), int(min(cnt.max(), max_taps))


def preprocess64(frames, view_of, boxes, resolution, antialias=False, half=0.5, swap=True, shift=0.0, centred=True):
    """k_preprocess_crops restated: per output pixel the bilinear sample (half-pixel centres, border replicate) of the box from the BGR
    uint8 frame -- with antialias the normalised triangle filter over the outward-rounded box -- then BGR->RGB, /255, (v - mean) / std.
    Coordinates come from the float32 boxes in float32; interpolation and normalisation are float64.
    -> (value, tol), both (n, 3, H, W) float64.  tol per pixel =
       half a bf16 ulp (at |value| + the terms below: the float32 value that is rounded may sit that far from the reference)
     + the change of the reference when its sample coordinate moves by +-delta along x, plus the same along y (delta: _axis_coords).
       Inside a 2 x 2 cell that is delta x the cell's slope; evaluated at the moved coordinate it takes the neighbour cell's slope where
       a cell edge lies within delta, and the loss of the last tap where a filter window ends within delta
     + 8 float32 ulps for the interpolation and normalisation, of the magnitude the float32 chain works at: |value| + (v/255 + mean) / std,
       the two terms whose difference the value is.  With antialias one more ulp per tap of the row accumulation (sum_x wx * pixel, at
       most 24 terms) and of the column accumulation (sum_y wy * row sum, at most 24): a float32 sum of n positive terms is within n
       ulps of its value.
    This departs from the issue's wording in two places, on purpose.  It says "8 float32 ulps of the value" and "half a bf16 ulp at the
    reference value".  (v/255 - mean) / std cancels where the pixel is near the mean: the float32 error there is a few ulps of the TERMS
    (and 0.485f is itself half an ulp off 0.485), not of their small difference, so a correct kernel cannot meet ulps of the value near
    zero; and the number the kernel rounds to bf16 is its own float32 value, which may lie in the next binade, so the half-ulp is taken
    at |value| + the other terms.  Both are bounds of the formats, not figures from a kernel, and the wrong restatements of
    test_image_ref.py are still rejected under them.
    half / swap / shift / centred exist for tests/test_image_ref.py only (deliberately wrong restatements)."""
    frames = np.asarray(frames); boxes = f32(boxes); view_of = np.asarray(view_of)
    H, W = resolution
    fh, fw = frames.shape[1], frames.shape[2]
    n = view_of.size
    val = np.empty((n, 3, H, W)); tol = np.empty((n, 3, H, W))
    for i in range(n):
        bx, by, bw, bh = [float(v) for v in boxes[i]]
        cx, scx, dx = _axis_coords(bx, bw, W, 0.0 if antialias else half)
        cy, scy, dy = _axis_coords(by, bh, H, 0.0 if antialias else half)
        cx = cx + shift
        taps = 0
        if antialias:
            rows = lambda c, ax: _triangle_rows(c, (scx, scy)[ax], (bx, by)[ax], (bw, bh)[ax], (fw, fh)[ax], centred=centred)
            (wx, tx), (wy, ty) = rows(cx, 0), rows(cy, 1)
            taps = tx + ty
            wxs = [rows(cx + d, 0)[0] for d in (-dx, dx)]; wys = [rows(cy + d, 1)[0] for d in (-dy, dy)]
        else:
            wx, wy = _bilinear_rows(cx, fw), _bilinear_rows(cy, fh)
            wxs = [_bilinear_rows(cx + d, fw) for d in (-dx, dx)]; wys = [_bilinear_rows(cy + d, fh) for d in (-dy, dy)]
        # only the frame rows / columns some weight touches
        ux = np.nonzero(sum([wx] + wxs).sum(0) > 0)[0]; uy = np.nonzero(sum([wy] + wys).sum(0) > 0)[0]
        x0, x1 = (int(ux[0]), int(ux[-1]) + 1) if ux.size else (0, 1)
        y0, y1 = (int(uy[0]), int(uy[-1]) + 1) if uy.size else (0, 1)
        sub = frames[int(view_of[i]), y0:y1, x0:x1].astype(np.float64)         # (h, w, 3) BGR
        hs, ws = sub.shape[:2]
        along_y = lambda w_, m: (w_[:, y0:y1] @ m.reshape(hs, -1)).reshape(H, -1, 3)                  # (h, X, 3) -> (H, X, 3)
        along_x = lambda w_, m: np.tensordot(m, w_[:, x0:x1], axes=([1], [1])).transpose(1, 0, 2)     # (Y, w, 3) -> (3, Y, W)
        v = along_x(wx, along_y(wy, sub))                                       # (3, H, W) BGR
        rowsum, colsum = along_y(wy, sub), along_x(wx, sub)                     # (H, w, 3), (3, h, W)
        slack = np.zeros_like(v)
        part = np.zeros_like(v)
        for w_ in wxs:
            part = np.maximum(part, np.abs(along_x(w_, rowsum) - v))
        slack += part
        part = np.zeros_like(v)
        for w_ in wys:
            part = np.maximum(part, np.abs(np.tensordot(w_[:, y0:y1], colsum, axes=([1], [1])).transpose(1, 0, 2) - v))
        slack += part
        if swap:
            v, slack = v[::-1], slack[::-1]
        out = (v / 255.0 - MEAN[:, None, None]) / STD[:, None, None]
        slack = slack / 255.0 / STD[:, None, None]
        mag = np.abs(out) + (v / 255.0 + MEAN[:, None, None]) / STD[:, None, None]
        t = slack + (8 + taps) * 2.0 * U32 * mag                       # float32 ulp = 2 * U32 relative
        val[i] = out
        tol[i] = 0.5 * bf16_ulp(np.abs(out) + t) + t
    return val, tol


def crop_check(got, val, tol):
    """got (float64 view of the kernel's bf16 output, (n, 3, H, W)) against preprocess64's (val, tol) -> (worst error / tolerance,
    number of elements out of tolerance)."""
    ratio = np.abs(np.asarray(got, dtype=np.float64) - val) / tol
    return float(ratio.max()), int((ratio > 1.0).sum())


# ---- head + decode -------------------------------------------------------------------------------------------------------------------
def head64(feat, w, b, channels=None):
    """feat (n, h, w, C) bf16 values as float, w (17, C), b (17,) float32 -> heat-maps (n, 17, h*w) float64 and the bound of a float32
    FMA chain of C + 1 terms per element, (C + 1) * 2^-24 * (|b| + sum_c |x_c w_c|).  channels: use only the first `channels` (tests)."""
    x = np.asarray(feat, dtype=np.float64); w = np.asarray(w, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    n, h, wd, C = x.shape
    k = C if channels is None else channels
    x = x.reshape(n, h * wd, C)
    with np.errstate(invalid='ignore'):
        hm = np.einsum('npc,jc->njp', x[:, :, :k], w[:, :k]) + b[None, :, None]
        bound = (C + 1) * U32 * (np.einsum('npc,jc->njp', np.abs(x), np.abs(w)) + np.abs(b)[None, :, None])
    return hm, bound


def argmax_check(hm, bound, got):
    """hm, bound (n, 17, P) float64, got (n, 17) flat indices the kernel returned.  Cell k can hold the float32 maximum only when
    hm[top] - hm[k] <= bound[top] + bound[k] (each float32 value lies within its bound of the float64 one; 'twice the bound').  A map is
    DECIDED when no cell but the float64 maximum can -- cells that equal the maximum exactly (engineered ties: identical feature
    vectors, so identical float32 values too) count as the maximum, and the first of them is the answer.  Decided maps must match
    exactly; an undecided map must return one of the possible cells.  A map of -inf decodes as cell 0 (np.argmax).
    -> dict(maps, undecided, wrong: [(crop, joint, got, want)])."""
    n, j, P = hm.shape
    wrong, undecided = [], 0
    for a in range(n):
        for c in range(j):
            m = hm[a, c]
            top = int(np.argmax(m))
            g = int(got[a, c])
            if not np.isfinite(m[top]):
                if g != top:
                    wrong.append((a, c, g, top))
                continue
            cand = np.nonzero(m[top] - m <= bound[a, c, top] + bound[a, c])[0]
            if np.all(m[cand] == m[top]):
                if g != top:
                    wrong.append((a, c, g, top))
            else:
                undecided += 1
                if g not in cand:
                    wrong.append((a, c, g, top))
    return dict(maps=n * j, undecided=undecided, wrong=wrong)


def last_index_argmax(hm):
    """The wrong tie rule: the LAST maximum."""
    P = hm.shape[-1]
    return P - 1 - np.argmax(hm[..., ::-1], axis=-1)


def soft64(hm, beta, h, w):
    """Soft-arg-max of (n, 17, h*w) float64 maps: expected (row, column) under softmax(beta * map), and the maximum."""
    m = hm.max(-1, keepdims=True)
    p = np.exp(beta * (hm - m))
    p /= p.sum(-1, keepdims=True)
    idx = np.arange(h * w)
    return (p * (idx // w)).sum(-1), (p * (idx % w)).sum(-1), m[..., 0]


def soft_slack(hm, bound, beta, h, w):
    """How far (row, column) of soft64 can move, in cells, when every value of the float64 map moves by at most its float32 bound: the
    kernel's softmax runs on float32 sums, each within `bound` of the float64 one.  Along v + t e, |e_k| <= eps_k:
        d E[y] / dt = beta * sum_k p_k(t) (y_k - E_t[y]) e_k,   p_k(t) <= p_k exp(2 beta eps_max),
    so |delta E[y]| <= S / (1 - g) with S = beta exp(2 beta eps_max) sum_k p_k |y_k - E[y]| eps_k and g = beta eps_max exp(2 beta eps_max)
    (the term for the moving mean); infinite when g >= 1.  -> (slack_y, slack_x), each (n, 17).  Nothing here is measured on a kernel."""
    with np.errstate(over='ignore', invalid='ignore'):
        m = hm.max(-1, keepdims=True)
        p = np.exp(beta * (hm - m))
        p /= p.sum(-1, keepdims=True)
        idx = np.arange(h * w)
        emax = bound.max(-1)
        amp = np.exp(np.minimum(2.0 * beta * emax, 700.0))
        g = beta * emax * amp
        out = []
        for pos in (idx // w, idx % w):
            mean = (p * pos).sum(-1, keepdims=True)
            S = beta * amp * (p * np.abs(pos - mean) * bound).sum(-1)
            out.append(np.where(g < 1.0, S / np.where(g < 1.0, 1.0 - g, 1.0), np.inf))
    return out[0], out[1]


def decode64(py, px, boxes, h, w):
    """Box mapping of selfcheck.reference_decode: float64 arithmetic, one float32 rounding -> (y, x) float64."""
    b = np.asarray(f32(boxes), dtype=np.float64)
    y = f32(np.asarray(py, dtype=np.float64) / h * b[:, 3:4] + b[:, 1:2]).astype(np.float64)
    x = f32(np.asarray(px, dtype=np.float64) / w * b[:, 2:3] + b[:, 0:1]).astype(np.float64)
    return y, x


# ---- the inputs of the GPU tests (and of the CPU tests that show the checks reject wrong code on them) --------------------------------
HEAD_CHANNELS = (32, 48, 256)               # HRNet-W32, HRNet-W48, PoseResNet
HEAD_MAPS = ((64, 48), (96, 72), (7, 5), (33, 17))
HEAD_CROPS = (1, 5, 20)
DECODE_MAPS = HEAD_MAPS + ((41, 27),)
SOFT_BETAS = (0.7, 4.0, 25.0)


def head_inputs(C, h, w, n, seed=0):
    """Seeded N(0,1) bf16 features (n, h, w, C) as float32, weights 0.2 N(0,1) (17, C), bias N(0,1), boxes xywh in [20, 320)."""
    rng = np.random.default_rng([seed, C, h, w, n])
    feat = bf16_rne(rng.standard_normal((n, h, w, C))).astype(np.float32)
    wt = (0.2 * rng.standard_normal((J, C))).astype(np.float32)
    b = rng.standard_normal(J).astype(np.float32)
    boxes = (rng.random((n, 4)) * 300 + 20).astype(np.float32)
    return feat, wt, b, boxes


def head_case_inputs(C, h, w, n, seed=0):
    """The inputs of the (C, map, n) head case of the GPU tests: at n = 5 the feature batch holds 7 crops (the calls cover the first 5)."""
    return head_inputs(C, h, w, 7 if n == 5 else n, seed)


def plant(feat, wt, crop, joint, pixels, gain=8.0):
    """Give the listed flat pixels of one crop the SAME feature vector, gain * sign(w[joint]): an exact tie of that joint's map at a
    value (b + gain * sum |w|) far above the random rest, in float64 and in the kernel alike."""
    n, h, w, C = feat.shape
    v = (gain * np.sign(wt[joint])).astype(np.float32)
    for p in pixels:
        feat[crop, p // w, p % w] = v


def seam_pairs(P, tile, groups=(0, 7, 15)):
    """(last pixel of tile t, first of tile t + 1) for the tiles t that have a successor; then (a pixel of tile 0, one of the last tile)."""
    tiles = (P + tile - 1) // tile
    out = [((t + 1) * tile - 1, (t + 1) * tile) for t in groups if t + 1 < tiles]
    if tiles > 1:
        out.append((3, P - 2))
    return out


def seam_inputs(C, h, w, seed=2):
    """One crop per planted case of a (h, w) map, joint 5 carrying the plant: the seam ties of seam_pairs (256-pixel tiles), then a
    unique maximum in the last pixel.  In every crop joint 3 has a zero weight row (constant map = its bias), joint 7 a bias of -inf
    (a map of -inf) and joint 9 a bias of -3e30 (every value rounds to -3e30 in float32: a constant map below -1e30).
    (Seed 2: with seed 1 the float64 reference alone leaves one of the 68 maps of C = 256 at 64 x 48 undecided, more than the 1 % the
    tests allow; test_image_ref.py asserts the share for this seed.)
    -> feat, wt, b, boxes, cases [(crop, name, pixels)]."""
    P = h * w
    pairs = seam_pairs(P, HEAD_TILE)
    cases = [(k, 'tie %d|%d' % p, p) for k, p in enumerate(pairs)] + [(len(pairs), 'last pixel', (P - 1,))]
    feat, wt, b, boxes = head_inputs(C, h, w, len(cases), seed)
    wt[3] = 0.0
    b[7] = -np.inf
    b[9] = -3.0e30
    for crop, _, px in cases:
        plant(feat, wt, crop, 5, px)
    return feat, wt, b, boxes, cases


def decode_inputs(h, w, seed=2):
    """Seeded N(0,1) float32 heat-maps (n, 17, h*w), one crop per planted case of joint 5 (value 9: above every N(0,1) draw): ties across
    the 1024-pixel tiles of k_decode_nhwc, across the 64-lane waves inside a tile (63|64, 255|256), tile 0 against the last tile, a
    unique maximum in the last pixel.  Joint 3 is constant, joint 7 all -inf, joint 9 all -3e30.  -> hm, boxes, cases."""
    P = h * w
    pairs = [p for p in [(63, 64), (255, 256)] if p[1] < P] + seam_pairs(P, DECODE_TILE, groups=(0, 1, 5))
    cases = [(k, 'tie %d|%d' % p, p) for k, p in enumerate(pairs)] + [(len(pairs), 'last pixel', (P - 1,))]
    n = max(len(cases), 2)                               # two crops at least: the second one's base address (41 x 27: misaligned)
    rng = np.random.default_rng([seed, h, w])
    hm = rng.standard_normal((n, J, P)).astype(np.float32)
    hm[:, 3] = 0.25
    hm[:, 7] = -np.inf
    hm[:, 9] = -3.0e30
    for crop, _, px in cases:
        hm[crop, 5, list(px)] = 9.0
    boxes = (rng.random((n, 4)) * 300 + 20).astype(np.float32)
    return hm, boxes, cases


def noise_frames(v, fh, fw, seed):
    """BGR frames whose left half is smooth (a slow sinusoid per channel: the coordinate slack is small there, so a small shift in a
    smooth region has to show against half a bf16 ulp) and whose right half is uniform noise (large local slopes, every rounding case).
    Frames narrower than 8 pixels are noise only."""
    rng = np.random.default_rng([seed, fh, fw])
    fr = rng.integers(0, 256, (v, fh, fw, 3), dtype=np.uint8)
    if fw >= 8:
        y, x, c = np.arange(fh)[:, None, None], np.arange(fw // 2)[None, :, None], np.arange(3)[None, None, :]
        smooth = 128.0 + 100.0 * np.sin(x / 41.0 + 1.3 * c) * np.cos(y / 57.0 + 0.7 * c)
        fr[:, :, :fw // 2] = np.rint(smooth).astype(np.uint8)[None]
    return fr


# (name, frame (h, w), views, boxes xywh); every list ends with the degenerate boxes of the issue where the frame allows them
CROP_CASES = [
    ('288x360', (288, 360), 3, [[10, 20, 100, 200], [-15.5, -8.25, 120, 260], [300, 200, 90, 120], [0, 0, 360, 288],     # test_preprocess_vs_torch
                               [57, 101, 1, 1], [-400, 30, 100, 200], [40, 500, 80, 120], [259.5, 87.75, 100.5, 200.25],
                               [33.3, 44.7, 17.9, 23.1]]),
    ('1080x1920', (1080, 1920), 3, [[-40.5, -25.25, 300, 420], [1700, 800, 400, 500], [900.3, -60, 210.7, 380], [-10, 500, 180, 700],
                                   [0, 0, 1920, 1080], [1000.5, 400.25, 96.5, 130.75], [1919, 1079, 30, 30],               # the HD test's list
                                   [1500, 700, 1, 1], [-900, 100, 300, 420], [100, 1300, 200, 300], [1620, 660, 300, 420],
                                   [512.37, 300.61, 255.19, 411.83]]),
    ('5x2', (5, 2), 2, [[0, 0, 2, 5], [0.25, 1.5, 1.5, 2.75], [1, 4, 1, 1], [-7, 0, 3, 5], [0, 9, 2, 3]]),
    ('4x1', (4, 1), 2, [[0, 0, 1, 4], [0, 1.25, 1, 2.5], [0, 3, 1, 1], [-5, 0, 2, 4], [0, 6, 1, 2]]),
    ('9x7', (9, 7), 3, [[0, 0, 7, 9], [1.5, 2.25, 4.75, 5.5], [6, 8, 1, 1], [3, 3, 1, 1], [-20, 1, 6, 6], [2, 15, 4, 4], [4, 5, 3, 4]]),
]
# antialias: fractional boxes, boxes leaving the frame or wholly outside it; aa_limit_case: down-scaling up to the 11.5 the tap window holds
# and beyond it (13 x)
AA_FRAME = (5200, 3800)
AA_CASES = [
    ('aa 1080x1920', (1080, 1920), 2, [[100, 50, 600, 900], [700, 0, 432, 1080], [400, 300, 150, 200], [1500, 600, 400, 300],  # the existing test's list
                                      [100.3, 50.7, 600.4, 900.9], [-120.5, -80.25, 700, 1000], [1500.5, 700.5, 800, 900],
                                      [10.5, 20.25, 57.3, 91.7],
                                      [1920.2, 300, 90, 200], [2400, 100, 600, 900], [500, 1080.4, 120, 150], [300, 1500, 700, 1000],   # wholly right / below
                                      [-300, 200, 120, 260], [-2000, 100, 700, 900]]),                                                 # wholly left
]


def aa_limit_case(resolution, scale=11.45):
    """One box down-scaled by `scale` along x only, one along y only (the other axis by 2), on one large frame.  11.45 is just inside
    the 11.5 the 24-tap window holds; 13 is beyond it (27 taps wanted)."""
    H, W = resolution
    return ('aa x%g %dx%d' % (scale, H, W), AA_FRAME, 1, [[20.5, 10.25, scale * W, 2.0 * H], [300.25, 30.5, 2.0 * W, scale * H]])


def crop_case_inputs(case, seed=7):
    name, (fh, fw), v, boxes = case
    frames = noise_frames(v, fh, fw, seed)
    boxes = np.asarray(boxes, dtype=np.float32)
    view_of = (np.arange(len(boxes)) % v).astype(np.int32)
    return frames, view_of, boxes
