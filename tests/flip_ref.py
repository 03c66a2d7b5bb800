"""Float64 restatement of the flip test (csrc/pam_head.hip: k_head_argmax_flip, k_argmax_finish_flip) with derived bounds, NumPy only:
the merge of a plain and a mirrored-back heat-map (merge64), the quarter-pixel offset of the official get_final_preds (quarter64), an
independent torch statement of the official steps (official_merge / official_offsets) and the inputs of tests/test_gpu_flip.py, so that
the CPU tests (tests/test_flip_ref.py) judge the same data the GPU tests run on.  Bounds come from image_ref.head64 (the float32 FMA
chain) plus the roundings the merge adds; nothing here is measured on a kernel."""
import numpy as np

import image_ref as R

J = R.J
U32 = R.U32
PAIR = np.array([0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15])     # COCO left/right
# image_ref.head_inputs seed of the random cases.  Seed 4 leaves no merged map undecided, but one of the 17 PLAIN maps (the flags-4 call,
# M = P) at C = 256, 7 x 5, one crop: more than the 1 % the tests allow.  Seed 5 leaves no map and no quarter-pixel sign undecided, merged
# with and without the shift and plain, in the float64 reference alone; tests/test_flip_ref.py asserts the share for this seed.
SEED = 5
FLIP_CHANNELS = (32, 48, 256)
FLIP_MAPS = ((7, 5), (33, 17), (64, 48), (96, 72))
FLIP_CROPS = (1, 3)
PLANT_MAPS = ((33, 17), (96, 72))
PLANT_C = 48


def source_columns(w, shift, variant='ok'):
    """xs[x]: the column of the mirrored crop's map that feeds column x of the merged map.  Without the shift w - 1 - x; with it
    w - x for x >= 1 and w - 1 at x = 0 (flipped[..., 1:] = flipped[..., :-1] after the flip-back: column 0 keeps its own value).
    variant (tests: deliberately wrong): 'other_direction' shifts left; 'x0_wrap' carries the rule of x >= 1 over to x = 0 as a circular
    shift would (column 0 reads the mirrored crop's column 0; w - x itself is outside the map there)."""
    x = np.arange(w)
    if not shift:
        return w - 1 - x
    if variant == 'other_direction':
        return np.where(x <= w - 2, w - 2 - x, 0)
    xs = np.where(x >= 1, w - x, w - 1)
    if variant == 'x0_wrap':
        xs[0] = 0
    return xs


def merge64(hmP, boundP, hmF, boundF, shift, variant='ok'):
    """hmP / hmF (n, 17, h, w) float64 maps of the plain / the mirrored crops with their FMA-chain bounds (image_ref.head64) ->
    (M, bound): M = 0.5 (P[j][y][x] + F[pair(j)][y][xs]), bound = 0.5 (boundP + boundF[pair][xs]) + 2^-24 |M| -- each float32 term lies
    within its bound, their float32 sum rounds once (2^-24 relative), the halving is exact.  variant 'no_swap' (tests) skips pair()."""
    w = hmP.shape[-1]
    xs = source_columns(w, shift, variant)
    jj = np.arange(J) if variant == 'no_swap' else PAIR
    with np.errstate(invalid='ignore'):
        M = 0.5 * (hmP + hmF[:, jj][..., xs])
        bound = 0.5 * (boundP + boundF[:, jj][..., xs]) + U32 * np.abs(M)
    return M, bound


def quarter64(M, bound, idx, strict=True):
    """The offset of the official get_final_preds at cells idx (n, 17) (flat) of maps M (n, 17, h, w): it applies only where
    1 < px < w - 1 and 1 < py < h - 1 (strict=False: <=, the wrong border test); then sign(M[py][px+1] - M[py][px-1]) along x and the
    same along y.  A sign is DECIDED when |difference| exceeds the two cells' bounds plus 2^-24 |difference| (the float32 subtraction).
    -> inside (n, 17) bool, sx, sy (n, 17) in {-1, 0, 1} (0 outside), dec_x, dec_y (n, 17) bool (True outside: the offset must be 0)."""
    n, j, h, w = M.shape
    py, px = idx // w, idx % w
    if strict:
        inside = (1 < px) & (px < w - 1) & (1 < py) & (py < h - 1)
    else:
        inside = (1 <= px) & (px <= w - 2) & (1 <= py) & (py <= h - 2)      # (the widest test that still reads inside the map)
    a, c = np.arange(n)[:, None], np.arange(j)[None, :]
    signs, decided = [], []
    for dy, dx in ((0, 1), (1, 0)):
        y0, x0 = np.clip(py - dy, 0, h - 1), np.clip(px - dx, 0, w - 1)
        y1, x1 = np.clip(py + dy, 0, h - 1), np.clip(px + dx, 0, w - 1)
        with np.errstate(invalid='ignore'):
            d = M[a, c, y1, x1] - M[a, c, y0, x0]
            tol = bound[a, c, y1, x1] + bound[a, c, y0, x0] + U32 * np.abs(d)
            s = np.where(d > 0, 1, np.where(d < 0, -1, 0))
            dec = np.abs(d) > tol
        signs.append(np.where(inside, s, 0)); decided.append(dec | ~inside)
    return inside, signs[0], signs[1], decided[0], decided[1]


# ---- the official steps, stated independently in torch (float64) --------------------------------------------------------------------------
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]


def official_merge(P, F, shift):
    """P, F torch (n, 17, h, w): flip_back (flip(3), then the joint pairs exchanged), the shift, the average."""
    import torch
    flipped = F.flip(3).clone()
    for a, b in FLIP_PAIRS:
        tmp = flipped[:, a].clone()
        flipped[:, a] = flipped[:, b]
        flipped[:, b] = tmp
    if shift:
        flipped[..., 1:] = flipped.clone()[..., :-1]
    return (P + flipped) * 0.5


def official_offsets(M):
    """get_final_preds up to the box mapping on torch maps M (n, 17, h, w): arg-max coordinates (x, y), then at floor(coord + 0.5)
    strictly inside, coords += sign(diff) * .25.  -> coords (n, 17, 2) float64 numpy (x, y)."""
    import math
    import torch
    n, j, h, w = M.shape
    flat = M.reshape(n, j, -1)
    idx = flat.argmax(2)
    coords = torch.stack([(idx % w).double(), (idx // w).double()], dim=2)
    for a in range(n):
        for p in range(j):
            hm = M[a][p]
            px = int(math.floor(coords[a][p][0] + 0.5))
            py = int(math.floor(coords[a][p][1] + 0.5))
            if 1 < px < w - 1 and 1 < py < h - 1:
                diff = torch.tensor([hm[py][px + 1] - hm[py][px - 1], hm[py + 1][px] - hm[py - 1][px]], dtype=torch.float64)
                coords[a][p] += torch.sign(diff) * .25
    return coords.numpy()


# ---- inputs of the GPU tests --------------------------------------------------------------------------------------------------------------
def flip_inputs(C, h, w, n, seed=SEED):
    """A feature batch of 2n + 1 rows: image_ref.head_inputs(C, h, w, 2n, seed) -- rows [0, n) plain, rows [n, 2n) mirrored -- and one
    spare row (a copy of the last) no call may decode.  -> feat (2n + 1, h, w, C), wt, b, boxes (n, 4)."""
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    return np.concatenate([feat, feat[-1:]]), wt, b, boxes[:n]


def maps64(feat, wt, b, n):
    """head64 of the plain rows [0, n) and the mirrored rows [n, 2n) as (n, 17, h, w) maps + bounds."""
    _, h, w, _ = feat.shape
    hm, bd = R.head64(feat[:2 * n], wt, b)
    hm, bd = hm.reshape(2 * n, J, h, w), bd.reshape(2 * n, J, h, w)
    return hm[:n], bd[:n], hm[n:], bd[n:]


def _vec(wt, joint, gain):
    return (gain * np.sign(wt[joint])).astype(np.float32)


def planted_inputs(h, w, shift, merged=True, C=PLANT_C, seed=SEED):
    """One crop per planted case of an (h, w) map, C channels; feature rows [0, n) plain, [n, 2n) mirrored, one spare.  The plants are
    feature vectors gain * sign(w[joint]) (image_ref.plant): identical vectors give identical float32 values, peaks stand far above
    the N(0, 1) rest.  shift: the column map the mirrored plants are placed for; merged=False places the neighbour plants for a call
    without the merge (flags 4).  Joint 7 has a bias of -inf.  In the crops named 'tie' the caller must use the weights of
    ``tie_weights`` (joint 6 = joint 5), which make a plain-fed and a mirror-fed cell tie exactly.
    -> feat, wt, b, boxes, cases [(crop, name, expect)] with expect a dict of what the case pins (joint, cell, offsets)."""
    xs = source_columns(w, shift)
    readers = lambda k: [x for x in range(w) if int(xs[x]) == k]   # the merged columns that read mirrored column k
    r, c = h // 2, w // 2
    names = (['mirror only c=%d' % k for k in (c - 2, 0, w - 1)] + ['tie'] + ['px=%d' % k for k in (1, 2, w - 2, w - 1)] +
             ['py=%d' % k for k in (1, 2, h - 2, h - 1)] + ['equal neighbours', 'mirror decides'])
    n = len(names)
    feat, wt, b, boxes = R.head_inputs(C, h, w, 2 * n, seed)
    b[7] = -np.inf
    P, F = feat[:n], feat[n:]
    peak, low = _vec(wt, 5, 8.0), _vec(wt, 5, 2.0)
    cases = []
    for i, name in enumerate(names):
        e = {}
        if name.startswith('mirror only'):
            k = int(name.split('=')[1])
            F[i, r, k] = peak                                  # F[5] peaks at column k -> M[6] peaks where xs == k, if any column reads k
            e = dict(joint=6, among=[r * w + x for x in readers(k)])      # (under the shift nobody reads column 0, two read w - 1)
        elif name == 'tie':
            A = 511 if h * w > 512 and 511 // w == 512 // w else 255           # a 256-pixel tile seam inside one row
            assert (A + 1) % R.HEAD_TILE == 0 and A // w == (A + 1) // w and xs[A % w] != xs[(A + 1) % w]
            ya, xa, xb = A // w, A % w, (A + 1) % w
            P[i, ya, xa] = peak                                # X from the plain crop at A ...
            F[i, ya, xs[xb]] = peak                            # ... and from the mirrored crop at A + 1 (joint 6 = joint 5 there)
            F[i, ya, xs[xa]] = P[i, ya, xb]                    # the other halves equal too: M[A] = .5 (X + Y), M[A + 1] = .5 (Y + X)
            e = dict(joint=5, cell=A, tie=A + 1)
        elif name.startswith('px=') or name.startswith('py='):
            k = int(name[3:])
            y, x = (r, k) if name[1] == 'x' else (k, c)
            P[i, y, x] = peak
            e = dict(joint=5, cell=y * w + x, inside=bool(1 < x < w - 1 and 1 < y < h - 1))
        elif name == 'equal neighbours':
            P[i, r, c] = peak; P[i, r, c - 1] = low; P[i, r, c + 1] = low
            if merged:
                F[i, r, xs[c - 1]] = low; F[i, r, xs[c + 1]] = low         # the mirrored halves of the two neighbours equal as well
            e = dict(joint=5, cell=r * w + c, dx=0)
        elif name == 'mirror decides':
            P[i, r, c] = peak; P[i, r, c - 1] = low; P[i, r, c + 1] = low   # equal in the plain crop ...
            F[i, r, xs[c + 1]] = _vec(wt, 6, 2.0); F[i, r, xs[c - 1]] = _vec(wt, 6, -2.0)     # ... ordered by the mirrored one alone
            e = dict(joint=5, cell=r * w + c, dx=1 if merged else 0)
        cases.append((i, name, e))
    return np.concatenate([feat, feat[-1:]]), wt, b, boxes[:n], cases


def tie_weights(wt, b):
    """Joint 6 computes what joint 5 computes: the merged joint 5 = 0.5 (P[5] + F[6]) then adds two values of ONE function."""
    wt, b = wt.copy(), b.copy()
    wt[6], b[6] = wt[5], b[5]
    return wt, b
