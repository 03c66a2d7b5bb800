"""What pam_spp_concat_nhwc_bf16 promises (include/pam.h), restated on the CPU for its tests (test infrastructure: nothing under the package
imports this): the contract as explicit loops, the kernel's decomposition as a model with its pitfalls as switches, the planted inputs and
the comparison rule.

``loop_spp`` is the contract: per output pixel the maximum over the window cut to the image, float64, written without torch's pooling.
``cascade_spp`` is how the kernel gets there: a separable radius-r1 pool, then each larger window as the union of smaller ones at a few
offsets, every tap position clamped to the map.  Its switches (skip instead of clamp) and loop_spp's (window start, channel order) are the
mistakes the tests must tell apart from the contract."""
import numpy as np
import torch

# (H, W): maps smaller than the windows, non-square maps, the networks' own maps (320 / 416 / 608 inputs), the kernel's limit
MAPS = [(1, 1), (3, 2), (6, 6), (8, 13), (13, 8), (10, 10), (13, 13), (19, 19), (32, 32)]
# (N, C, H, W, sizes): every map at C = 24 (no multiple of a 16- / 32- / 64-channel slab) and three views, the two 512-channel network
# shapes at five views, one 16-byte vector of channels, and other sizes (window 7 from window 3 takes three taps, not two) on two maps
CASES = ([(3, 24, h, w, (5, 9, 13)) for h, w in MAPS] +
         [(5, 512, 13, 13, (5, 9, 13)), (5, 512, 19, 19, (5, 9, 13)), (1, 8, 13, 13, (5, 9, 13)), (1, 8, 6, 6, (5, 9, 13)),
          (3, 24, 13, 13, (3, 7, 11)), (3, 24, 8, 13, (3, 7, 11))])
CASE_IDS = ['n%d-c%d-%dx%d-%s' % (n, c, h, w, '_'.join(str(s) for s in sz)) for n, c, h, w, sz in CASES]
BIG = 8192.0                # above every normal draw; exact in bf16


def planted_input(n, c, h, w, seed):
    """(n, c, h, w) bf16: seeded normals, a few -inf pixels, and on ten channels spread over c (two of them may coincide when c = 8): the global
    maximum in each corner and in the middle of each edge, one all -inf channel, one constant channel (ties everywhere)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c, h, w), generator=g)
    for _ in range(4):
        i = [int(torch.randint(0, d, (1,), generator=g)) for d in (n, c, h, w)]
        x[i[0], i[1], i[2], i[3]] = float('-inf')
    ch = [k * c // 10 for k in range(10)]
    spots = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    for k, (yy, xx) in enumerate(spots):
        x[:, ch[k], yy, xx] = BIG
    x[:, ch[9]] = 0.375
    x[:, ch[8]] = float('-inf')
    return x.to(torch.bfloat16)


def torch_spp(x, sizes):
    """The reference the issue names: yolov3.darknet_maxpool + cat, (n, c, h, w) float -> (n, 4c, h, w)."""
    from pam import yolov3
    a, b, c = sizes
    return torch.cat([yolov3.darknet_maxpool(x, c, 1), yolov3.darknet_maxpool(x, b, 1), yolov3.darknet_maxpool(x, a, 1), x], 1)


def loop_spp(x, sizes, start='half', order='c b a x'):
    """x: (n, c, h, w) float64 ndarray.  out[:, :, y, x] of a pool of size s = max over rows y + o .. y + o + s - 1 and columns alike, cut
    to the image, with o = -(s - 1) / 2 (start='half'; 'full': o = -(s - 1), a mistake).  Channels: pool c, pool b, pool a, x."""
    n, c, h, w = x.shape
    pools = {}
    for name, s in zip('abc', sizes):
        o = -((s - 1) // 2) if start == 'half' else -(s - 1)
        out = np.full((n, c, h, w), -np.inf)
        for y in range(h):
            for xx in range(w):
                m = out[:, :, y, xx]
                for ty in range(max(y + o, 0), min(y + o + s, h)):
                    for tx in range(max(xx + o, 0), min(xx + o + s, w)):
                        m = np.maximum(m, x[:, :, ty, tx])
                out[:, :, y, xx] = m
        pools[name] = out
    pools['x'] = x
    return np.concatenate([pools[k] for k in order.split()], 1)


def taps(rs, rt):
    """Offsets of the radius-rs windows whose union is the radius-rt window (the kernel's spp_taps)."""
    d, k = rt - rs, (2 * rt + 2 * rs + 1) // (2 * rs + 1)
    return [-d + (2 * d * j) // (k - 1) for j in range(k)]


def cascade_spp(x, sizes, clamp=True):
    """The kernel's decomposition on (n, c, h, w) float64: rows then columns at radius r1, then P2 from P1 and P3 from P2 at taps(.) in
    both directions.  clamp=False skips a tap that falls outside the map instead of clamping its position (a mistake: border columns are lost)."""
    n, c, h, w = x.shape
    r1, r2, r3 = [s // 2 for s in sizes]
    t = np.full(x.shape, -np.inf)
    for xx in range(w):
        for tx in range(max(xx - r1, 0), min(xx + r1, w - 1) + 1):
            t[:, :, :, xx] = np.maximum(t[:, :, :, xx], x[:, :, :, tx])
    p1 = np.full(x.shape, -np.inf)
    for y in range(h):
        for ty in range(max(y - r1, 0), min(y + r1, h - 1) + 1):
            p1[:, :, y] = np.maximum(p1[:, :, y], t[:, :, ty])

    def level(src, offs):
        out = np.full(x.shape, -np.inf)
        for y in range(h):
            for xx in range(w):
                for oy in offs:
                    for ox in offs:
                        ty, tx = y + oy, xx + ox
                        if clamp:
                            ty, tx = min(max(ty, 0), h - 1), min(max(tx, 0), w - 1)
                        elif not (0 <= ty < h and 0 <= tx < w):
                            continue
                        out[:, :, y, xx] = np.maximum(out[:, :, y, xx], src[:, :, ty, tx])
        return out
    p2 = level(p1, taps(r1, r2))
    p3 = level(p2, taps(r2, r3))
    return np.concatenate([p3, p2, p1, x], 1)


def bits(t):
    """bf16 tensor -> its 16-bit patterns (int16)."""
    return t.contiguous().view(torch.int16)


def same_up_to_zero_sign(got, want):
    """bf16 tensors: every element of got has want's bits, or both are zeros (of either sign)."""
    g, w = bits(got), bits(want)
    return (g == w) | (((g & 0x7fff) == 0) & ((w & 0x7fff) == 0))
