"""GPU: k_fuse_sum's units (csrc/pam_fuse.hip).  A workgroup takes 16 pixels of an anchor level L (a small rectangle that may hang over
the map's edge), each wave keeps its channel tile's 1x1 weights in registers, and the sum leaves through LDS.  Every (C, shifts) HRNet-W48 uses, with 0 / 1 / 2 plain terms (as many as k_upsample_add, the reference, takes beside
the sources), and maps that break the unit rectangle in every way,
each at every anchor level the entry point can be asked for (tile = (L, anything)) and at the library's own choice, must
equal bit for bit the launches the kernel replaces (one 1x1 convolution per source + k_upsample_add), inside sentinel bands.
Which kernel a launch takes is asked of pam_fuse_sum_plan for every case and tile and asserted: a named level is the register-weights
k_fuse_sum, the library's choice is the persistent k_fuse_sum_lds for every C = 192 case here (at most 64 units, or more than one per
CU) and for the 40-image C = 96 case under two sources (1 080 units), and k_fuse_sum everywhere else.  A (C, shifts) outside the table
of csrc/pam_fuse_plan.hpp is refused before a kernel is chosen, and nothing is written."""
import ctypes

import pytest
import torch
import torch.nn as nn

import pam
import guarded_mem as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipHRNet.__new__(hrnet_hip.HipHRNet)
    e.lib = _lib.load(); e.device = torch.device('cuda:0'); e.tile_cfg = -1
    return e


def _conv(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, cout, 1, 1, 0, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / cin) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
    return conv


def _cl(shape, seed, dev):
    """test_gpu_fuse's values in NHWC memory with exact channels-last strides (contiguous(memory_format=...) leaves a 1 x 1 map's strides
    as they are, which the launch helpers' stride checks do not take)"""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    buf = torch.empty((n, h, w, c), dtype=torch.bfloat16, device=dev)
    buf.copy_(torch.randn(shape, generator=g).to(torch.bfloat16).permute(0, 2, 3, 1))
    return buf.permute(0, 3, 1, 2)


# every (C, shifts) of the network + a lone source two levels down
COMBOS = [(48, (1,)), (48, (1, 2)), (48, (1, 2, 3)), (96, (1,)), (96, (1, 2)), (192, (1,)), (96, (2,))]

# n, coarsest map (rows, columns), c, shifts, plain terms, relu, plain terms as channel slices of a wider tensor
# (k_upsample_add, the reference, takes three terms: a sum of s sources has at most 3 - s plain terms, as in the network)
CASES = [(2, (5, 3), c, sh, npl, True, False) for c, sh in COMBOS for npl in (0, 1, 2) if npl + len(sh) <= 3]
CASES += [
    (2, (5, 3), 96, (1, 2), 1, True, True),             # channel-sliced plain terms, as the merged strided heads hand them over
    (2, (5, 3), 192, (1,), 2, True, True),
    (2, (5, 3), 48, (1, 2), 1, False, False),           # no ReLU
]
# maps against the unit rectangle (16 anchor pixels as 4 x 4, 2 x 8, 8 x 2, 1 x 16 or 16 x 1): a single coarsest pixel (every unit hangs
# over both edges at L = 1 .. 2), ragged in both directions, one row, one column, and the real 12 x 9.  The launcher rounds the grid to
# nothing (one workgroup per unit); 3 images of 5 x 3 are 45 units at L = 1 and 15 at L = 2, 3 of 12 x 9 are 324 and 81.
CASES += [(n, m, 48, (1, 2, 3), 0, True, False) for m in ((1, 1), (5, 3), (1, 7), (7, 1), (12, 9)) for n in (1, 3)]
# the sizes at which the library's own choice is the persistent kernel (more units than the dispatch's thresholds: 360 of C = 192, 1 080
# of C = 96 under two sources); a named level still runs the register-weights kernel there
CASES += [(40, (12, 9), 192, (1,), 2, True, False), (40, (12, 9), 96, (1, 2), 1, True, False)]


def _planned_kernel(eng, case, tile, max_wg=0):
    """Kernel (1 = k_fuse_sum, 2 = k_fuse_sum_lds) and level pam_fuse_sum_plan names for a case at this tile, on this device (n_cu = 0)."""
    n, (mh, mw), c, shifts, nplain = case[:5]
    k = len(shifts)
    out = (ctypes.c_int32 * 8)()
    rc = eng.lib.pam_fuse_sum_plan(n, mh << shifts[-1], mw << shifts[-1], c, nplain, k, (ctypes.c_int32 * k)(*shifts),
                                   (ctypes.c_int32 * k)(*[c << sh for sh in shifts]), tile[0], tile[1], max_wg, 0, out)
    assert rc == 0, (case, tile, rc)
    return out[0], out[1]


def _tiles(smax):
    """(L, 0) for every anchor level the entry point takes at this depth (it clamps L to min(2, coarsest shift)), then the library's
    choice and values the network's callers and tools pass (hints: any positive value is taken)"""
    return [(L, 0) for L in range(1, min(2, smax) + 1)] + [(0, 0), (1, 3), (2, 2), (7, 9)]


@pytest.mark.parametrize('case', CASES)
def test_fuse_sum_units_equal_the_launches_they_replace(eng, case):
    from pam import hrnet_hip
    n, (mh, mw), c, shifts, nplain, relu, sliced = case
    dev = eng.device
    smax = shifts[-1]
    h, w = mh << smax, mw << smax
    convs = [_conv(c << sh, c, 40 + sh + c) for sh in shifts]
    op = hrnet_hip.PackedUp(convs, shifts, dev)
    base = _cl((n, c, h, w), 3, dev)
    if sliced:
        wide = _cl((n, 2 * c + 16, h, w), 4, dev)
        plain = [wide[:, 8:8 + c], wide[:, 8 + c:8 + 2 * c]][:nplain]
    else:
        plain = [_cl((n, c, h, w), 11 + t, dev) for t in range(nplain)]
    srcs = [_cl((n, c << sh, h >> sh, w >> sh), 5 + sh, dev) for sh in shifts]
    tiles = _tiles(smax)
    # the library's choice: the persistent kernel for the sizes the docstring names, else (and at every named level) the register weights
    lds = 2 if (c == 192 or (n == 40 and len(shifts) == 2)) else 1
    for t in tiles:
        assert _planned_kernel(eng, case, t) == ((1, min(t[0], 2, smax)) if t[0] > 0 else (lds, 0 if lds == 2 else 1)), (case, t)
    assert _planned_kernel(eng, case, (0, 0), max_wg=5)[0] == lds, case
    eng._keep = []
    eng.arena = arena = G.GuardArena(dev, (len(tiles) + 4) * 2 * base.numel() + (1 << 20))
    try:
        packed = [hrnet_hip.PackedConv(cv, dev) for cv in convs]
        terms = [eng.conv(pk, s) for pk, s in zip(packed, srcs)]
        y0 = eng.upsample_add(base, plain + terms, [0] * nplain + list(shifts), relu=relu)       # the reference, computed once
        ys = [eng.fuse_sum(op, base, plain, srcs, relu=relu, tile=t) for t in tiles]
        ys.append(eng.fuse_sum(op, base, plain, srcs, relu=relu, max_wg=5))                        # a cap is accepted and changes nothing
    finally:
        eng.arena = None
    torch.cuda.synchronize()
    assert arena.report() == '', case                          # no write outside an output, nothing of an output left unwritten
    for t, y in zip(tiles + ['max_wg=5'], ys):
        assert torch.equal(y0, y), (case, t, (y0.float() - y.float()).abs().max().item())


@pytest.mark.parametrize('shifts', [(2,), (1, 2)])
def test_a_combination_outside_the_table_is_refused_where_the_size_used_to_pick_the_kernel_first(eng, shifts):
    """C = 192 with shifts (2) or (1, 2) on a 1-image 4 x 4 map: one unit, which is the persistent kernel's size for C = 192.  The
    combination is no row of the table, so the call raises and the output, carved out of sentinel memory, stays sentinel."""
    from pam import _lib, hrnet_hip
    dev, c, h, w = eng.device, 192, 4, 4
    op = hrnet_hip.PackedUp([_conv(c << sh, c, 40 + sh + c) for sh in shifts], shifts, dev)
    base = _cl((1, c, h, w), 3, dev)
    srcs = [_cl((1, c << sh, h >> sh, w >> sh), 5 + sh, dev) for sh in shifts]
    eng._keep = []
    eng.arena = arena = G.GuardArena(dev, 2 * base.numel() + (1 << 20))
    try:
        with pytest.raises(_lib.PamError):
            eng.fuse_sum(op, base, [], srcs, relu=True)
    finally:
        eng.arena = None
    torch.cuda.synchronize()
    assert [a['shape'] for a in arena.allocs] == [(1, c, h, w)]
    assert arena.violations() == [] and arena.unwritten() == [base.numel()]
