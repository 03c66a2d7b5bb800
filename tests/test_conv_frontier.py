"""CPU: pam_conv_plan at the sizes where the conv kernels' 32-bit address arithmetic ends (the frontier table).

Every kernel family and stated form of pam_conv2d_nhwc_bf16_ex is asked twice per operand: one image below the operand's frontier,
where the answer must be the (rc, kernel, form) of the same layer at the network's own batch, and at the first N on or beyond it, where
the call must be refused (PAM_E_ARG, outputs untouched) or land on a family whose table row can address it.  The frontiers are computed
here from the table's rule (bytes or counts per image), not read back from the library:

    input     k_conv_igemm / k_conv3x3 / k_conv_stem / k_conv_gs   N H W in_cstride 2 < 2^31   (padding tap = offset 2^31, int offsets)
              k_conv_igemm, pad 0 and KH KW Cin % 64 == 0          ... < 2^32                  (no padding offset is ever formed)
              k_conv3x3s                                            none (64-bit pointers); N H W < 2^31
    residual  every family                                          N Ho Wo Cout 2 < 2^32      (32-bit offsets, sentinel only on unstored rows)
    output    every family                                          none (64-bit pointers); N Ho Wo < 2^31; tile_cfg -7 / -8: < 2^31 bytes

Needs the built library, no GPU."""
import pytest

import conv_plan_cases as P
from test_conv_plan import K_3X3, K_3X3S, K_GS, K_IGEMM, K_STEM, _lib_cdll, plan

REFUSED = (-1, -99, -99)             # PAM_E_ARG, and the outputs still hold what the caller put there


def q(N, H, W, Cin, Cout, k, stride, pad, relu=1, tile=-1, in_cs=0, relu_from=0, w_img=0, res=0):
    return dict(zip(P.INTS + P.FLAGS, (N, H, W, Cin, Cout, k, k, stride, pad, relu, tile, in_cs or Cin, relu_from, 1, 1, w_img, res, 1)))


def out_hw(c):
    return (c['H'] + 2 * c['pad'] - c['KH']) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - c['KW']) // c['stride'] + 1


def in_bytes(c):
    return c['H'] * c['W'] * c['in_cstride'] * 2


def out_bytes(c):
    ho, wo = out_hw(c)
    return ho * wo * c['Cout'] * 2


def first_n(per_image, frontier):
    """the smallest N with N * per_image >= frontier"""
    return -(-frontier // per_image)


# id -> (query at the network's own N, the family it runs on there, [(operand, per-image amount, frontier, what happens from it on)])
# `above` is REFUSED or the kernel that takes over.
ROWS = {
    # the un-fused stem's second convolution (HRNet, 384 x 288 crops): 20 crops = the benchmark's batch
    # (the executor's automatic choice runs it on k_conv_gs, the classic code -2 on the implicit GEMM)
    'igemm-3x3s2-in': (q(20, 192, 144, 64, 64, 3, 2, 1, tile=-2), K_IGEMM, [('in', in_bytes, 2 ** 31, REFUSED)]),
    'gs-3x3s2-64-in': (q(20, 192, 144, 64, 64, 3, 2, 1), K_GS, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # layer1's 1x1 layers on the classic kernels (tile_cfg -2): no padding tap, K = 256 = 4 chunks -> the implicit GEMM is right to 2^32
    'igemm-1x1-in': (q(20, 96, 72, 256, 64, 1, 1, 0, tile=-2), K_IGEMM, [('in', in_bytes, 2 ** 32, REFUSED)]),
    # the same layer where the plan prefers k_conv_gs: from 2^31 bytes of input the implicit GEMM takes over, from 2^32 nothing does
    'gs-1x1-in': (q(20, 96, 72, 256, 64, 1, 1, 0, tile=8), K_GS, [('in', in_bytes, 2 ** 31, REFUSED)]),
    'gs-auto-1x1-in': (q(20, 96, 72, 256, 64, 1, 1, 0), None, [('in', in_bytes, 2 ** 31, K_IGEMM), ('in', in_bytes, 2 ** 32, REFUSED)]),
    # 64 -> 256 with the residual: the residual (= output size) reaches 2^32 while the input is at 1 GiB
    'igemm-1x1-res': (q(20, 96, 72, 64, 256, 1, 1, 0, tile=-2, res=1), K_IGEMM, [('res', out_bytes, 2 ** 32, REFUSED)]),
    'gs-1x1-res': (q(20, 96, 72, 64, 256, 1, 1, 0, tile=8, res=1), K_GS, [('res', out_bytes, 2 ** 32, REFUSED)]),
    # a 1x1 layer with a K tail (48 channels: the chunk's last 16 lanes load the padding offset) over a slice of a 144-channel tensor
    'igemm-sliced-in': (q(20, 96, 72, 48, 48, 1, 1, 0, tile=-2, in_cs=144), K_IGEMM, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # HRNet-W32's 32-channel outputs: the implicit GEMM's 32-channel slabs (24 crops: the batch from which its tile rule takes 128-pixel blocks)
    'igemm-out32-in': (q(24, 64, 48, 64, 32, 3, 1, 1), K_IGEMM, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # the detector's leaky strided layer on the classic kernels (5 views of 608 x 608)
    'general-3x3s2-in': (q(5, 608, 608, 32, 64, 3, 2, 1, relu=2, tile=-2), None, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # merged fuse-layer head on k_conv_gs's 96-channel slabs
    'gs-3x3s2-in': (q(20, 96, 72, 48, 96, 3, 2, 1), K_GS, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # the 48-channel branch's layers on k_conv3x3 (classic image)
    'c3-48-in': (q(20, 96, 72, 48, 48, 3, 1, 1, w_img=1, tile=-4), K_3X3, [('in', in_bytes, 2 ** 31, REFUSED)]),
    'c3-48-res-in': (q(20, 96, 72, 48, 96, 3, 1, 1, w_img=1, tile=-4, res=1), K_3X3, [('in', in_bytes, 2 ** 31, REFUSED)]),
    # layer1's 3x3 on k_conv3x3s: the input has no byte frontier, the pixel count has one
    'c3s-64-pixels': (q(20, 96, 72, 64, 64, 3, 1, 1, w_img=1, tile=-3), K_3X3S, [('pixels', lambda c: c['H'] * c['W'], 2 ** 31, REFUSED)]),
    # the deep branches on k_conv3x3s with a residual twice the input's size
    'c3s-192-res': (q(20, 24, 18, 192, 384, 3, 1, 1, w_img=1, tile=-3, res=1), K_3X3S, [('res', out_bytes, 2 ** 32, REFUSED)]),
    # tile_cfg -7 / -8: the stated streamed forms keep their output (and residual) below 2^31 bytes
    'c3s-gen-out': (q(5, 52, 52, 128, 128, 3, 1, 1, relu=2, w_img=1, tile=-7), K_3X3S, [('out', out_bytes, 2 ** 31, REFUSED)]),
    'c3s-small-out': (q(2, 24, 18, 192, 192, 3, 1, 1, w_img=1, tile=-8), K_3X3S, [('out', out_bytes, 2 ** 31, REFUSED)]),
    # the 8-channel first layers: HRNet's (stride 2, 64 channels) and Darknet's (stride 1, 32 channels, leaky)
    'stem-s2-in': (q(20, 384, 288, 8, 64, 3, 2, 1, w_img=1), K_STEM, [('in', in_bytes, 2 ** 31, REFUSED)]),
    'stem-s1-in': (q(5, 416, 416, 8, 32, 3, 1, 1, relu=2, w_img=1, tile=-2), K_STEM, [('in', in_bytes, 2 ** 31, REFUSED)]),
}


@pytest.fixture(scope='module')
def lib():
    return _lib_cdll()


def test_rows_run_on_the_family_they_name(lib):
    for name, (c, family, _) in ROWS.items():
        rc, kernel, _ = plan(lib, c)
        assert rc == 0 and (family is None or kernel == family), (name, rc, kernel)
    assert {f for _, f, _ in ROWS.values()} >= {K_IGEMM, K_3X3, K_3X3S, K_GS, K_STEM}


@pytest.mark.parametrize('name', sorted(ROWS))
def test_one_image_below_and_on_each_frontier(lib, name):
    c, _, operands = ROWS[name]
    at_home = plan(lib, c)
    assert at_home[0] == 0, at_home
    took_over = None
    for operand, per_image, frontier, above in sorted(operands, key=lambda o: o[2]):
        n = first_n(per_image(c), frontier)
        assert (n - 1) * per_image(c) < frontier <= n * per_image(c)
        below, on = plan(lib, dict(c, N=n - 1)), plan(lib, dict(c, N=n))
        # below: the network's own answer -- or, beyond an earlier frontier of this row, the family that took over there
        assert below == (at_home if took_over is None else took_over), (operand, n - 1, below, at_home, took_over)
        if above == REFUSED:
            assert on == REFUSED, (operand, n, on)
            # and it stays refused: twice as many images, and far beyond
            assert plan(lib, dict(c, N=2 * n)) == REFUSED and plan(lib, dict(c, N=64 * n)) == REFUSED, (operand, n)
        else:
            assert on[0] == 0 and on[1] == above, (operand, n, on)
            took_over = on


# the queries of the issue that the plan answered with rc = 0 before it knew the frontiers: (query, what is right)
ISSUE_QUERIES = [
    ('stem conv2 at 607 crops', q(607, 192, 144, 64, 64, 3, 2, 1), REFUSED),                    # in 2.001 GiB, padding taps
    ('stem conv2 at 607 crops, classic', q(607, 192, 144, 64, 64, 3, 2, 1, tile=-2), REFUSED),
    ('256->64 1x1 at 607 crops', q(607, 96, 72, 256, 64, 1, 1, 0, tile=-2), K_IGEMM),            # in 2.001 GiB, no padding offset: right to 4 GiB
    ('64->256 1x1 + residual at 607 crops', q(607, 96, 72, 64, 256, 1, 1, 0, tile=-2, res=1), K_IGEMM),   # residual 2.001 GiB < 4 GiB
    ('two 4096 x 4100 images, 1x1', q(2, 4096, 4100, 64, 64, 1, 1, 0, tile=-2), REFUSED),        # in 4.004 GiB
    ('48->48 3x3 at 3300 images', q(3300, 96, 72, 48, 48, 3, 1, 1, w_img=1), REFUSED),          # k_conv3x3, in 2.04 GiB
    ('stem at 1300 crops', q(1300, 384, 288, 8, 64, 3, 2, 1, w_img=1), REFUSED),                # k_conv_stem, in 2.14 GiB
    ('leaky 3x3 s2 at 100 views of 608', q(100, 608, 608, 32, 64, 3, 2, 1, relu=2, tile=-2), REFUSED),   # in 2.2 GiB
    ('N Ho Wo overflows an int', q(40000, 256, 256, 8, 64, 1, 1, 0, tile=-2), REFUSED),         # M = 2.6e9, in 39 GiB
]


@pytest.mark.parametrize('what,c,right', ISSUE_QUERIES, ids=[w for w, _, _ in ISSUE_QUERIES])
def test_queries_beyond_a_frontier(lib, what, c, right):
    got = plan(lib, c)
    if right == REFUSED:
        assert got == REFUSED, (what, got)
    else:
        assert got[0] == 0 and got[1] == right, (what, got)


def test_one_image_inside_which_the_frontier_falls(lib):
    """N = 1: 4096 x 4096 x 64 is exactly 2^31 bytes.  The 1x1 layer has no padding offset and runs; the 3x3 layer is refused, and no
    slicing over N could help it."""
    assert plan(lib, q(1, 4096, 4096, 64, 64, 1, 1, 0, tile=-2))[:2] == (0, K_IGEMM)
    assert plan(lib, q(1, 4096, 4096, 64, 64, 3, 1, 1, tile=-2)) == REFUSED
    assert plan(lib, q(1, 4096, 4096, 64, 64, 3, 1, 1, w_img=1, tile=-4)) == REFUSED             # k_conv3x3's input
    assert plan(lib, q(1, 4096, 4096, 64, 64, 1, 1, 0, tile=8)) == REFUSED                       # a stated k_conv_gs form: its int offsets


def test_int_products_of_the_host(lib):
    """N Ho Wo, N H W and N H W in_cstride are formed in 64 bits: counts that overflow an int are refused whatever the family, also
    where the bytes the layer itself reads (N H W Cin 2) are few."""
    # k_conv3x3s has no byte frontier on its input; its tile and pixel indices are ints
    c = q(20, 96, 72, 64, 64, 3, 1, 1, w_img=1, tile=-3)
    n = first_n(96 * 72, 2 ** 31)
    assert plan(lib, dict(c, N=n - 1))[:2] == (0, K_3X3S) and plan(lib, dict(c, N=n)) == REFUSED
    assert plan(lib, dict(c, N=2 ** 31 - 1)) == REFUSED                                          # N H W = 1.5e13
    # 8 of 4096 channels (sliced input): N H W Cin 2 is 1 MiB per image, the tensor the offsets run over 512 MiB per image
    c = q(1, 256, 256, 8, 64, 1, 1, 0, tile=-2, in_cs=4096)
    assert plan(lib, dict(c, N=3))[0] == 0 and plan(lib, dict(c, N=4)) == REFUSED and plan(lib, dict(c, N=16)) == REFUSED
    # 2^31 and 2^32 bytes exactly, and products beyond 2^63 / 2^64 bytes cannot wrap back below the frontier
    for n in (2 ** 15, 2 ** 16, 2 ** 20, 2 ** 30, 2 ** 31 - 1):
        assert plan(lib, q(n, 256, 256, 64, 64, 1, 1, 0, tile=-2)) == REFUSED, n
        assert plan(lib, q(n, 32767, 32767, 512, 64, 3, 1, 1, tile=-2)) == REFUSED, n


def test_host_slices_stay_below_the_frontiers():
    """ConvEngine.conv_slice: the images per launch of a call above a frontier -- every slice below all three, none empty, even."""
    from pam.engine import ConvEngine
    cases = [(607, 192 * 144 * 128, 0, 192 * 144), (1214, 96 * 72 * 128, 96 * 72 * 512, 96 * 72), (5000, 96 * 72 * 512, 96 * 72 * 512, 96 * 72),
             (20, 96 * 72 * 128, 0, 96 * 72), (3, 2 ** 31 - 16, 0, 2 ** 20), (1, 100, 100, 100)]
    for n, per_in, per_res, pix in cases:
        step = ConvEngine.conv_slice(n, per_in, per_res, pix)
        assert 1 <= step <= n and step * per_in < 2 ** 31 and step * per_res < 2 ** 32 and step * pix < 2 ** 31, (n, step)
        cap = min((2 ** 31 - 1) // per_in, (2 ** 32 - 1) // per_res if per_res else n, (2 ** 31 - 1) // pix)
        assert -(-n // step) == -(-n // min(cap, n)), (n, step, cap)                                 # as few launches as the frontiers allow
    assert ConvEngine.conv_slice(606, 192 * 144 * 128, 0, 192 * 144) == 606 and ConvEngine.conv_slice(607, 192 * 144 * 128, 0, 192 * 144) == 304
    from pam._lib import PamError
    with pytest.raises(PamError):
        ConvEngine.conv_slice(2, 2 ** 31, 0, 2 ** 20)
