"""GPU: the HRNet-W32 convolution forms against fp32 F.conv2d (bf16-rounded weights, fp32 bias) at the W32 shapes of 256 x 192 crops
(branches 64x48 / 32x24 / 16x12 / 8x6) for 1, 5 and 20 crops -- 32-channel outputs on k_conv3x3<32> and on the implicit GEMM with
32-channel slabs, 3x3 stride 2, the 1x1 up-convolutions, the 224-channel merged up-convolution, transition1 (256 -> 32), sliced inputs
with a partial activation -- and the fused 32-channel BasicBlock (k_bblock2_32): bit-identical to its two k_conv3x3<32> launches at the
library's tile and at tiles that leave ragged last items, and close to the fp32 torch BasicBlock on calibrated weights."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import hrnet_calibrated_w as HW

pytestmark = pytest.mark.gpu

CROPS = [1, 5, 20]
DEV = torch.device('cuda:0')


def engine():
    from pam import _lib
    from pam.hrnet_hip import ConvEngine
    e = ConvEngine()
    e.lib = _lib.load()
    return e


def bf(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def make_conv(cin, cout, k, stride, seed):
    g = torch.Generator().manual_seed(seed)
    c = nn.Conv2d(cin, cout, k, stride, k // 2, bias=True)
    with torch.no_grad():
        c.weight.copy_((torch.randn(c.weight.shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5).to(torch.bfloat16).float())
        c.bias.copy_(0.2 * torch.randn(cout, generator=g))
    return c


def ref_conv(c, x, res=None, relu=False, relu_from=0):
    y = F.conv2d(x.float(), c.weight.to(x.device), c.bias.to(x.device), c.stride, c.padding)
    if res is not None:
        y = y + res.float()
    if relu:
        y = torch.cat([y[:, :relu_from], torch.relu(y[:, relu_from:])], 1)
    return y


def check(got, ref, what):
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(ref.shape), what
    g, r = got.float(), ref.float()
    rel = float((g - r).norm() / r.norm())
    worst = float((g - r).abs().max())
    assert rel < 4e-3 and worst <= 0.02 * float(r.abs().max()) + 1e-2, (what, rel, worst)


# (name, cin, cout, k, stride, H, W): the layers of HRNet-W32 whose output width is a multiple of 32 only, plus the stride-2 32 -> 64 step
LAYERS = [('3x3 32->32 (branch 0)', 32, 32, 3, 1, 64, 48),
          ('3x3 s2 32->32 (down chain)', 32, 32, 3, 2, 64, 48),
          ('3x3 s2 32->64 (down chain)', 32, 64, 3, 2, 64, 48),
          ('1x1 64->32 (up)', 64, 32, 1, 1, 64, 48),
          ('1x1 128->32 (up)', 128, 32, 1, 1, 64, 48),
          ('1x1 256->32 (up)', 256, 32, 1, 1, 64, 48),
          ('1x1 256->224 (merged up)', 256, 224, 1, 1, 8, 6),
          ('3x3 256->32 (transition1)', 256, 32, 3, 1, 64, 48)]


@pytest.mark.parametrize('n', CROPS)
@pytest.mark.parametrize('layer', LAYERS, ids=[l[0] for l in LAYERS])
def test_w32_layers_vs_fp32(layer, n):
    from pam.hrnet_hip import PackedConv
    name, cin, cout, k, stride, h, w = layer
    e = engine()
    c = make_conv(cin, cout, k, stride, seed=cin * 7 + cout + k + stride)
    op = PackedConv(c, DEV)
    x = bf(torch.randn((n, cin, h, w), generator=torch.Generator().manual_seed(n + cin)).to(DEV))
    for relu in (False, True):
        check(e.conv(op, x, relu=relu), ref_conv(c, x, relu=relu), (name, n, relu))
    if stride == 1 and cin == cout:
        res = bf(torch.randn((n, cout, h, w), generator=torch.Generator().manual_seed(3)).to(DEV))
        for relu in (False, True):
            check(e.conv(op, x, res=res, relu=relu), ref_conv(c, x, res=res, relu=relu), (name, n, 'res', relu))


@pytest.mark.parametrize('n', CROPS)
def test_3x3_32_classic_and_generic_forms(n):
    """The branch-0 layer on k_conv3x3<32> (automatic choice) and forced onto the implicit GEMM's two 32-channel tiles (tile_cfg 0 / 2),
    with and without residual and ReLU; the classic form is the one the library reports."""
    from pam.hrnet_hip import PackedConv
    e = engine()
    c = make_conv(32, 32, 3, 1, seed=5)
    op = PackedConv(c, DEV)
    x = bf(torch.randn((n, 32, 64, 48), generator=torch.Generator().manual_seed(n)).to(DEV))
    res = bf(torch.randn((n, 32, 64, 48), generator=torch.Generator().manual_seed(n + 1)).to(DEV))
    for tile_cfg in (-1, 0, 2):
        e.tile_cfg = tile_cfg
        for r in (None, res):
            for relu in (False, True):
                y = e.conv(op, x, res=r, relu=relu)
                if tile_cfg == -1:
                    assert e.lib.pam_conv_last_kernel() == 1                  # PAM_CONV_KERNEL_3X3: k_conv3x3
                check(y, ref_conv(c, x, res=r, relu=relu), (n, tile_cfg, r is not None, relu))


@pytest.mark.parametrize('n', CROPS)
def test_sliced_inputs_and_partial_activation(n):
    """Down-chain steps read channel slices of a merged head (in_cstride > Cin); a merged head's activation starts at relu_from."""
    from pam.hrnet_hip import PackedConv
    e = engine()
    wide = bf(torch.randn((n, 128, 64, 48), generator=torch.Generator().manual_seed(9)).to(DEV))
    xs = wide[:, 64:96]                                            # a 32-channel slice, 128 channels between pixels
    for cout, relu in ((32, True), (32, False), (64, False)):
        c = make_conv(32, cout, 3, 2, seed=cout + 1)
        check(e.conv(PackedConv(c, DEV), xs, relu=relu), ref_conv(c, xs, relu=relu), ('slice', n, cout, relu))
    for cout, relu_from in ((160, 32), (224, 96)):                 # out-of-32-only widths with a partial activation
        c = make_conv(32, cout, 3, 2, seed=cout)
        x = bf(torch.randn((n, 32, 64, 48), generator=torch.Generator().manual_seed(cout)).to(DEV))
        check(e.conv(PackedConv(c, DEV), x, relu=True, relu_from=relu_from), ref_conv(c, x, relu=True, relu_from=relu_from),
              ('relu_from', n, cout, relu_from))


def _calibrated_block():
    m = HW.bf16_weights(HW.folded_copy(32))
    return m.stage3[1].branches[0][2]                              # a BasicBlock of the 32-channel branch, folded, bf16 weights


@pytest.mark.parametrize('n', CROPS)
def test_fused_block_is_bit_identical_to_the_two_launch_form(n):
    from pam.hrnet_hip import PackedBlock, PackedConv
    e = engine()
    blk = _calibrated_block()
    pb, o1, o2 = PackedBlock(blk.conv1, blk.conv2, DEV), PackedConv(blk.conv1, DEV), PackedConv(blk.conv2, DEV)
    x = bf(torch.relu(torch.randn((n, 32, 64, 48), generator=torch.Generator().manual_seed(40 + n))).to(DEV))
    two = e.conv(o2, e.conv(o1, x, relu=True), res=x, relu=True)
    t2 = (C.c_int32 * 2)()
    assert e.lib.pam_basic_block2_tile(32, n, 64, 48, t2) == 0 and t2[0] > 0 and t2[1] > 0
    fused = e.basic_block2(pb, x)
    torch.cuda.synchronize()
    assert torch.equal(fused, two), (n, tuple(t2), float((fused.float() - two.float()).abs().max()))
    # tiles that leave ragged last items (64 rows / 48 columns are no multiple of them), down to 1 x 1 items
    for tile in ((5, 7), (10, 44), (3, 48), (1, 1), (17, 5)):
        y = e.basic_block2(pb, x, tile=tile)
        torch.cuda.synchronize()
        assert torch.equal(y, two), (n, tile)
    with torch.no_grad():
        r = blk.to(DEV)(x.float())
    check(fused, r, ('fp32 block', n))


def test_fused_block_rejects_tiles_that_do_not_fit():
    e = engine()
    from pam.hrnet_hip import PackedBlock
    blk = _calibrated_block()
    pb = PackedBlock(blk.conv1, blk.conv2, DEV)
    x = bf(torch.randn((1, 32, 64, 48)).to(DEV))
    y = torch.empty_like(x)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tile in ((30, 48), (64, 48)):
        assert e.lib.pam_basic_block2_nhwc_bf16(st, C.c_void_p(x.data_ptr()), C.c_void_p(pb.wpack.data_ptr()), C.c_void_p(y.data_ptr()),
                                                1, 64, 48, 32, tile[0], tile[1]) != 0
