"""GPU: PoseResNet's own kernels (csrc/pam_resnet.hip) against fp32 torch on the same bf16 inputs and bf16-rounded weights --
k_resnet_stem (7x7 stride-2 conv + bias + ReLU + 3x3 stride-2 max-pool) at 1 / 5 / 20 crops and both pose resolutions, and
k_deconv4x4s2 at the three deconvolution shapes of the network (2048 / 256 / 256 -> 256 channels on H/32, H/16, H/8 inputs) with and
without ReLU and with a non-zero bias.  One layer each: fp32 accumulation and one bf16 rounding of the output, so every metric of
test_gpu_hrnet_modules.metrics is bounded by 0.005 (TOL).  Guard bands around every output stay untouched, and shapes the kernels were
not written for are refused with PAM_E_ARG."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_gpu_hrnet_modules import Checker, METRICS, metrics

pytestmark = pytest.mark.gpu

TOL = {'stem': {k: 0.005 for k in METRICS}, 'deconv': {k: 0.005 for k in METRICS}}
RESOLUTIONS = [(256, 192), (384, 288)]
CROPS = [1, 5, 20]
GUARD = 4096                 # bf16 elements of guard band on each side of an output


class KChecker(Checker):
    """test_gpu_hrnet_modules.Checker with this file's TOL."""

    def __call__(self, family, where, got, ref):
        import json
        assert tuple(got.shape) == tuple(ref.shape), (where, tuple(got.shape), tuple(ref.shape))
        m = metrics(got, ref)
        print('PARITY ' + json.dumps(dict(test=self.test, family=family, where=where, **{k: round(v, 6) for k, v in m.items()})))
        self.bad += ['%s %s: %s %.4g > %.4g' % (family, where, k, m[k], TOL[family][k]) for k in METRICS if not m[k] <= TOL[family][k]]


@pytest.fixture(scope='module')
def dev():
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        yield torch.device('cuda:0')
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def guarded(shape, dev):
    """(N, C, H, W) channels-last bf16 view into a buffer with GUARD sentinel elements on both sides -> (view, buffer, sentinel)."""
    n, c, h, w = shape
    numel = n * c * h * w
    buf = torch.full((numel + 2 * GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
    view = buf[GUARD:GUARD + numel].as_strided((n, c, h, w), (h * w * c, 1, w * c, c))
    return view, buf


def guards_intact(buf):
    return bool((buf[:GUARD].float() == -7.0).all()) and bool((buf[-GUARD:].float() == -7.0).all())


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _stem_layer(seed):
    from pam.hrnet_hip import PackedResNetStem
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=True)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(conv.weight.shape, generator=g) * 0.08).to(torch.bfloat16).float())
        conv.bias.copy_(0.3 * torch.randn(64, generator=g))
    return conv, PackedResNetStem


@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
@pytest.mark.parametrize('n', CROPS)
def test_stem_vs_fp32(dev, res, n):
    from pam import _lib
    lib = _lib.load()
    conv, P = _stem_layer(100 + n)
    op = P(conv, dev)
    g = torch.Generator().manual_seed(200 + n + res[0])
    x3 = torch.randn((n, 3) + res, generator=g).to(torch.bfloat16)
    x8 = torch.cat([x3, torch.zeros((n, 5) + res, dtype=torch.bfloat16)], 1).to(dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = F.max_pool2d(F.relu(F.conv2d(x3.float().to(dev), conv.weight.to(dev), conv.bias.to(dev), 2, 3)), 3, 2, 1)
    y, buf = guarded(tuple(ref.shape), dev)
    rc = lib.pam_resnet_stem_nhwc_bf16(stream(dev), C.c_void_p(x8.data_ptr()), C.c_void_p(op.frag.data_ptr()), C.c_void_p(op.bias.data_ptr()),
                                       C.c_void_p(y.data_ptr()), n, res[0], res[1])
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(buf)
    chk = KChecker('stem %dx%d n%d' % (res + (n,)))
    chk('stem', 'n%d' % n, y, ref)
    chk.done()


# (Cin, input H, W) of the three deconvolutions at 256 x 192 and 384 x 288
DECONV_SHAPES = [(2048, 8, 6), (256, 16, 12), (256, 32, 24), (2048, 12, 9), (256, 24, 18), (256, 48, 36)]


@pytest.mark.parametrize('shape', DECONV_SHAPES, ids=['%d-%dx%d' % s for s in DECONV_SHAPES])
@pytest.mark.parametrize('n', CROPS)
def test_deconv_vs_fp32(dev, shape, n):
    from pam import _lib
    from pam.hrnet_hip import PackedDeconv
    lib = _lib.load()
    cin, h, w = shape
    g = torch.Generator().manual_seed(300 + n + cin + h)
    ct = nn.ConvTranspose2d(cin, 256, 4, 2, 1, bias=True)
    with torch.no_grad():
        ct.weight.copy_((torch.randn(ct.weight.shape, generator=g) * (2.0 / (cin * 4)) ** 0.5).to(torch.bfloat16).float())
        ct.bias.copy_(0.5 * torch.randn(256, generator=g))
    op = PackedDeconv(ct, dev)
    x = torch.randn((n, cin, h, w), generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
    chk = KChecker('deconv %d %dx%d n%d' % (cin, h, w, n))
    for relu in (0, 1):
        with torch.no_grad():
            ref = F.conv_transpose2d(x.float(), ct.weight.to(dev), ct.bias.to(dev), 2, 1)
            if relu:
                ref = F.relu(ref)
        y, buf = guarded(tuple(ref.shape), dev)
        rc = lib.pam_deconv4x4s2_nhwc_bf16(stream(dev), C.c_void_p(x.data_ptr()), C.c_void_p(op.w.data_ptr()), C.c_void_p(op.bias.data_ptr()),
                                           C.c_void_p(y.data_ptr()), n, h, w, cin, 256, relu)
        assert rc == 0
        torch.cuda.synchronize()
        assert guards_intact(buf), relu
        chk('deconv', 'relu=%d' % relu, y, ref)
    chk.done()


def test_refused_shapes_return_e_arg(dev):
    from pam import _lib
    lib = _lib.load()
    E_ARG = -1
    x = torch.zeros(1 << 16, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(1 << 16, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(4096, dtype=torch.float32, device=dev)
    y = torch.zeros(1 << 16, dtype=torch.bfloat16, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    d = lambda *a: lib.pam_deconv4x4s2_nhwc_bf16(stream(dev), *a)
    assert d(p(x), p(w), p(b), p(y), 1, 4, 4, 48, 64, 1) == E_ARG          # Cin % 32
    assert d(p(x), p(w), p(b), p(y), 1, 4, 4, 64, 96, 1) == E_ARG          # Cout % 64
    assert d(p(x), p(w), p(b), p(y), 1, 4, 4, 64, 64, 2) == E_ARG          # activation code
    assert d(None, p(w), p(b), p(y), 1, 4, 4, 64, 64, 1) == E_ARG          # null pointers
    assert d(p(x), None, p(b), p(y), 1, 4, 4, 64, 64, 1) == E_ARG
    assert d(p(x), p(w), None, p(y), 1, 4, 4, 64, 64, 1) == E_ARG
    assert d(p(x), p(w), p(b), None, 1, 4, 4, 64, 64, 1) == E_ARG
    assert d(p(x), p(w), p(b), p(y), 0, 4, 4, 64, 64, 1) == E_ARG          # empty batch
    assert d(p(x), p(w), p(b), p(y), 1, 4, 200, 64, 64, 1) == E_ARG        # rows wider than a workgroup's band
    assert d(p(x), p(w), p(b), p(y), 4096, 64, 64, 256, 256, 1) == E_ARG   # 32-bit offsets would overflow
    s = lambda *a: lib.pam_resnet_stem_nhwc_bf16(stream(dev), *a)
    assert s(None, p(w), p(b), p(y), 1, 256, 192) == E_ARG
    assert s(p(x), p(w), p(b), None, 1, 256, 192) == E_ARG
    assert s(p(x), p(w), p(b), p(y), 0, 256, 192) == E_ARG
    assert s(p(x), p(w), p(b), p(y), 1, 256, 1024) == E_ARG                # H/2 rows wider than the LDS band
    assert s(p(x), p(w), p(b), p(y), 2048, 1024, 384) == E_ARG             # 32-bit offsets would overflow
    torch.cuda.synchronize()
    assert not y.any()
