"""GPU: YOLOv4 and YOLOv4-tiny on the HIP conv stack -- k_route bit for bit against torch.cat of the slices, the scale_x_y decode
entry points against tests/yolo4_ref.py, every step of both plans on its own against the fp32 torch op on the same bf16 input (the walk
of test_gpu_yolo_tiny.py with route, SPP and shortcut-fused steps; the per-family bounds of test_gpu_darknet_layers.py, imported), the
whole networks against their bf16 floor, and the detectors end to end (cfg / weights files and ``arch=``, graph replay, the facade built
from the shipped configs)."""
import ctypes as C
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_v4_calibrated as VC
import guarded_mem as G
import yolo4_ref as R
from oracle import yolo_ref as Y
from test_gpu_darknet_layers import HEAD_FLOOR_RATIO, Checker, family_of, input_x8, padded_bf16, rel
from test_yolo4_cpu import DECODE_CASES, decode_anchors, decode_heads

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _engine():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.ConvEngine()
    e.lib = _lib.load(); e.device = torch.device(DEV)
    return e


# ---- k_route ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 7, 5), (3, 13, 13), (2, 26, 28)]
# name -> ([(source channels, first channel, channels, x2)], padded output channels)
ROUTES = {
    'group-32..63-of-64': ([(64, 32, 32, False)], 64),
    'two-64+64': ([(64, 0, 64, False), (64, 0, 64, False)], 128),
    'two-32-real-of-64': ([(64, 0, 32, False), (64, 0, 32, False)], 64),
    'three-8+24+40-pad-128': ([(16, 8, 8, False), (64, 24, 24, False), (40, 0, 40, False)], 128),
}
ROUTE_CASES = [(s, k) for s in SHAPES for k in ROUTES] + [((2, 26, 26), 'up-128+256'), ((2, 2, 6), 'up-128+256'), ((1, 13, 13), 'four-512')]
ROUTES['up-128+256'] = ([(128, 0, 128, False), (256, 0, 256, True)], 384)
ROUTES['four-512'] = ([(512, 0, 512, False)] * 4, 2048)


def _route_inputs(shape, spec, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    srcs = []
    for c, off, cnt, up in spec:
        hw = (h // 2, w // 2) if up else (h, w)
        t = torch.randn((n, c) + hw, generator=g).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
        srcs.append((t, off, cnt, up))
    return srcs


@pytest.mark.parametrize('shape,kind', ROUTE_CASES, ids=['%dx%dx%d-%s' % (s + (k,)) for s, k in ROUTE_CASES])
def test_route_bit_exact_vs_torch_cat(shape, kind):
    """NHWC bf16: the slices side by side, an x2 source through nearest interpolation, then +0 bits up to the padded count; the output
    between sentinel bands (tests/guarded_mem.py): nothing outside it written, nothing of it left unwritten."""
    spec, c_out = ROUTES[kind]
    srcs = _route_inputs(shape, spec, 7 + shape[1] * 100 + len(kind))
    e = _engine()
    e.arena = G.GuardArena(e.device, 2 * shape[0] * shape[1] * shape[2] * c_out + (1 << 20))
    y = e.route(srcs, c_out)
    torch.cuda.synchronize()
    assert e.arena.report() == ''
    parts = [(F.interpolate(t.float(), scale_factor=2, mode='nearest').to(torch.bfloat16) if up else t)[:, off:off + cnt] for t, off, cnt, up in srcs]
    want = torch.cat(parts, 1)
    real = want.shape[1]
    assert tuple(y.shape) == (shape[0], c_out, shape[1], shape[2]) and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_bits(y[:, :real].permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1)))
    if c_out > real:
        assert int(_bits(y[:, real:].permute(0, 2, 3, 1)).abs().max()) == 0          # +0, not -0


def test_route_rejects_bad_arguments():
    from pam import _lib
    lib = _lib.load()
    a = torch.zeros((1, 4, 4, 64), dtype=torch.bfloat16, device=DEV)
    y = torch.full((1, 4, 4, 128), 3.0, dtype=torch.bfloat16, device=DEV)
    odd = torch.zeros((1, 5, 4, 64), dtype=torch.bfloat16, device=DEV)

    def call(n_src, ptrs, cs, off, cnt, up, out, N, H, W, c_out, tables=True):
        k = max(len(ptrs), 1)
        sp = (C.c_void_p * k)(*[C.c_void_p(p) if p else None for p in ptrs])
        arr = lambda v: (C.c_int32 * k)(*v)
        return lib.pam_route_concat_nhwc_bf16(None, n_src, sp, arr(cs) if tables else None, arr(off), arr(cnt), arr(up), C.c_void_p(out) if out else None, N, H, W, c_out)
    pa, py = a.data_ptr(), y.data_ptr()
    assert call(1, [None], [64], [0], [64], [0], py, 1, 4, 4, 128) == -1                         # NULL source
    assert call(1, [pa], [64], [0], [64], [0], None, 1, 4, 4, 128) == -1                         # NULL output
    assert call(1, [pa], [64], [0], [64], [0], py, 1, 4, 4, 128, tables=False) == -1             # NULL table
    assert call(0, [pa], [64], [0], [64], [0], py, 1, 4, 4, 128) == -1                           # no source
    assert call(5, [pa] * 5, [64] * 5, [0] * 5, [8] * 5, [0] * 5, py, 1, 4, 4, 128) == -1        # five sources
    assert call(1, [pa], [64], [0], [12], [0], py, 1, 4, 4, 128) == -1                           # a slice that is no multiple of 8
    assert call(1, [pa], [64], [4], [8], [0], py, 1, 4, 4, 128) == -1                            # ... or does not start at one
    assert call(1, [pa], [64], [32], [40], [0], py, 1, 4, 4, 128) == -1                          # a slice that leaves its source
    assert call(1, [pa], [64], [0], [0], [0], py, 1, 4, 4, 128) == -1
    assert call(1, [odd.data_ptr()], [64], [0], [64], [1], py, 1, 5, 4, 128) == -1               # x2 with odd H
    assert call(1, [odd.data_ptr()], [64], [0], [64], [1], py, 1, 4, 5, 128) == -1               # x2 with odd W
    assert call(2, [pa, pa], [64, 64], [0, 0], [64, 64], [0, 0], py, 1, 4, 4, 64) == -1          # padded count below the real one
    assert call(1, [pa], [64], [0], [64], [0], py, 1, 4, 4, 100) == -1                           # padded count no multiple of 8
    assert call(1, [pa], [64], [0], [64], [0], py, 0, 4, 4, 128) == -1
    assert call(1, [pa + 2], [64], [0], [64], [0], py, 1, 4, 4, 128) == -1                       # a source that is not 16-byte aligned
    assert call(1, [pa], [64], [0], [64], [0], py, 1 << 14, 1 << 10, 1 << 10, 128) == -1         # 2^38 pieces: past the 32-bit piece index
    torch.cuda.synchronize()
    assert float((y.float() - 3.0).abs().max()) == 0.0                                           # nothing was launched
    assert call(1, [pa], [64], [0], [64], [0], py, 1, 4, 4, 128) == 0
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0


# ---- decode + NMS with scale_x_y -------------------------------------------------------------------------------------------------------
def _run_sxy(heads_np, anchors, scales, net, nc, cls, st, nt, fw, fh, max_det, split, plain=False):
    """pam_yolo_detect_heads_sxy[_ws] (plain: pam_yolo_detect_heads[_ws], no table) on bf16 copies of heads_np -> boxes, count, the heads."""
    from pam import _lib
    lib = _lib.load()
    n, nh = heads_np[0].shape[0], len(heads_np)
    hd = [torch.from_numpy(h).to(torch.bfloat16).to(DEV).contiguous() for h in heads_np]
    hp = (C.c_void_p * nh)(*[C.c_void_p(h.data_ptr()) for h in hd])
    gh = (C.c_int32 * nh)(*[h.shape[1] for h in hd]); gw = (C.c_int32 * nh)(*[h.shape[2] for h in hd]); cs = (C.c_int32 * nh)(*[h.shape[3] for h in hd])
    an = np.ascontiguousarray(anchors.reshape(-1), dtype=np.float32)
    sc = np.ascontiguousarray(scales, dtype=np.float32)
    assert an.size == 6 * nh and sc.size == nh
    boxes = torch.full((n, max_det, 5), -1.0, dtype=torch.float32, device=DEV)
    count = torch.full((2 * n,), -1, dtype=torch.int32, device=DEV)
    head = (None, n, nh, hp, gh, gw, cs, an.ctypes.data_as(C.c_void_p))
    tail = (net[0], net[1], nc, cls, st, nt, fw, fh, max_det, C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr()))
    table = () if plain else (sc.ctypes.data_as(C.c_void_p),)
    if split:
        need = lib.pam_yolo_detect_heads_workspace_bytes(n, nh, gh, gw)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        fn = lib.pam_yolo_detect_heads_ws if plain else lib.pam_yolo_detect_heads_sxy_ws
        rc = fn(*head, *table, *tail, C.c_void_p(ws.data_ptr()), need)
    else:
        fn = lib.pam_yolo_detect_heads if plain else lib.pam_yolo_detect_heads_sxy
        rc = fn(*head, *table, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), count.cpu().numpy(), [h.float().cpu().numpy() for h in hd]


V4_ANCHORS = np.array([(12, 16), (19, 36), (40, 28), (36, 75), (76, 55), (72, 146), (142, 110), (192, 243), (459, 401)], dtype=np.float32).reshape(3, 3, 2)
SXY_CASES = [
    # n, grids, nc, chan stride, cls, score_thresh, nms_thresh, max_det, logit sigma | scales | anchors (None: the tiny test's)
    ((3, (13, 26), 80, 256, 0, 0.6, 0.45, 64, 1.5), (1.05, 1.05), None),                 # YOLOv4-tiny's two heads
    ((2, (52, 26, 13), 80, 256, 0, 0.6, 0.45, 64, 1.5), (1.2, 1.1, 1.05), V4_ANCHORS),   # YOLOv4's three heads, finest first, shipped anchors
    ((2, (13,), 80, 256, 0, 0.5, 0.45, 64, 1.5), (1.2,), None),                          # one head
    ((1, (8, 16), 1, 24, 0, 0.2, 0.5, 100, 1.0), (1.05, 1.05), None),                    # > 1024 candidates are counted, 1024 enter
    ((2, (5, 9), 3, 32, 2, 0.999999, 0.45, 16, 1.0), (1.05, 1.05), None),                # nothing passes
]


@pytest.mark.parametrize('case,scales,anchors', SXY_CASES, ids=['two', 'three-finest-first', 'one', 'two-overflow', 'two-none'])
@pytest.mark.parametrize('split', [False, True], ids=['one_wg', 'ws'])
def test_yolo_detect_sxy_vs_reference(case, scales, anchors, split):
    n, grids, nc, cs, cls, st, nt, max_det, sigma = case
    anchors = decode_anchors(len(grids)) if anchors is None else anchors
    heads = decode_heads(case)
    boxes, count, hq = _run_sxy(heads, anchors, scales, (416, 448), nc, cls, st, nt, 1032, 776, max_det, split)
    shift = 0.0
    for i in range(n):
        exp, nfound = R.decode([h[i] for h in hq], anchors, scales, 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        assert count[n + i] == nfound, (i, count[n + i], nfound)
        assert count[i] == len(exp), (i, count[i], len(exp))
        got = boxes[i, :count[i]]
        assert np.allclose(got, exp, rtol=2e-5, atol=1e-3), np.abs(got - exp).max()
        assert (boxes[i, count[i]:] == -1.0).all()
        one, _ = R.decode([h[i] for h in hq], anchors, [1.0] * len(grids), 416, 448, nc, cls, st, nt, 1032, 776, max_det)
        if len(one) == len(exp) and len(exp):
            shift = max(shift, float(np.abs(one[:, :4] - exp[:, :4]).max()))
    if st > 0.99:
        assert (count[:n] == 0).all()
    else:
        assert count[:n].sum() > 0
    if grids == (8, 16):
        assert count[n] > 1024
    if scales[0] == 1.2 and len(grids) == 3:
        assert shift > 1.0                                   # a decode that ignores the table misses the boxes by pixels, not by the tolerance


@pytest.mark.parametrize('case', [DECODE_CASES[0], DECODE_CASES[6], DECODE_CASES[4]], ids=['two', 'three', 'one'])
@pytest.mark.parametrize('split', [False, True], ids=['one_wg', 'ws'])
def test_scales_of_one_give_the_bytes_of_the_plain_entry_points(case, split):
    n, grids, nc, cs, cls, st, nt, max_det, sigma = case
    heads, anchors = decode_heads(case), decode_anchors(len(grids))
    b1, c1, _ = _run_sxy(heads, anchors, [1.0] * len(grids), (416, 448), nc, cls, st, nt, 1032, 776, max_det, split)
    b0, c0, _ = _run_sxy(heads, anchors, [1.0] * len(grids), (416, 448), nc, cls, st, nt, 1032, 776, max_det, split, plain=True)
    assert b1.tobytes() == b0.tobytes() and c1.tobytes() == c0.tobytes() and c1[:n].sum() > 0


def test_sxy_rejects_bad_tables():
    from pam import _lib
    lib = _lib.load()
    h = torch.zeros((1, 4, 4, 24), dtype=torch.bfloat16, device=DEV)
    hp = (C.c_void_p * 2)(*[C.c_void_p(h.data_ptr())] * 2)
    g = (C.c_int32 * 2)(4, 4); cs = (C.c_int32 * 2)(24, 24)
    an = np.ones(12, dtype=np.float32)
    boxes = torch.full((1, 4, 5), 3.0, dtype=torch.float32, device=DEV); count = torch.full((2,), 3, dtype=torch.int32, device=DEV)

    def call(table):
        return lib.pam_yolo_detect_heads_sxy(None, 1, 2, hp, g, g, cs, an.ctypes.data_as(C.c_void_p), table, 64, 64, 3, 0, 0.5, 0.45, 64, 64, 4,
                                             C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr()))
    assert call(None) == -1
    for bad in ((1.0, 0.99), (float('nan'), 1.0), (1.0, float('inf')), (-1.2, 1.0)):
        t = np.array(bad, dtype=np.float32)
        assert call(t.ctypes.data_as(C.c_void_p)) == -1, bad
    torch.cuda.synchronize()
    assert float((boxes - 3.0).abs().max()) == 0.0 and int((count - 3).abs().max()) == 0
    t = np.array((1.0, 2.0), dtype=np.float32)
    assert call(t.ctypes.data_as(C.c_void_p)) == 0


# ---- every step of both plans on its own -------------------------------------------------------------------------------------------------
class Spy4(object):
    """The executor's library with its launch entries recorded: a conv launch as (kernel, form) read right after it returns."""
    NAMES = {'pam_upsample_add_nhwc_bf16_ex': 'k_upsample_add', 'pam_upsample_concat_nhwc_bf16': 'k_upsample_concat',
             'pam_route_concat_nhwc_bf16': 'k_route', 'pam_maxpool_nhwc_bf16': 'k_maxpool', 'pam_spp_concat_nhwc_bf16': 'k_spp'}

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.NAMES and name not in ('pam_conv2d_nhwc_bf16_ex', 'pam_pointwise64_act_nhwc_bf16'):
            return fn

        def launch(*args):
            rc = fn(*args)
            if name == 'pam_conv2d_nhwc_bf16_ex':
                self.calls.append(form_name(self._lib.pam_conv_last_kernel(), self._lib.pam_conv_last_form()) + ' act=%d' % args[16])
            elif name == 'pam_pointwise64_act_nhwc_bf16':
                self.calls.append('k_pw1 act=%d' % args[-1])
            else:
                self.calls.append(self.NAMES[name])
            return rc
        return launch


def form_name(kind, form):
    """(pam_conv_last_kernel, pam_conv_last_form) -> the kernel's name as DESIGN.md section 10u lists it (encoding: include/pam.h)."""
    if kind == 0:
        return 'k_conv_igemm%s %dx%d' % (' gen' if form >= 1000000 else '', form // 1000 % 1000, form % 1000)
    if kind == 1:
        return 'k_conv3x3 Cin=%d slab=%d' % (form // 10, 16 * (form % 10))
    if kind == 2:
        return 'k_conv3x3s%s Cin=%d slab=%d MT=%d' % (' gen' if form >= 100000 else '', form // 100 % 1000, 16 * (form // 10 % 10), form % 10)
    if kind == 3:
        return 'k_conv_gs%s tile=%d slab=%d nbuf=%d' % ('_mish' if form % 1000 >= 500 else '', form // 1000 % 1000, form % 500, form // 1000000)
    if kind == 4:
        return 'k_conv_stem%s s%d Cout=%d' % ('_mish' if form >= 1000 else '', form // 100 % 10, form % 100)
    raise AssertionError('unknown conv kernel %d (form %d)' % (kind, form))


# (arch, width, height, views)
CASES = [('yolov4-tiny', 416, 416, 1), ('yolov4-tiny', 416, 416, 5), ('yolov4-tiny', 320, 256, 2), ('yolov4-tiny', 64, 64, 3),
         ('yolov4', 416, 416, 1), ('yolov4', 320, 256, 2), ('yolov4', 96, 64, 3)]
CASE_IDS = ['%s-%dx%d-n%d' % c for c in CASES]


class Env(object):
    pass


@pytest.fixture(scope='module')
def env():
    """One executor per network and input size (packing is per network), TF32 off for the fp32 reference."""
    from pam import _lib, yolov4
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    e = Env()
    e.dev = torch.device(DEV)
    e.nets = {}

    def net(arch, w, h):
        if (arch, w, h) not in e.nets:
            model = VC.calibrated(arch, width=w, height=h)
            hip = yolov4.HipDarknet4(model, e.dev)
            hip.lib = Spy4(_lib.load())
            convs = {i: c.to(e.dev) for i, c in VC.folded_convs(model).items()}
            e.nets[(arch, w, h)] = (model, hip, convs)
        return e.nets[(arch, w, h)]
    e.net = net
    try:
        yield e
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def walk(e, arch, w, h, n, check):
    """Run the plan step by step on the reference's bf16 inputs (the walk of test_gpu_yolo_tiny.py plus route, SPP and shortcut-fused
    steps): a conv step against yolo4_ref.layer -- the fp32 torch op on the same input, F.mish or F.leaky_relu, the shortcut added after
    the activation --, bounded per family; route, pool, SPP and upsample + route steps bitwise; padded output channels exactly 0.
    -> {(dst, family): launches}."""
    from pam import yolov3
    model, hip, convs = e.net(arch, w, h)
    last_use = {}
    for k, step in enumerate(hip.plan):
        reads = ([step[3]] + ([step[5]] if step[5] is not None else [])) if step[0] == 'conv' else \
            ([p[0] for p in step[2]] if step[0] == 'route' else [s for s in step[2:4] if isinstance(s, int)] if step[0] in ('add', 'upcat') else [step[2]])
        for s in reads:
            last_use[s] = k
    outs = {-1: input_x8(e, w, h, n, 4000 + 31 * n + w)}
    rec = {}
    for k, step in enumerate(hip.plan):
        kind, dst = step[0], step[1]
        hip.lib.calls = []
        with torch.no_grad():
            y = hip.run_step(step, outs)
        torch.cuda.synchronize()
        real = hip.real[dst]
        if kind == 'conv':
            _, _, op, src, act, skip = step
            fam = family_of(hip, step, outs[src])
            c = convs[dst - 1 if skip is not None else dst]
            with torch.no_grad():
                r = R.layer(outs[src][:, :c.in_channels].float(), c, act, outs[skip][:, :c.out_channels].float() if skip is not None else None)
            assert c.out_channels == real and y.shape[1] == hip.padded[dst]
            check(fam, 'layer %d' % dst, y[:, :real], r)
            outs[dst] = padded_bf16(r, y.shape[1])
            rec[(dst, fam + ('/mish' if act == 'mish' else ''))] = list(hip.lib.calls)
            del r
        elif kind == 'route':
            parts = [(F.interpolate(outs[l].float(), scale_factor=2, mode='nearest').to(torch.bfloat16) if up else outs[l])[:, off:off + cnt]
                     for l, off, cnt, up in step[2]]
            want = torch.cat(parts, 1)
            assert want.shape[1] == real and tuple(y.shape) == (n, step[3]) + tuple(want.shape[2:]), (dst, tuple(y.shape), tuple(want.shape))
            assert torch.equal(_bits(y[:, :real].permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1))), 'route of layer %d' % dst
            outs[dst] = y
            rec[(dst, 'route')] = list(hip.lib.calls)
        elif kind == 'pool':
            want = yolov3.darknet_maxpool(outs[step[2]].float(), step[3], step[4]).to(torch.bfloat16)
            assert tuple(y.shape) == tuple(want.shape) and torch.equal(_bits(y.permute(0, 2, 3, 1)), _bits(want.permute(0, 2, 3, 1))), 'max-pool of layer %d' % dst
            outs[dst] = y
            rec[(dst, 'pool')] = list(hip.lib.calls)
        elif kind == 'spp':
            x = outs[step[2]]
            want = torch.cat([yolov3.darknet_maxpool(x.float(), s, 1) for s in reversed(step[3])] + [x.float()], 1)
            assert tuple(y.shape) == tuple(want.shape) and torch.equal(y.float(), want), 'SPP block of layer %d' % dst      # float compare: a pooled zero may have either sign
            assert torch.equal(_bits(y[:, 3 * x.shape[1]:].permute(0, 2, 3, 1)), _bits(x.permute(0, 2, 3, 1)))
            outs[dst] = y
            rec[(dst, 'spp')] = list(hip.lib.calls)
        elif kind == 'upcat':
            a, b = outs[step[2]], outs[step[3]]
            want = torch.cat([F.interpolate(a.float(), scale_factor=2, mode='nearest'), b.float()], 1)
            assert torch.equal(y.float(), want), 'upsample + route of layer %d' % dst
            outs[dst] = y
            rec[(dst, 'upcat')] = list(hip.lib.calls)
        else:                                          # alias, head: the same tensor (no [shortcut] of these cfgs is left unfused)
            assert kind in ('alias', 'head'), kind
            outs[dst] = outs[step[2]]
        if kind not in ('alias', 'head') and y.shape[1] > real:
            assert int(_bits(y[:, real:].permute(0, 2, 3, 1)).abs().max()) == 0, ('padded channels of layer %d' % dst)
        del y
        for s in [s for s in outs if last_use.get(s, -1) <= k and s != dst]:
            del outs[s]
    return rec


def design_kernels():
    """The kernels DESIGN.md section 10u lists as carrying the mish epilogue (the rows of its table whose first cell is `k_...`)."""
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    sec = text[text.index('\n## 10u.') + 1:]
    nxt = re.search(r'\n## ', sec)
    sec = sec[:nxt.start()] if nxt else sec
    return set(re.findall(r'^\| `(k_[a-z0-9_]+)', sec, re.M))


@pytest.mark.parametrize('arch,w,h,n', CASES, ids=CASE_IDS)
def test_every_step_vs_fp32(env, arch, w, h, n):
    """Every step of the plan at this input size and view count against the fp32 op on the same bf16 input, within the per-family bounds
    of test_gpu_darknet_layers.TOL (set for leaky layers; a mish layer adds an epilogue error of 1.7e-4 bf16 half-ulp)."""
    cid = CASE_IDS[CASES.index((arch, w, h, n))]
    chk = Checker(cid)
    rec = walk(env, arch, w, h, n, chk)
    print('FORMS ' + json.dumps(dict(case=cid, layers=['%d %s: %s' % (d, f, ', '.join(v)) for (d, f), v in sorted(rec.items())])))
    fams = [f for _, f in sorted(rec)]
    listed = design_kernels()
    assert {'k_conv_stem_mish', 'k_conv_gs_mish', 'k_conv_igemm', 'k_conv3x3s'} <= listed
    if arch == 'yolov4':
        assert rec[(0, 'stem/mish')] == ['k_conv_stem_mish s1 Cout=32 act=3']
        mish = {k: v for k, v in rec.items() if k[1].endswith('/mish')}
        assert len(mish) == 72
        for (dst, fam), calls in mish.items():
            conv = [c for c in calls if c.startswith('k_conv')]
            assert len(conv) == 1 and conv[0].endswith(' act=%d' % (7 if fam == 'conv3x3+shortcut/mish' else 3)), (dst, fam, calls)
            assert conv[0].split()[0] in listed and ('_mish' in conv[0] or ' gen ' in conv[0]), (dst, fam, calls)
        assert fams.count('route') == 9 and fams.count('spp') == 1 and fams.count('head1x1') == 3
        assert fams.count('conv3x3+shortcut/mish') + fams.count('unfused3x3+add/mish') == 23
    else:
        assert rec[(0, 'stem')] == ['k_conv_stem s2 Cout=32 act=2']
        assert fams.count('route') == 9 and fams.count('upcat') == 1 and fams.count('pool') == 3 and fams.count('head1x1') == 2
        assert all(v == ['k_route'] for (d, f), v in rec.items() if f == 'route')
    chk.done()


# ---- the whole networks and the detectors ----------------------------------------------------------------------------------------------
SIZES = {'yolov4-tiny': 24251276, 'yolov4': 257717640}
GRIDS = {'yolov4-tiny': [13, 26], 'yolov4': [52, 26, 13]}


@pytest.fixture(scope='module')
def detectors(env, tmp_path_factory):
    from pam import yolov4
    made = {}

    def get(arch):
        if arch not in made:
            d = str(tmp_path_factory.mktemp(arch.replace('-', '_')))
            cfg, weights = os.path.join(d, arch + '.cfg'), os.path.join(d, 'calibrated.weights')
            with open(cfg, 'w') as f:
                f.write(yolov4.ARCHS4[arch]())
            VC.calibrated(arch).save_darknet_weights(weights)
            assert os.path.getsize(weights) == SIZES[arch]
            # arch names the OTHER network: a cfg file always decides
            det = yolov4.YOLOv4(cfg, weights, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64,
                                arch='yolov4' if arch == 'yolov4-tiny' else 'yolov4-tiny')
            assert det.weights == weights and det.anchors.shape == (len(GRIDS[arch]), 3, 2) and det.size == (416, 416)
            assert [round(float(s), 3) for s in det.scale_xy] == ([1.05, 1.05] if arch == 'yolov4-tiny' else [1.2, 1.1, 1.05])
            det.test_files = (cfg, weights)
            made[arch] = det
        return made[arch]
    return get


@pytest.mark.parametrize('arch', ['yolov4-tiny', 'yolov4'])
def test_heads_within_the_bf16_floor(env, detectors, arch):
    """Every head vs the fp32 network at 2 views: within HEAD_FLOOR_RATIO (1.1, test_gpu_darknet_layers) of the error that bf16 weights
    and a bf16 store after every convolution alone cost on the same images (darknet_v4_calibrated.storage_forward)."""
    det, model, n = detectors(arch), VC.calibrated(arch), 2
    x8 = input_x8(env, 416, 416, n, 79)
    with torch.no_grad():
        heads = det.net.forward(x8)
        x = x8[:, :3].float()
        ref = VC.storage_forward(model, x, bf16_weights=False, bf16_store=False)
        floor = VC.storage_forward(model, x)
    torch.cuda.synchronize()
    assert [tuple(h.shape) for h in heads] == [(n, 256, g, g) for g in GRIDS[arch]]
    bad = []
    for k, (hd, r, fl) in enumerate(zip(heads, ref, floor)):
        assert float(hd[:, 255:].float().abs().max()) == 0.0
        err, ferr = rel(hd[:, :255].float() - r, r), rel(fl - r, r)
        print('HEAD ' + json.dumps(dict(arch=arch, n=n, head=k, rel=err, floor=ferr, ratio=err / ferr)))
        if not err <= HEAD_FLOOR_RATIO * ferr:
            bad.append('head %d: rel err %.4g > %.2f x the bf16 floor %.4g' % (k, err, HEAD_FLOOR_RATIO, ferr))
    assert not bad, bad


def _check_detector(det, eager, imgs, fw, fh):
    """Graph replay == eager bitwise, boxes == yolo4_ref.decode on the kernel's own heads, sorted by score, single image == element 0."""
    n = len(imgs)
    H, W = det.size
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    b1, c1 = [t.clone() for t in det.detect_dev(frames)]
    b2, c2 = [t.clone() for t in det.detect_dev(frames)]                      # replay
    b3, c3 = [t.clone() for t in eager.detect_dev(frames)]
    torch.cuda.synchronize()
    assert (n, fh, fw) in det._graphs and det._graphs[(n, fh, fw)][0] is not None and eager._graphs[(n, fh, fw)][0] is None
    assert torch.equal(b1, b2) and torch.equal(c1, c2)
    assert torch.equal(b1, b3) and torch.equal(c1, c3)
    x8 = torch.from_numpy(Y.resize_frames(np.stack(imgs), H, W)).to(DEV).permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        hq = [t.permute(0, 2, 3, 1).float().cpu().numpy() for t in det.net.forward(x8)]
    boxes, count = b1.cpu().numpy(), c1.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = det(imgs)
        single = det(imgs[0])
    per_view = []
    for i in range(n):
        exp, cand = R.decode([t[i] for t in hq], det.anchors, det.scale_xy, W, H, det.num_classes, 0, det.score_thresh, det.nms_thresh, fw, fh, det.max_det)
        assert count[n + i] == cand and count[i] == len(exp), (i, count[i], len(exp), count[n + i], cand)
        assert np.allclose(boxes[i, :count[i]], exp, rtol=2e-5, atol=1e-3), np.abs(boxes[i, :count[i]] - exp).max()
        assert res[i].dtype == np.float32 and res[i].shape == (len(exp), 5) and np.array_equal(res[i], boxes[i, :count[i]])
        assert (np.diff(res[i][:, 4]) <= 0).all()
        per_view.append(len(exp))
    assert np.array_equal(single, res[0])
    return per_view


@pytest.mark.parametrize('arch', ['yolov4-tiny', 'yolov4'])
def test_detector_from_files_replay_and_reference(env, detectors, arch):
    from pam import yolov4
    det = detectors(arch)
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (416, 416, 3), dtype=np.uint8) for _ in range(3)]
    eager = yolov4.YOLOv4(*det.test_files, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64, use_graph=False)
    assert min(_check_detector(det, eager, imgs, 416, 416)) >= 1             # the calibrated network: boxes in every view


@pytest.mark.parametrize('arch', ['yolov4-tiny', 'yolov4'])
def test_detector_by_arch_keyword(arch):
    from pam import yolov4
    kw = dict(score_thresh=0.05, nms_thresh=0.45, use_cuda=True, max_det=32, seed=1, arch=arch)
    det, eager = yolov4.YOLOv4(None, None, None, **kw), yolov4.YOLOv4(None, None, None, use_graph=False, **kw)
    assert det.anchors.shape == (len(GRIDS[arch]), 3, 2) and type(det.net).__name__ == 'HipDarknet4'
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(2)]
    _check_detector(det, eager, imgs, 320, 240)
    with pytest.raises(ValueError):
        yolov4.YOLOv4(None, None, None, arch='yolov5')


def test_default_arch_and_v3_bytes():
    """YOLOv4's default network is YOLOv4; on a yolov3-tiny cfg it gives the plan and the bytes YOLOv3 gives."""
    from pam import yolov3, yolov4
    kw = dict(score_thresh=0.05, nms_thresh=0.45, use_cuda=True, max_det=32, seed=1)
    assert len(yolov4.YOLOv4(None, None, None, **kw).net.plan) == 132        # 162 layers less 23 fused shortcuts, 5 SPP inner layers, 2 lazy upsamples
    a, b = yolov3.YOLOv3(None, None, None, arch='yolov3-tiny', **kw), yolov4.YOLOv4(None, None, None, arch='yolov3-tiny', **kw)
    assert [s[:2] for s in a.net.plan] == [s[:2] for s in b.net.plan] and list(b.scale_xy) == [1.0, 1.0]
    rng = np.random.default_rng(6)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 240, 320, 3), dtype=np.uint8)).to(DEV)
    ba, ca = [t.clone() for t in a.detect_dev(frames)]
    bb, cb = [t.clone() for t in b.detect_dev(frames)]
    torch.cuda.synchronize()
    assert int(ca[:2].sum()) > 0 and torch.equal(ba.view(torch.int32), bb.view(torch.int32)) and torch.equal(ca, cb)


def _facade(arch, weights):
    import pam
    from pam import ivclabpose as IV
    from pam.dataset import GetConfig
    name = 'model_configs_yolov4tiny.yaml' if arch == 'yolov4-tiny' else 'model_configs_yolov4.yaml'
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', name))
    pipe = cfg.PIPELINE_COMBINATION
    assert str(pipe['DETECT_MODEL']) == 'YOLOv4'
    d = dict(cfg.DETECT_MODELS[str(pipe['DETECT_MODEL']).upper()])
    assert d['NAME'] == 'YOLOv4' and d['ARCH'] == arch and d['CFG'].endswith(arch + '.cfg') and d['WEIGHT'].endswith(arch + '.weights')
    assert not os.path.exists(d['CFG'])                                   # no cfg file here: ARCH decides
    d['WEIGHT'], d['SCORE_THRESH'], d['NMS_THRESH'] = weights, 0.5, 0.45  # the calibrated test weights: boxes in every view
    api = IV.ivclabpose(person_detector=d, pose_detector=None, person_matcher=None)
    assert type(api.bbox_detector).__name__ == 'YOLOv4' and api.bbox_detector.anchors.shape == (len(GRIDS[arch]), 3, 2) and api.bbox_detector.weights == weights
    return api


@pytest.mark.parametrize('arch', ['yolov4-tiny', 'yolov4'])
def test_facade_persondetect_format_and_a_frame_ahead(detectors, arch):
    """ivclabpose built from the shipped YAML: PersonDetect dicts in the format test_persondetect_facade_format checks, and
    PersonDetectAhead / PersonDetectResult return PersonDetect's boxes."""
    api = _facade(arch, detectors(arch).test_files[1])
    rng = np.random.default_rng(9)
    sets = [[rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)] for _ in range(2)]
    want = [api.PersonDetect(imgs, image_id=k) for k, imgs in enumerate(sets)]
    assert sum(len(v) for f in want for v in f) > 0
    for persons, im in zip(want[0], sets[0]):
        for p in persons:
            assert p['image_id'] == 0 and p['category_id'] == 1 and p['data'] is im and p['feature'] == []
            x, y, w, h = p['bbox']
            assert x >= 0 and y >= 0 and x + w <= 320 + 1e-3 and y + h <= 240 + 1e-3
            assert isinstance(p['score'], float) and round(p['score'], 4) == p['score']
    t0 = api.PersonDetectAhead(sets[0], 0)
    t1 = api.PersonDetectAhead(sets[1], 1)                                # issued BEFORE frame 0 is collected
    got = [api.PersonDetectResult(t0), api.PersonDetectResult(t1)]
    strip = lambda frames: [[(p['image_id'], p['bbox'], p['score']) for p in v] for v in frames]
    assert [strip(f) for f in got] == [strip(f) for f in want]


def test_facade_yolov3_name_still_builds_yolov3():
    from pam import ivclabpose as IV
    api = IV.ivclabpose(person_detector=dict(NAME='YOLOv3', ARCH='yolov3-tiny', CFG='', WEIGHT='', CLASS_NAMES='', SCORE_THRESH=0.5, NMS_THRESH=0.45),
                        pose_detector=None, person_matcher=None)
    assert type(api.bbox_detector).__name__ == 'YOLOv3' and type(api.bbox_detector.net).__name__ == 'HipDarknet'
    with pytest.raises(ValueError):
        IV.ivclabpose(person_detector=dict(NAME='YOLOv3', ARCH='yolov4', CFG='', WEIGHT='', CLASS_NAMES='', SCORE_THRESH=0.5, NMS_THRESH=0.45),
                      pose_detector=None, person_matcher=None)
