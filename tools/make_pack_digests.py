#!/usr/bin/env python3
"""What the weight packers and the shape-only walks of pam/hrnet_hip.py produce, written down so that a change of that code which is
meant to change nothing can be checked (tests/test_packing_cpu.py):

  tests/golden/pack_digests.json     sha256 of every packed image built from seeded convolutions on the CPU (``digests``) and, per
                                     executor configuration, the ``count`` tally + the measuring arena's peak of one shape-only forward
                                     on the meta device (``walks``)

Only names of ``pam.hrnet_hip`` (and the network modules) are used, so the same file runs on the commit before a refactor and after it.

Usage (from the repository root):  python tools/make_pack_digests.py [--out tests/golden]
"""
import argparse
import hashlib
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pam  # noqa: E402,F401  (the package alias)
from pam import hrnet, hrnet_hip, poseresnet, yolov3  # noqa: E402


def sha(*tensors):
    """sha256 over dtype, shape and bytes of every tensor (None and plain values hash as their repr)."""
    h = hashlib.sha256()
    for t in tensors:
        if not torch.is_tensor(t):
            h.update(repr(t).encode())
            continue
        t = t.detach().cpu().contiguous()
        h.update(('%s%s' % (t.dtype, tuple(t.shape))).encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def seeded(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return mod


def conv(cin, cout, k=3, stride=1, pad=None, bias=True, seed=0):
    return seeded(nn.Conv2d(cin, cout, k, stride, k // 2 if pad is None else pad, bias=bias), 1000 * seed + 7 * cin + cout + k)


class StubLayout(object):
    """Stands in for the library's layout queries: the streamed slab width (0 = the classic kernel) and the classic slab width."""

    def __init__(self, streamed_bn, classic_bn):
        self.s, self.c = streamed_bn, classic_bn

    def pam_conv3x3_layout_ex(self, h, w, cin, cout, c96_slab):
        return self.s

    def pam_conv3x3_slab(self, h, w, cin, cout):
        return self.c


class NoLib(object):
    """Every entry point succeeds without doing anything."""

    def __getattr__(self, name):
        return lambda *a, **k: 0


class HostStream(object):
    cuda_stream = 0


def pw64_image_as_conv_builds_it(op):
    """The image ConvEngine.conv() caches in op._images['pw64'], from a real call of conv() whose launch goes to a library that does nothing."""
    eng = hrnet_hip.ConvEngine.__new__(hrnet_hip.ConvEngine)
    eng.lib = NoLib()
    x = torch.zeros((1, 64, 256, 256), dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    real = torch.cuda.current_stream
    torch.cuda.current_stream = lambda device=None: HostStream()
    try:
        eng.conv(op, x, relu=True)
    finally:
        torch.cuda.current_stream = real
    return op._images['pw64']


def pack_digests():
    H = hrnet_hip
    d = {}
    for c in (32, 48, 96):
        d['PackedBlock/%d/wpack' % c] = sha(H.PackedBlock(conv(c, c, seed=1), conv(c, c, bias=(c != 96), seed=2), 'cpu').wpack)
    for down in (False, True):
        for nxt in (False, True):
            t = H.PackedTail(conv(64, 256, 1, seed=3), conv(64, 256, 1, bias=False, seed=4) if down else None,
                             conv(256, 64, 1, seed=5) if nxt else None, 'cpu')
            d['PackedTail/down=%d/next=%d' % (down, nxt)] = sha(t.w3, t.b3, t.w1, t.b1, t.S)
    pw = H.PackedPointwise64(conv(64, 64, 1, seed=6), 'cpu')
    d['PackedPointwise64'] = sha(pw.w, pw.b)
    d['PackedPointwise64/no-bias'] = sha(H.PackedPointwise64(conv(64, 64, 1, bias=False, seed=6), 'cpu').b)
    d['conv64_image'] = sha(H.conv64_image(conv(64, 64, seed=7), 'cpu'))
    bn = H.PackedBneck(conv(64, 64, seed=8), None, 'cpu')
    d['PackedBneck'] = sha(bn.w2, bn.b2)
    c1 = H.PackedConv(conv(3, 64, 3, 2, seed=9), 'cpu', pad_cin_to=8)
    st = H.PackedStem(c1, conv(64, 64, 3, 2, bias=False, seed=10), pw, 'cpu')
    d['PackedStem'] = sha(st.w2, st.b2)
    for c, widths in ((48, (96, 192, 384)), (32, (64, 128, 256))):
        up = H.PackedUp([conv(cs, c, 1, bias=(i != 1), seed=11) for i, cs in enumerate(widths)], [1, 2, 3], 'cpu')
        for i, cs in enumerate(widths):
            d['PackedUp/%d/from%d' % (c, cs)] = sha(up.wimg[i], up.bias[i], up.shifts[i], up.chans[i])
    for cout in (48, 96, 192):
        d['down48_image/%d' % cout] = sha(H.down48_image(H.PackedConv(conv(48, cout, 3, 2, seed=12), 'cpu')))
    w_ohwi = torch.randn((192, 3, 3, 192), generator=torch.Generator().manual_seed(13))
    for bn_ in (32, 48, 64):
        d['streamed_image/%d' % bn_] = sha(H.streamed_image(w_ohwi, bn_, 'cpu'))
    for name, op in (('8to64s2', c1), ('8to32s1', H.PackedConv(conv(3, 32, seed=14), 'cpu', pad_cin_to=8)),
                     ('16to32', H.PackedConv(conv(3, 16, bias=False, seed=15), 'cpu', pad_cin_to=8, pad_cout_to=32)),
                     ('merged', H.PackedConv.merged([conv(192, 48, 1, seed=16), conv(192, 96, 1, bias=False, seed=17), conv(192, 384, 1, seed=18)], 'cpu'))):
        d['PackedConv/%s' % name] = sha(op.w, op.bias, op._stem, op.cin, op.cout, op.kh, op.kw, op.stride, op.pad)
    # PackedConv.image(): (cin, cout, streamed slab or 0, classic slab)
    saved = H.PackedConv.layout_lib
    try:
        for cin, cout, s, c in ((48, 96, 0, 48), (96, 96, 48, 32), (96, 96, 96, 96), (96, 192, 64, 64), (192, 192, 64, 64), (192, 192, 32, 32),
                                (384, 384, 64, 64), (32, 32, 32, 32), (96, 96, 64, 64)):
            op = H.PackedConv(conv(cin, cout, seed=19), 'cpu')
            for classic in (False, True):
                H.PackedConv.layout_lib = StubLayout(s, c)
                img = op.image(24, 18, classic=classic)
                d['PackedConv.image/%d-%d/s%d-c%d/classic=%d' % (cin, cout, s, c, classic)] = sha(
                    img, getattr(op, 'last_streamed', None), getattr(op, 'last_c96', None))
    finally:
        H.PackedConv.layout_lib = saved
    d['conv/pw64'] = sha(pw64_image_as_conv_builds_it(H.PackedConv(conv(64, 64, 1, seed=20), 'cpu')))
    rs = H.PackedResNetStem(conv(3, 64, 7, 2, bias=False, seed=21), 'cpu')
    d['PackedResNetStem'] = sha(rs.frag, rs.bias)
    for cin in (2048, 256):
        dc = H.PackedDeconv(seeded(nn.ConvTranspose2d(cin, 256, 4, 2, 1, bias=(cin == 256)), 22), 'cpu')
        d['PackedDeconv/%d' % cin] = sha(dc.w, dc.bias, dc.cin, dc.cout)
    return d


class MetaLib(object):
    """The library for a shape-only walk: the host-side layout queries (the executor's plan depends on them) are the real ones."""

    def __getattr__(self, name):
        if name in ('pam_conv3x3_slab', 'pam_conv3x3_layout', 'pam_conv3x3_layout_ex'):
            return getattr(pam._lib.load(), name)
        return lambda *a, **k: 0


def _walk(eng, run, shape):
    eng.count = dict(bytes=0, flops=0, launches=0)
    eng.arena = hrnet_hip.ActivationArena()
    x = torch.empty(shape, dtype=torch.bfloat16, device='meta').contiguous(memory_format=torch.channels_last)
    run(x)
    out = dict(eng.count, peak=eng.arena.peak)
    eng.count = eng.arena = None
    return out


def _uninitialised(build):
    """The module with storage but without the cost of initialising it: a walk reads shapes only.  The executors pack the convolutions
    of the un-folded module just as well (a missing bias packs as zeros), so BN folding is skipped too."""
    with torch.device('meta'):
        model = build()
    return model.to_empty(device='cpu')


def _walk_hrnet(cls, width, shape):
    meta = torch.device('meta')
    eng = cls.__new__(cls)
    eng.lib, eng.device, eng.tile_cfg, eng.multi_stream = MetaLib(), meta, -1, False
    model = _uninitialised(lambda: hrnet.PoseHighResolutionNet(width))
    cls._pack(eng, model, meta)
    out = {}
    for name in cls.CONFIGS:
        eng.apply_config(name)
        out['%s/%s' % (cls.__name__, name)] = _walk(eng, eng._features, shape)
    return out


def _walk_poseresnet():
    cls, meta = hrnet_hip.HipPoseResNet, torch.device('meta')
    eng = cls.__new__(cls)
    eng.lib, eng.device = None, meta
    model = _uninitialised(lambda: poseresnet.PoseResNet(50))
    cls._pack(eng, model, meta)
    out = {}
    for name in cls.CONFIGS:
        eng.apply_config(name)
        out['%s/%s' % (cls.__name__, name)] = _walk(eng, eng._features, (20, 8, 256, 192))
    return out


def _walk_darknet(arch, cfg):
    real_load = pam._lib.load
    pam._lib.load = lambda: NoLib()
    try:
        hd = yolov3.HipDarknet(_uninitialised(lambda: yolov3.Darknet(cfg())), torch.device('meta'))
    finally:
        pam._lib.load = real_load
    return {'HipDarknet/%s' % arch: _walk(hd, hd.forward, (5, 8, 416, 416))}


# network -> its shape-only walks {executor/configuration: dict(bytes, flops, launches, peak)}: 20 crops (HRNet-W48 at 384 x 288, the
# others at 256 x 192), the detectors on 5 views of 416 x 416
WALKS = {
    'hrnet_w48': lambda: _walk_hrnet(hrnet_hip.HipHRNet, 48, (20, 8, 384, 288)),
    'hrnet_w32': lambda: _walk_hrnet(hrnet_hip.HipHRNetW32, 32, (20, 8, 256, 192)),
    'poseresnet50': _walk_poseresnet,
    'darknet53': lambda: _walk_darknet('darknet53', yolov3.default_cfg),
    'yolov3_tiny': lambda: _walk_darknet('tiny', yolov3.tiny_cfg),
}


def walks():
    out = {}
    for net in sorted(WALKS):
        out.update(WALKS[net]())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'pack_digests.json')
    with open(path, 'w') as f:
        json.dump(dict(digests=pack_digests(), walks=walks()), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
