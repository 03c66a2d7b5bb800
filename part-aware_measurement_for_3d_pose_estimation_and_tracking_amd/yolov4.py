"""YOLOv4 and YOLOv4-tiny person detectors (Bochkovskiy, Wang & Liao 2020; the public Darknet cfg files -- parity unpinned, like yolov3's)
on the conv stack of yolov3.py.  ``YOLOv4`` has the constructor and call form of ``yolov3.YOLOv3`` and understands every cfg that class
understands -- a v3 cfg gives the same plan and the same bytes -- plus what the two networks need:

  [convolutional] activation=mish          activation code 3 of the convolution epilogue (csrc/pam_conv.hpp, epi_mish)
  [route] layers=L groups=G group_id=K     the K-th of G equal channel groups of layer L
  [route] over 2 .. 4 layers anywhere      one k_route launch (csrc/pam_route.hip): slices side by side, real channels compact
  [upsample] stride=2 anywhere             read through k_route's "nearest x2" flag by the routes that use it; materialised (a k_route of
                                           one source) only when another layer reads it
  [yolo] scale_x_y=s                       the decode's centre (sigmoid(t) * s - (s - 1) / 2 + cell) / grid (pam_yolo_detect_heads_sxy_ws)
  heads in any order                       anchors follow each head's own mask, grids its own layer

``yolov3.parse_cfg``, ``Darknet``, ``HipDarknet``, ``YOLOv3`` and ``ARCHS`` keep their behaviour, refusals included; the classes here are
subclasses that replace the constructors.  A group route is COPIED by k_route, not handed on as a channel-offset view: the 3x3 kernels
(k_conv3x3s, k_conv3x3) take whole tensors only, so a view would move the convolution behind it to the generic implicit GEMM, and the
copy of a half-width slice costs less than that."""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, yolov3
from .hrnet_hip import PackedConv, TileCfg
from .yolov3 import _layer_sizes, _round_channels, _spp_block, darknet_maxpool, fold_conv

TINY_ANCHORS = yolov3.TINY_ANCHORS
ANCHORS = [(12, 16), (19, 36), (40, 28), (36, 75), (76, 55), (72, 146), (142, 110), (192, 243), (459, 401)]
ROUTE_MAX_SRC = 4           # PAM_ROUTE_MAX_SRC in include/pam.h


# ---- cfg ------------------------------------------------------------------------------------------------------------
class _Cfg(object):
    """The lines of a cfg under construction."""

    def __init__(self, width, height, anchors, classes):
        self.out = ['[net]', 'width=%d' % width, 'height=%d' % height, 'channels=3', '']
        self.anchors, self.classes = anchors, classes

    def conv(self, filters, size, stride=1, bn=1, act='leaky'):
        self.out.extend(['[convolutional]'] + (['batch_normalize=1'] if bn else []) +
                        ['filters=%d' % filters, 'size=%d' % size, 'stride=%d' % stride, 'pad=1', 'activation=%s' % act, ''])

    def route(self, *layers, **groups):
        self.out.extend(['[route]', 'layers = %s' % ', '.join(str(l) for l in layers)] +
                        (['groups=%d' % groups['groups'], 'group_id=%d' % groups['group_id']] if groups else []) + [''])

    def add(self, *lines):
        self.out.extend(list(lines) + [''])

    def head(self, mask, scale):
        self.conv(3 * (5 + self.classes), 1, bn=0, act='linear')
        self.add('[yolo]', 'mask = %s' % ','.join(str(m) for m in mask), 'anchors = %s' % ',  '.join('%d,%d' % a for a in self.anchors),
                 'classes=%d' % self.classes, 'num=%d' % len(self.anchors), 'jitter=.3', 'ignore_thresh = .7', 'truth_thresh = 1', 'random=0',
                 'scale_x_y = %s' % scale, 'iou_thresh=0.213', 'cls_normalizer=1.0', 'iou_normalizer=0.07', 'iou_loss=ciou',
                 'nms_kind=greedynms', 'beta_nms=0.6')

    def text(self):
        return '\n'.join(self.out)


def yolov4_tiny_cfg(width=416, height=416, classes=80):
    """The standard yolov4-tiny.cfg (38 layers, 21 convolutions, 6 062 814 weights: three CSP blocks of group routes, two heads with
    scale_x_y = 1.05; the second head's mask 1,2,3 is the public file's), generated rather than shipped."""
    c = _Cfg(width, height, TINY_ANCHORS, classes)
    c.conv(32, 3, 2); c.conv(64, 3, 2); c.conv(64, 3)
    for f in (64, 128, 256):
        if f != 64:
            c.conv(f, 3)
        c.route(-1, groups=2, group_id=1)
        c.conv(f // 2, 3); c.conv(f // 2, 3)
        c.route(-1, -2)
        c.conv(f, 1)
        c.route(-6, -1)
        c.add('[maxpool]', 'size=2', 'stride=2')
    c.conv(512, 3); c.conv(256, 1); c.conv(512, 3)
    c.head((3, 4, 5), '1.05')
    c.route(-4)
    c.conv(128, 1)
    c.add('[upsample]', 'stride=2')
    c.route(-1, 23)
    c.conv(256, 3)
    c.head((1, 2, 3), '1.05')
    return c.text()


def yolov4_cfg(width=416, height=416, classes=80):
    """The standard yolov4.cfg (162 layers, 110 convolutions, 64 429 405 weights: the CSPDarknet53 backbone with mish as layers 0 .. 104,
    YOLOv3-SPP's pooling block, the PAN neck with leaky convolutions, three heads listed finest first with scale_x_y 1.2 / 1.1 / 1.05)."""
    c = _Cfg(width, height, ANCHORS, classes)
    m = 'mish'
    c.conv(32, 3, act=m)
    for f, n in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        half = f if f == 64 else f // 2          # the first stage keeps 64 channels on both arms, its blocks squeeze to 32
        c.conv(f, 3, 2, act=m)
        c.conv(half, 1, act=m)
        c.route(-2)
        c.conv(half, 1, act=m)
        for _ in range(n):
            c.conv(32 if f == 64 else half, 1, act=m); c.conv(half, 3, act=m)
            c.add('[shortcut]', 'from=-3', 'activation=linear')
        c.conv(half, 1, act=m)
        c.route(-1, -(4 + 3 * n))
        c.conv(f, 1, act=m)
    c.conv(512, 1); c.conv(1024, 3); c.conv(512, 1)
    for size, back in ((5, -2), (9, -4), (13, None)):
        c.add('[maxpool]', 'stride=1', 'size=%d' % size)
        if back is not None:
            c.route(back)
        else:
            c.route(-1, -3, -5, -6)
    c.conv(512, 1); c.conv(1024, 3); c.conv(512, 1)
    for f, skip in ((256, 85), (128, 54)):
        c.conv(f, 1)
        c.add('[upsample]', 'stride=2')
        c.route(skip)
        c.conv(f, 1)
        c.route(-1, -3)
        for k in range(5):
            c.conv(f * 2 if k & 1 else f, 3 if k & 1 else 1)
    c.conv(256, 3)
    c.head((0, 1, 2), '1.2')
    for f, back, mask, scale in ((256, -16, (3, 4, 5), '1.1'), (512, -37, (6, 7, 8), '1.05')):
        c.route(-4)
        c.conv(f, 3, 2)
        c.route(-1, back)
        for k in range(5):
            c.conv(f * 2 if k & 1 else f, 3 if k & 1 else 1)
        c.conv(f * 2, 3)
        c.head(mask, scale)
    return c.text()


ARCHS4 = dict(yolov3.ARCHS)
ARCHS4.update({'yolov4': yolov4_cfg, 'yolov4-tiny': yolov4_tiny_cfg})


def parse_cfg(text):
    """yolov3.parse_cfg plus the keys of the YOLOv4 cfgs: [route] groups / group_id, [yolo] scale_x_y, new_coords, nms_kind.  Training-only
    keys stay unread strings, as there."""
    net, layers = yolov3.parse_cfg(text)
    for i, b in enumerate(layers):
        if b['type'] == 'route':
            b['groups'], b['group_id'] = int(b.get('groups', 1)), int(b.get('group_id', 0))
            if b['groups'] < 1 or not 0 <= b['group_id'] < b['groups']:
                raise ValueError('[route] layer %d: groups=%d group_id=%d' % (i, b['groups'], b['group_id']))
            if b['groups'] > 1 and len(b['layers']) != 1:
                raise NotImplementedError('[route] layer %d: groups=%d over %d layers (a group route takes one layer)' % (i, b['groups'], len(b['layers'])))
            if not 1 <= len(b['layers']) <= ROUTE_MAX_SRC:
                raise NotImplementedError('[route] layer %d: layers= names %d sources, the route kernel takes 1 to %d' % (i, len(b['layers']), ROUTE_MAX_SRC))
        elif b['type'] == 'yolo':
            b['scale_x_y'] = float(b.get('scale_x_y', 1.0))
            if not (1.0 <= b['scale_x_y'] < float('inf')):
                raise ValueError('[yolo] layer %d: scale_x_y=%r must be finite and >= 1' % (i, b['scale_x_y']))
            if int(b.get('new_coords', 0)) != 0:
                raise NotImplementedError('[yolo] layer %d: new_coords=1 (the scaled-YOLOv4 box coding) is not supported' % i)
            if b.get('nms_kind', 'greedynms') not in ('greedynms', 'default'):
                raise NotImplementedError('[yolo] layer %d: nms_kind=%s: only greedynms (what the decode kernel does) is supported' % (i, b['nms_kind']))
    return net, layers


def _sources(b, i):
    return [l if l >= 0 else i + l for l in b['layers']]


# ---- float32 PyTorch form ---------------------------------------------------------------------------------------------------------------
class Darknet4(yolov3.Darknet):
    """yolov3.Darknet with mish convolutions and group routes; the same module names, so weights and state dicts are interchangeable."""

    def __init__(self, cfg_text=None):
        nn.Module.__init__(self)
        self.net, self.layers = parse_cfg(cfg_text if cfg_text is not None else yolov4_cfg())
        self.width, self.height = int(self.net.get('width', 416)), int(self.net.get('height', 416))
        chans = []
        mods = nn.ModuleList()
        c_in = int(self.net.get('channels', 3))
        for i, b in enumerate(self.layers):
            m = nn.Sequential()
            t = b['type']
            if t == 'convolutional':
                pad = (b['size'] - 1) // 2 if b['pad'] else 0
                m.add_module('conv', nn.Conv2d(c_in, b['filters'], b['size'], b['stride'], pad, bias=not b['batch_normalize']))
                if b['batch_normalize']:
                    m.add_module('bn', nn.BatchNorm2d(b['filters']))
                if b['activation'] == 'leaky':
                    m.add_module('act', nn.LeakyReLU(0.1))
                elif b['activation'] == 'mish':
                    m.add_module('act', nn.Mish())
                elif b['activation'] != 'linear':
                    raise NotImplementedError('activation %s' % b['activation'])
                c_out = b['filters']
            elif t == 'route':
                c_out = sum(chans[l] for l in _sources(b, i))
                if c_out % b['groups'] != 0:
                    raise ValueError('[route] layer %d: groups=%d does not divide its %d channels' % (i, b['groups'], c_out))
                c_out //= b['groups']
            else:                       # shortcut, upsample, maxpool, yolo
                c_out = chans[i - 1]
            mods.append(m)
            chans.append(c_out)
            c_in = c_out
        self.mods, self.chans = mods, chans

    def forward(self, x):
        """x: (N, 3, H, W) float RGB in [0, 1] -> raw head tensors [(N, 3*(5+nc), g_h, g_w)] in cfg order."""
        outs, heads = [], []
        for i, (b, m) in enumerate(zip(self.layers, self.mods)):
            t = b['type']
            if t == 'convolutional':
                x = m(x)
            elif t == 'shortcut':
                x = outs[i - 1] + outs[i + b['from']]
            elif t == 'route':
                xs = [outs[l] for l in _sources(b, i)]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, 1)
                if b['groups'] > 1:
                    x = torch.chunk(x, b['groups'], 1)[b['group_id']]
            elif t == 'upsample':
                x = F.interpolate(x, scale_factor=b['stride'], mode='nearest')
            elif t == 'maxpool':
                x = darknet_maxpool(x, b['size'], b['stride'])
            else:
                heads.append(x)
            outs.append(x)
        return heads


# ---- product path -----------------------------------------------------------------------------------------------------------------------
class HipDarknet4(yolov3.HipDarknet):
    """yolov3.HipDarknet's plan with three more things: convolutions with activation 'mish', ``('route', layer, [(source layer, first
    channel, channels, x2 flag)], padded channels)`` steps on k_route, and [upsample] layers that only routes read (no step: the routes read
    the half-size map through the x2 flag).  A cfg that yolov3.HipDarknet takes gives the same steps."""

    def __init__(self, model, device):
        self.lib = _lib.load()
        self.device = device
        self.count = None
        self.tile_cfg = TileCfg.AUTO
        self.unfuse_wide = True
        layers = model.layers
        n = len(layers)
        used_by = [[] for _ in range(n)]                 # consumers of each layer's output other than the next layer
        for i, b in enumerate(layers):
            if b['type'] == 'shortcut':
                used_by[i + b['from']].append(i)
            elif b['type'] == 'route':
                for l in _sources(b, i):
                    used_by[l].append(i)
        self.plan, real, padded = [], [], []
        self.head_scales = [float(b.get('scale_x_y', 1.0)) for b in layers if b['type'] == 'yolo']
        sizes = _layer_sizes(model)
        lazy_up = {}                                     # [upsample] layer that has no tensor -> the half-size layer it doubles
        c_pad = 8
        i = 0
        while i < n:
            b, t = layers[i], layers[i]['type']
            if t in ('convolutional', 'shortcut', 'maxpool', 'yolo', 'upsample') and i - 1 in lazy_up:
                raise AssertionError('layer %d reads an [upsample] that was not materialised' % i)       # _materialise decides this below
            if t == 'convolutional':
                cin_pad = c_pad if i == 0 else padded[i - 1]
                stem = i == 0 and cin_pad == 8 and b['size'] == 3 and b['pad'] and b['stride'] in (1, 2) and b['filters'] in (16, 32, 64)
                if stem and b['activation'] == 'mish' and b['stride'] != 1:
                    stem = False                            # k_conv_stem's mish form is stride 1 (YOLOv4's layer 0): the generic kernel takes it
                if b['activation'] not in ('leaky', 'linear', 'mish'):
                    raise NotImplementedError('layer %d: activation %s' % (i, b['activation']))
                op = PackedConv(fold_conv(model.mods[i]), device, pad_cin_to=cin_pad,
                                pad_cout_to=(32 if b['filters'] == 16 else None) if stem else _round_channels(b['filters']))
                nxt = layers[i + 1] if i + 1 < n else None
                fuse = nxt is not None and nxt['type'] == 'shortcut' and nxt['activation'] == 'linear' and used_by[i] == []
                if fuse:                                    # conv + activation, then + skip: one launch produces layer i+1
                    self.plan.append(('conv', i + 1, op, i - 1, b['activation'], i + 1 + nxt['from']))
                    real += [b['filters'], b['filters']]; padded += [op.cout, op.cout]
                    i += 2
                    continue
                self.plan.append(('conv', i, op, i - 1, b['activation'], None))
                real.append(b['filters']); padded.append(op.cout)
            elif t == 'shortcut':
                self.plan.append(('add', i, i - 1, i + b['from']))
                real.append(real[i - 1]); padded.append(padded[i - 1])
            elif t == 'route':
                src = _sources(b, i)
                if len(src) == 1 and b['groups'] == 1 and src[0] not in lazy_up:
                    self.plan.append(('alias', i, src[0]))
                    real.append(real[src[0]]); padded.append(padded[src[0]])
                else:
                    parts = []
                    for l in src:
                        cnt = real[l]
                        if cnt % b['groups'] != 0:
                            raise ValueError('[route] layer %d: groups=%d does not divide the %d channels of layer %d' % (i, b['groups'], cnt, l))
                        cnt //= b['groups']
                        if cnt % 8 != 0:
                            raise NotImplementedError('[route] layer %d: a slice of %d channels of layer %d: the route kernel copies multiples of 8 channels' %
                                                      (i, cnt, l))
                        parts.append((lazy_up.get(l, l), cnt * b['group_id'], cnt, l in lazy_up))
                    if len({sizes[l] for l in src}) != 1:
                        raise ValueError('[route] layer %d: its sources have different sizes %s' % (i, [sizes[l] for l in src]))
                    c = sum(p[2] for p in parts)
                    self._check_route(i, sizes[i], _round_channels(c))
                    self.plan.append(('route', i, parts, _round_channels(c)))
                    real.append(c); padded.append(_round_channels(c))
            elif t == 'upsample':
                nxt = layers[i + 1] if i + 1 < n else None
                if b['stride'] != 2:
                    raise NotImplementedError('[upsample] layer %d: stride=%d, only stride=2 is supported' % (i, b['stride']))
                upcat = (nxt is not None and nxt['type'] == 'route' and len(nxt['layers']) == 2 and nxt['groups'] == 1 and
                         nxt['layers'][0] in (-1, i) and used_by[i] == [i + 1])
                if upcat:
                    skip = _sources(nxt, i + 1)[1]
                    upcat = real[i - 1] == padded[i - 1] and real[skip] == padded[skip] and skip not in lazy_up
                if upcat:                                   # yolov3's step: upsample + route -1, <skip> in one launch of k_upsample_concat
                    self.plan.append(('upcat', i + 1, i - 1, skip))
                    real += [real[i - 1], real[i - 1] + real[skip]]; padded += [padded[i - 1], padded[i - 1] + padded[skip]]
                    i += 2
                    continue
                only_routes = (nxt is None or nxt['type'] == 'route') and all(
                    layers[u]['type'] == 'route' and (len(layers[u]['layers']) > 1 or layers[u]['groups'] > 1) for u in used_by[i])
                if only_routes:                             # nothing reads it but k_route launches: they double the half-size map themselves
                    lazy_up[i] = i - 1
                else:                                       # a stand-alone upsample: k_route with one x2 source
                    if real[i - 1] % 8 != 0:
                        raise NotImplementedError('[upsample] layer %d: %d channels: the route kernel copies multiples of 8 channels' % (i, real[i - 1]))
                    self._check_route(i, sizes[i], padded[i - 1])
                    self.plan.append(('route', i, [(i - 1, 0, real[i - 1], True)], padded[i - 1]))
                real.append(real[i - 1]); padded.append(padded[i - 1])
            elif t == 'maxpool' and _spp_block(layers, i, used_by) is not None:
                src, pools = i - 1, _spp_block(layers, i, used_by)
                if real[src] != padded[src]:
                    raise NotImplementedError('SPP block over a channel-padded layer (%d of %d channels real)' % (real[src], padded[src]))
                if max(sizes[src]) > _lib.SPP_MAX_HW:
                    raise NotImplementedError('SPP block on a %d x %d map: the kernel holds maps up to %d a side (network inputs up to %d)' %
                                              (sizes[src] + (_lib.SPP_MAX_HW, 32 * _lib.SPP_MAX_HW)))
                self.plan.append(('spp', i + 5, src, pools))
                real += [real[src]] * 5 + [4 * real[src]]; padded += [padded[src]] * 5 + [4 * padded[src]]
                i += 6
                continue
            elif t == 'maxpool':
                if b['size'] not in (2, 3) or b['stride'] not in (1, 2):
                    raise NotImplementedError('[maxpool] size=%d stride=%d: the max-pool kernel takes size 2 or 3 and stride 1 or 2' %
                                              (b['size'], b['stride']))
                self.plan.append(('pool', i, i - 1, b['size'], b['stride']))
                real.append(real[i - 1]); padded.append(padded[i - 1])
            else:                                           # yolo
                self.plan.append(('head', i, i - 1))
                real.append(real[i - 1]); padded.append(padded[i - 1])
            i += 1
        self.real, self.padded = real, padded

    @staticmethod
    def _check_route(i, hw, c_pad, views=64):
        """k_route's piece index is 32-bit: refuse, while the plan is built, a layer whose output could not be indexed at `views` views."""
        if views * hw[0] * hw[1] * (c_pad // 8) >= 1 << 31:
            raise NotImplementedError('[route] layer %d: %d x %d x %d channels at %d views exceeds the route kernel\'s 2^31 16-byte pieces' %
                                      ((i,) + tuple(hw) + (c_pad, views)))

    def run_step(self, step, outs):
        if step[0] == 'route':
            return self.route([(outs[l], off, cnt, up) for l, off, cnt, up in step[2]], step[3])
        return super(HipDarknet4, self).run_step(step, outs)


class YOLOv4(yolov3.YOLOv3):
    """``yolov3.YOLOv3`` over Darknet4 / HipDarknet4: the same constructor arguments and call form, graph replay, ``detect_dev``,
    ``submit`` / ``collect`` and ``frame_buffer``; arch is one of ARCHS4's five names (a cfg file always decides); the decode applies each
    head's scale_x_y."""

    def __init__(self, cfgfile=None, weightfile=None, namesfile=None, score_thresh=0.7, nms_thresh=0.45, use_cuda=True,
                 device=0, max_det=64, seed=0, use_graph=True, arch='yolov4'):
        super(YOLOv4, self).__init__(cfgfile, weightfile, namesfile, score_thresh=score_thresh, nms_thresh=nms_thresh, use_cuda=use_cuda,
                                     device=device, max_det=max_det, seed=seed, use_graph=use_graph, arch=arch)

    @staticmethod
    def _flavour():
        return ARCHS4, Darknet4, HipDarknet4

    def _decode(self, st, n, nh, hp, gh, gw, cs, an, W, H, fw, fh, boxes, count, ws, need):
        return self.lib.pam_yolo_detect_heads_sxy_ws(
            C.c_void_p(st), n, nh, hp, gh, gw, cs, an.ctypes.data_as(C.c_void_p), self.scale_xy.ctypes.data_as(C.c_void_p), W, H, self.num_classes,
            self.class_id, self.score_thresh, self.nms_thresh, fw, fh, self.max_det,
            C.c_void_p(boxes.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(ws.data_ptr()), need), 'pam_yolo_detect_heads_sxy_ws'
