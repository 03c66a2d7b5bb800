"""What the conv-plan table and its tests launch (tools/record_conv_plans.py, tests/test_conv_plan.py, tests/test_gpu_conv_plan.py).

``ConvSpy`` wraps the library like ``Spy`` of tests/test_gpu_darknet_layers.py: every ``pam_conv2d_nhwc_bf16_ex`` call is reported to a
callback as (query, return code), the query being the call's integer arguments and the presence of its five pointers (``COLUMNS``).
``drive_networks`` runs forwards of the six networks with random weights through a spy, ``drive_cases`` the convolution cases of
tests/exact_ref.py over every tile code.  Nothing here compares numbers: tests/test_gpu_exact.py owns the bits."""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import exact_ref as E  # noqa: E402

INTS = ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad', 'relu', 'tile_cfg', 'in_cstride', 'relu_from')
FLAGS = ('has_in', 'has_w_packed', 'has_w_img', 'has_residual', 'has_out')
COLUMNS = INTS + FLAGS + ('rc', 'kernel', 'form')        # a row of tests/golden/conv_plan.json; kernel / form are null when rc != 0
ENTRY = 'pam_conv2d_nhwc_bf16_ex'


def _present(p):
    return int(bool(p.value if hasattr(p, 'value') else p))


def query_of(args):
    """The arguments of one pam_conv2d_nhwc_bf16_ex call -> the 13 integers and 5 presence flags of COLUMNS."""
    _, x, w, wimg, _, res, out = args[:7]
    return tuple(int(v) for v in args[7:20]) + tuple(_present(p) for p in (x, w, wimg, res, out))


class ConvSpy(object):
    """The library with its conv entry reported: on_conv(query, rc) right after every call returns."""

    def __init__(self, lib, on_conv):
        self._lib, self._on_conv = lib, on_conv

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != ENTRY:
            return fn

        def launch(*args):
            rc = fn(*args)
            self._on_conv(query_of(args), rc)
            return rc
        return launch


def x8(n, h, w, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros((n, 8, h, w))
    x[:, :3] = torch.rand((n, 3, h, w), generator=g)
    return x.to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)


def _pose_nets(dev):
    """(name, constructor of the executor, input height, width): the shipped pose networks with random weights."""
    from pam import hrnet, hrnet_hip, poseresnet
    yield 'hrnet_w48', lambda: hrnet_hip.HipHRNet(hrnet.fold_batchnorm(hrnet.init_random(hrnet.PoseHighResolutionNet(48, 17), seed=0)), dev), 384, 288
    yield 'hrnet_w32', lambda: hrnet_hip.HipHRNetW32(hrnet.fold_batchnorm(hrnet.init_random(hrnet.PoseHighResolutionNet(32, 17), seed=0)), dev), 256, 192
    yield 'poseresnet50', lambda: hrnet_hip.HipPoseResNet(poseresnet.folded_random_model(50), dev), 256, 192


def _detectors(dev):
    from pam import yolov3
    for name, cfg in (('darknet53', yolov3.default_cfg), ('yolov3_tiny', yolov3.tiny_cfg), ('yolov3_spp', yolov3.spp_cfg)):
        yield name, lambda cfg=cfg: yolov3.HipDarknet(yolov3.Darknet(cfg()).init_random(0).eval(), dev), 416, 416


def drive_networks(wrap, dev, crops=(2,), views=(1,), all_configs=False, log=None):
    """One forward per network, crop / view count and (all_configs) named executor configuration, the executor's library replaced by
    wrap(library)."""
    for nets, counts, is_pose in ((_pose_nets(dev), crops, True), (_detectors(dev), views, False)):
        for name, make, h, w in nets:
            hip = make()
            hip.lib = wrap(hip.lib)
            configs = list(hip.CONFIGS) if (all_configs and hip.CONFIGS) else [hip.config_name]
            for cfg in configs:
                if cfg is not None:
                    hip.apply_config(cfg)
                for n in counts:
                    if log:
                        log('%s %s n=%d' % (name, cfg, n))
                    with torch.no_grad():
                        hip.features(x8(n, h, w, dev)) if is_pose else hip.forward(x8(n, h, w, dev))
                    torch.cuda.synchronize()
                    hip._keep = None
            del hip
            torch.cuda.empty_cache()


def _engine(wrap, dev, plain, **attrs):
    from pam import _lib, hrnet_hip
    e = hrnet_hip.ConvEngine() if plain else hrnet_hip.HipHRNet.__new__(hrnet_hip.HipHRNet)
    e.lib, e.device, e._keep = wrap(_lib.load()), dev, []
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


def case_launches():
    """(case, engine attributes) of every launch drive_cases issues: each CONV_CASES case with its own variants, then over every code of
    ALL_TILES (the pairs exact_ref.tile_refused names included), and a 96 -> 96 layer under the code -6, which no executor states."""
    for c in E.CONV_CASES:
        for v in c['variants']:
            yield c, {k: a for k, a in v.items() if k not in ('kernel', 'image')}
        for t in E.ALL_TILES:
            yield c, dict(tile_cfg=t)
    yield next(c for c in E.CONV_CASES if c['id'] == 'c96-ragged'), dict(tile_cfg=-6)


def drive_cases(wrap, dev):
    """Every launch of case_launches() at the case's own shape with random operands; a refusal (PamError) is what the spy records."""
    from pam import _lib, hrnet_hip
    ops = {}
    for c, attrs in case_launches():
        if c['id'] not in ops:
            g = torch.Generator().manual_seed(len(ops))
            conv = nn.Conv2d(c['cin'], c['cout'], c['k'], c['stride'], c['k'] // 2, bias=True)
            wide, off = c.get('wide', c['cin']), c.get('off', 0)
            xw = torch.randn((c['n'], wide, c['h'], c['w']), generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
            ho, wo = E.out_hw(c['h'], c['w'], c['k'], c['stride'])
            res = torch.randn((c['n'], c['cout'], ho, wo), generator=g).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
            ops[c['id']] = (hrnet_hip.PackedConv(conv, dev), xw[:, off:off + c['cin']] if wide != c['cin'] else xw, res)
        op, x, res = ops[c['id']]
        e = _engine(wrap, dev, c['launch'] == 'plain' and 'tile_cfg' not in attrs, **attrs)
        e.down48 = e.tile_cfg == -1                  # as tests/test_gpu_exact.py: a stated tile keeps the strided 48-channel layers on the generic kernels
        try:
            e.conv(op, x, res=res if c.get('res', 'none') != 'none' else None, relu=c.get('act', 'relu'),
                   res_after_act=c.get('res') == 'after', relu_from=c.get('relu_from', 0))
        except _lib.PamError:
            pass
        torch.cuda.synchronize()
