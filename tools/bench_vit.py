#!/usr/bin/env python3
"""ViTPose-B / -L (256 x 192) beside HRNet-W48 (384 x 288), HRNet-W32 and PoseResNet-50 (256 x 192) in ONE process, interleaved over
rounds, medians: the captured (hipGraph) feature forward at --crops crops; each token kernel of csrc/pam_vit.hip alone at the
networks' shapes; and pam_vit_linear_bf16 beside ConvEngine.conv (the implicit-GEMM 1x1 form) for the three GELU-free linear shapes of
a block -- qkv, proj + residual, fc2 + residual --, so that a later change of the linear path can decide with numbers.
--only forward | kernels | linear -> that part alone; --variants B -> ViTPose-B alone.  One JSON line per result."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import pam  # noqa: E402,F401
from pam import _lib, hrnet, hrnet_hip, packing, poseresnet, vitpose  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA peak (public spec)
ap = argparse.ArgumentParser()
ap.add_argument('--crops', type=int, default=20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--variants', default='B,L')
ap.add_argument('--only', default='forward,kernels,linear')
args = ap.parse_args()
dev = torch.device('cuda:0')
variants = [v for v in args.variants.split(',') if v]
parts = args.only.split(',')


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def interleaved(cases):
    """cases: {name: zero-argument launch} -> {name: sorted ms over the rounds}, the cases taking turns inside every round"""
    out = {}
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in cases.items():
            fn()
            out.setdefault(name, []).append(timed(fn, args.iters))
    return {k: sorted(v) for k, v in out.items()}


def line(kind, name, ms, flops=None, nbytes=None, **kw):
    med = ms[len(ms) // 2]
    d = dict(kind=kind, name=name, ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_all=[round(q, 4) for q in ms], **kw)
    if flops:
        d.update(tflops=round(flops / med / 1e9, 1), mfma_peak_share=round(flops / med / 1e9 / PEAK_BF16_TFLOPS, 4))
    if nbytes:
        d.update(gbytes_per_s=round(nbytes / med / 1e6, 1))
    print(json.dumps(d), flush=True)


n = args.crops
if 'forward' in parts:
    models = {'ViTPose-' + v: ('ViTPose', v, (256, 192)) for v in variants}
    models.update({'W48': ('HRNet', 48, (384, 288)), 'W32': ('HRNet', 32, (256, 192)), 'R50': ('PoseResNet', 50, (256, 192))})
    cases, flops = {}, {}
    for name, (family, c, res) in models.items():
        net = hrnet.HRNetPose(c, 17, None, model_name=family, resolution=res, use_graph=True, max_crops=n)
        x = net.input_buffer(n)
        x.zero_()
        x[:, :3].copy_(torch.randn((n, 3) + res, generator=torch.Generator().manual_seed(n)).to(x.dtype).to(dev))
        net.features(x)                                         # capture
        flops[name] = (vitpose.count_flops(c) if family == 'ViTPose' else poseresnet.count_flops(c, res) if family == 'PoseResNet'
                       else hrnet.count_flops(c, 17, res[0], res[1]))
        cases[name] = lambda net=net, x=x: net.features(x)
    for name, ms in interleaved(cases).items():
        line('forward', name, ms, flops=flops[name] * n, crops=n, gflop_per_crop=round(flops[name] / 1e9, 3))

eng = hrnet_hip.HipViTPose.__new__(hrnet_hip.HipViTPose)
eng.lib, eng.device, eng.count = _lib.load(), dev, None
g = torch.Generator().manual_seed(0)


def tokens(c):
    """a (crops, c, 16, 12) channels-last bf16 token tensor of N(0, 1) values"""
    return torch.randn((n, 16, 12, c), generator=g).to(torch.bfloat16).to(dev).permute(0, 3, 1, 2)


def linear_op(k, m):
    return packing.PackedLinear(torch.randn((m, k), generator=g) * 0.02, torch.randn(m, generator=g) * 0.1, dev)


def keep(fn):
    """launches through the engine allocate their output per call: the timed closure drops it again"""
    def run():
        eng._keep = None
        fn()
    return run


if 'kernels' in parts:
    for v in variants:
        d, heads = vitpose.VARIANTS[v]['dim'], vitpose.VARIANTS[v]['heads']
        M = n * 192
        x8 = torch.zeros((n, 8, 256, 192), dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
        x8[:, :3] = torch.randn((n, 3, 256, 192), generator=g).to(torch.bfloat16).to(dev)
        pe = packing.PackedLinear(torch.randn((d, 2048), generator=g) * 0.02, None, dev)
        pos = torch.randn((192, d), generator=g).to(dev)
        ln = (torch.ones(d, device=dev), torch.zeros(d, device=dev), 1e-6)
        xd, x3, x4 = tokens(d), tokens(3 * d), tokens(4 * d)
        ops = dict(qkv=linear_op(d, 3 * d), proj=linear_op(d, d), fc1=linear_op(d, 4 * d), fc2=linear_op(4 * d, d))
        cases = {
            'patch_embed': (keep(lambda: eng.patch_embed(pe, pos, x8)), 2 * M * d * 768, 2 * (x8.numel() + M * d + d * 2048)),
            'layernorm': (keep(lambda: eng.layernorm(ln, xd)), 0, 4 * M * d),
            'linear qkv': (keep(lambda: eng.linear(ops['qkv'], xd)), 2 * M * d * 3 * d, 2 * (M * 4 * d + 3 * d * d)),
            'linear proj + residual': (keep(lambda: eng.linear(ops['proj'], xd, res=xd)), 2 * M * d * d, 2 * (M * 3 * d + d * d)),
            'linear fc1 + GELU': (keep(lambda: eng.linear(ops['fc1'], xd, gelu=True)), 2 * M * d * 4 * d, 2 * (M * 5 * d + 4 * d * d)),
            'linear fc2 + residual': (keep(lambda: eng.linear(ops['fc2'], x4, res=xd)), 2 * M * d * 4 * d, 2 * (M * 6 * d + 4 * d * d)),
            'attention': (keep(lambda: eng.attention(x3, heads)), 4 * n * heads * 192 * 192 * 64, 2 * M * 4 * d),
        }
        for name, ms in interleaved({k: c[0] for k, c in cases.items()}).items():
            line('kernel', name, ms, flops=cases[name][1], nbytes=cases[name][2], variant=v, crops=n, M=M, D=d)

if 'linear' in parts:
    for v in variants:
        d = vitpose.VARIANTS[v]['dim']
        M = n * 192
        xd, x4 = tokens(d), tokens(4 * d)
        cases = {}
        for name, k, m, x, res in (('qkv', d, 3 * d, xd, None), ('proj + residual', d, d, xd, xd), ('fc2 + residual', 4 * d, d, x4, xd)):
            conv = torch.nn.Conv2d(k, m, 1)
            cases['linear ' + name] = keep(lambda op=packing.PackedLinear(conv.weight.reshape(m, k), conv.bias, dev), x=x, res=res:
                                           eng.linear(op, x, res=res))
            cases['conv ' + name] = keep(lambda op=packing.PackedConv(conv, dev), x=x, res=res: eng.conv(op, x, res=res))
            cases['flops ' + name] = 2 * M * k * m
        fl = {k[6:]: c for k, c in cases.items() if k.startswith('flops ')}
        for name, ms in interleaved({k: c for k, c in cases.items() if not k.startswith('flops ')}).items():
            line('linear_vs_conv', name, ms, flops=fl[name.split(' ', 1)[1]], variant=v, crops=n, M=M)
