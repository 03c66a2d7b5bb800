#!/usr/bin/env python3
"""The YOLOv3-SPP block's launch (pam_spp_concat_nhwc_bf16: three stride-1 max-pools of one layer + the route over them), in ONE process,
forms interleaved, medians of --rounds rounds (tools/bench_flip.py's method: each form captured --iters times into one graph).  One
JSON line per shape (N x H x W x C, NHWC bf16; defaults: the 416 network's 5 x 13 x 13 x 512 and the 608 network's 2 x 19 x 19 x 512):
  slab8 .. slab64   the launch at each channel slab per workgroup (pam_spp_concat_slab_nhwc_bf16; a slab whose map does not fit the
                    workgroup's LDS runs as the next smaller one, `runs_as` says which)
  shipped           pam_spp_concat_nhwc_bf16 itself
  copy              a float4 copy of the launch's bytes (in + out read, the same written): the rate such a stream reaches here
  torch             what the launch replaces: three F.max_pool2d on the -inf-padded channels-last tensor + torch.cat"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import pam  # noqa: E402,F401
from pam import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='5x13x13x512,2x19x19x512')
ap.add_argument('--sizes', default='5,9,13')
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--iters', type=int, default=100)       # launches per captured replay: ~1 ms of work per timing
args = ap.parse_args()
dev = torch.device('cuda:0')
lib = _lib.load()
SIZES = tuple(int(s) for s in args.sizes.split(','))


def graph_of(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev); side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = _lib.new_graph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def us(g, iters):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record(); g.replay(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def case(n, h, w, c):
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(c + h)).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = torch.empty((n, 4 * c, h, w), dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
    nbytes = 2 * (x.numel() + y.numel())
    src = torch.zeros((nbytes // 2 // 16, 4), dtype=torch.float32, device=dev)        # half the bytes: the copy reads and writes them
    dst = torch.empty_like(src)

    def slab(s):
        def run():
            assert lib.pam_spp_concat_slab_nhwc_bf16(st(), p(x), p(y), n, h, w, c, *SIZES, s) == 0
        return run

    def shipped():
        assert lib.pam_spp_concat_nhwc_bf16(st(), p(x), p(y), n, h, w, c, *SIZES) == 0

    def composed():
        pools = [F.max_pool2d(F.pad(x, (s // 2,) * 4, value=float('-inf')), s, 1) for s in SIZES]
        return torch.cat(pools[::-1] + [x], 1)

    def copy():
        dst.copy_(src)
    shipped(); torch.cuda.synchronize()
    same = bool(torch.equal(y.float(), composed().float()))                 # -0.0 == 0.0 here: the contract's rule for zeros
    forms = dict([('slab%d' % s, slab(s)) for s in (8, 16, 32, 64)] + [('shipped', shipped), ('copy', copy), ('torch', composed)])
    graphs = {k: graph_of(fn, args.iters) for k, fn in forms.items()}
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k in forms:
            t[k].append(us(graphs[k], args.iters))
    m = {k: median(v) for k, v in t.items()}
    runs_as = {}
    for s in (8, 16, 32, 64):
        r = s
        while r > 8 and 2 * h * w * r * 2 > 65536:
            r //= 2
        runs_as['slab%d' % s] = r
    print(json.dumps(dict(bench='spp', shape=[n, h, w, c], sizes=SIZES, bytes=nbytes, us={k: round(v, 2) for k, v in m.items()},
                          runs_as=runs_as, workgroups={k: n * ((c + r - 1) // r) for k, r in runs_as.items()},
                          shipped_gbps=round(nbytes / m['shipped'] / 1e3, 1), copy_gbps=round(nbytes / m['copy'] / 1e3, 1),
                          shipped_over_torch=round(m['shipped'] / m['torch'], 3), shipped_over_copy=round(m['shipped'] / m['copy'], 3),
                          equals_torch=same)), flush=True)


for shp in args.shapes.split(','):
    case(*[int(v) for v in shp.split('x')])
