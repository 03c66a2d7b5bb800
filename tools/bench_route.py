#!/usr/bin/env python3
"""GPU timing of the general [route] launch (pam_route_concat_nhwc_bf16, k_route) at the route shapes of YOLOv4-tiny and YOLOv4 for 5
views of a 416 x 416 input, against a plain device copy (Tensor.copy_) of the same number of bytes (development tool).  One process,
the launches interleaved, medians over rounds; each timed region is one replay, between two events, of a captured graph of `iters`
launches (issued eagerly from Python a launch costs ~13 us of host time, more than most of these kernels run).  The buffers of
the largest shapes are tens of MB, far below the Infinity Cache: the rates are cache-resident rates, for both sides alike."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pam  # noqa: F401
from pam import _lib, hrnet_hip

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=5); ap.add_argument('--iters', type=int, default=50); ap.add_argument('--rounds', type=int, default=7)
args = ap.parse_args()
dev = torch.device('cuda:0')
# name, H = W, [(source channels, first channel, channels, x2)], padded output channels
SHAPES = [('tiny 3   group 32..63 of 64', 104, [(64, 32, 32, False)], 64), ('tiny 6   32 of 64 + 32 of 64', 104, [(64, 0, 32, False)] * 2, 64),
          ('tiny 8   64 + 64', 104, [(64, 0, 64, False)] * 2, 128), ('tiny 16  128 + 128', 52, [(128, 0, 128, False)] * 2, 256),
          ('tiny 24  256 + 256', 26, [(256, 0, 256, False)] * 2, 512), ('v4 9     64 + 64', 208, [(64, 0, 64, False)] * 2, 128),
          ('v4 53    128 + 128', 52, [(128, 0, 128, False)] * 2, 256), ('v4 103   512 + 512', 13, [(512, 0, 512, False)] * 2, 1024),
          ('v4 121   256 + up(256)', 26, [(256, 0, 256, False), (256, 0, 256, True)], 512),
          ('v4 131   128 + up(128)', 52, [(128, 0, 128, False), (128, 0, 128, True)], 256)]
e = hrnet_hip.ConvEngine()
e.lib = _lib.load(); e.device = dev


def captured(fn):
    """fn issued `iters` times into one graph -> the graph (the launches run back to back on replay)."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = _lib.new_graph()
    with torch.cuda.graph(g):
        for _ in range(args.iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g


def timed(g):
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record(); g.replay(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / args.iters * 1e3          # us per launch


for name, hw, spec, c_out in SHAPES:
    srcs = [(torch.randn((args.n, c, hw // 2 if up else hw, hw // 2 if up else hw), device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last), off, cnt, up)
            for c, off, cnt, up in spec]
    out_bytes = 2 * args.n * hw * hw * c_out
    moved = out_bytes + 2 * args.n * hw * hw * sum(cnt // (4 if up else 1) for _, _, cnt, up in spec)     # bytes read (an x2 source once) + written
    flat_a = torch.empty(moved // 2, dtype=torch.uint8, device=dev); flat_b = torch.empty_like(flat_a)
    out = torch.empty((args.n, c_out, hw, hw), dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
    e._new = lambda *a: out                                # one output for every launch: the graph needs no pool
    gr, gc = captured(lambda: e.route(srcs, c_out)), captured(lambda: flat_b.copy_(flat_a))
    tr, tc = [], []
    for _ in range(args.rounds):
        tr.append(timed(gr)); tc.append(timed(gc))
    r, c = statistics.median(tr), statistics.median(tc)
    print('%-30s %3dx%-3d -> %4d ch  %6.2f MB moved  k_route %7.2f us %6.2f TB/s   copy %7.2f us %6.2f TB/s   ratio %.2f' % (
        name, hw, hw, c_out, moved / 1e6, r, moved / r / 1e6, c, moved / c / 1e6, r / c))
