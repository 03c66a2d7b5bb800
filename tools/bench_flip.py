#!/usr/bin/env python3
"""The flip test's price, in ONE process, interleaved, medians of --rounds rounds.  One JSON line per result.
head: pam_head_decode_flip (flags 7, no heat-map pointer) on a batch of 2n feature rows against (a) the composed path -- two
pam_head_heatmaps launches, the torch flip / joint swap / shift / average, pam_decode_heatmaps -- (b) pam_head_decode on the n plain
rows, and (c) a float4 copy of the bytes the fused pass reads (the HBM rate such a stream reaches here), at C = 48, 96 x 72 and C = 256,
64 x 48.  Each form is captured --iters times into one graph.
--predict: whole captured predict() with flip_test on against off, W48 (384 x 288) and PoseResNet-50 (256 x 192)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pam  # noqa: E402,F401
from pam import _lib, hrnet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--boxes', type=int, default=20)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--predict', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')
lib = _lib.load()
PAIR = torch.tensor([0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15], device=dev)


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


def head_case(Cc, h, w, n):
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator().manual_seed(Cc)
    f = torch.randn((2 * n, Cc, h, w), generator=g).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = (0.2 * torch.randn((17, Cc), generator=g)).to(dev); b = torch.randn(17, generator=g).to(dev)
    view_of = torch.zeros(n, dtype=torch.int32, device=dev); slot_of = torch.arange(n, dtype=torch.int32, device=dev)
    boxes = torch.tensor([[10.0, 20.0, 100.0, 200.0]] * n, dtype=torch.float32, device=dev)
    det = torch.zeros((1, n, 17, 3), dtype=torch.float64, device=dev); det2 = torch.zeros_like(det)
    scratch = torch.empty((int(lib.pam_head_decode_flip_scratch_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    hm = torch.empty((2 * n, h, w, 17), dtype=torch.float32, device=dev)
    src = torch.zeros((2 * n * h * w * Cc // 8, 4), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    P = h * w

    def fused(flags=7):
        assert lib.pam_head_decode_flip(st(), n, n, h, w, p(f), Cc, p(wt), p(b), 17, flags, None, p(view_of), p(slot_of), p(boxes), n, p(det), None, p(scratch)) == 0

    def plain():
        assert lib.pam_head_decode(st(), n, h, w, p(f), Cc, p(wt), p(b), 17, None, p(view_of), p(slot_of), p(boxes), n, p(det), None, p(scratch)) == 0

    def composed():
        assert lib.pam_head_heatmaps(st(), n * P, p(f), Cc, p(wt), p(b), 17, p(hm)) == 0
        assert lib.pam_head_heatmaps(st(), n * P, C.c_void_p(f.data_ptr() + n * P * Cc * 2), Cc, p(wt), p(b), 17, C.c_void_p(hm.data_ptr() + n * P * 17 * 4)) == 0
        back = hm[n:].flip(2)[..., PAIR].clone()
        back[:, :, 1:] = back.clone()[:, :, :-1]
        m = ((hm[:n] + back) * 0.5).contiguous()
        assert lib.pam_decode_heatmaps(st(), n, p(m), 0, h, w, p(view_of), p(slot_of), p(boxes), n, p(det2), None) == 0

    def copy():
        dst.copy_(src)
    fused(3); composed(); torch.cuda.synchronize()
    same = bool(torch.equal(det, det2))                               # flags 3: what the composed path computes, bit for bit
    forms = dict(fused=fused, composed=composed, plain_n=plain, copy=copy)
    graphs = {k: graph_of(fn, args.iters) for k, fn in forms.items()}
    t = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k in forms:
            t[k].append(us(graphs[k], args.iters))
    m = {k: median(v) for k, v in t.items()}
    read = 2 * n * P * Cc * 2
    print(json.dumps(dict(bench='head', C=Cc, map=[h, w], boxes=n, us={k: round(v, 2) for k, v in m.items()},
                          fused_over_composed=round(m['fused'] / m['composed'], 3), fused_over_plain_n=round(m['fused'] / m['plain_n'], 3),
                          fused_gbps=round(read / m['fused'] / 1e3, 1), copy_gbps=round(2 * read / m['copy'] / 1e3, 1),
                          fused_share_of_copy_rate=round((read / m['fused']) / (2 * read / m['copy']), 3),
                          composed_equals_fused_without_offset=same)), flush=True)


def predict_case(name, kw, res, n):
    nets = {flip: hrnet.HRNetPose(*kw['args'], resolution=res, max_dets=8, max_crops=2 * n, flip_test=flip, post_process=flip,
                                  **{k: v for k, v in kw.items() if k != 'args'}) for flip in (False, True)}
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (776, 1032, 3), dtype=np.uint8)).to(dev) for _ in range(5)]
    pbl = [[dict(bbox=[40.0 + 60 * s, 50.0 + 30 * v, 180.0, 420.0], data=frames[v]) for s in range(n // 5)] for v in range(5)]
    t = {False: [], True: []}

    def run(net, iters):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(iters):
            d = net.predict(pbl, batch_size=n)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, d
    for flip in nets:
        run(nets[flip], 3)
    for _ in range(args.rounds):
        for flip in nets:
            t[flip].append(run(nets[flip], args.iters)[0])
    off, on = median(t[False]), median(t[True])
    print(json.dumps(dict(bench='predict', net=name, boxes=n, ms_off=round(off, 3), ms_on=round(on, 3), on_over_off=round(on / off, 3),
                          forward_crops=[nets[False].forward_crops(n), nets[True].forward_crops(n)])), flush=True)


head_case(48, 96, 72, args.boxes)
head_case(256, 64, 48, args.boxes)
if args.predict:
    predict_case('hrnet_w48_384x288', dict(args=(48, 17, None)), (384, 288), args.boxes)
    predict_case('pose_resnet50_256x192', dict(args=(50, 17, None), model_name='PoseResNet'), (256, 192), args.boxes)
