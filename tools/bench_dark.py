#!/usr/bin/env python3
"""The DARK decode's price, in ONE process, interleaved, medians of --rounds rounds.  One JSON line per result.
head: pam_head_decode_dark at flags 0 and 3 against pam_head_decode_flip at flags 4 and 7 (the quarter-cell decoders it replaces: the
yardstick for the option's price) and the composed path -- pam_head_heatmaps, the full-map Gaussian blur in torch (float64, zero
padding), the logarithm, and the Taylor step on the host -- at C = 48, 96 x 72, k = 17 and C = 256, 64 x 48, k = 11.  Each device form is
captured --iters times into one graph; the composed path cannot be captured (it ends on the host) and is timed eagerly, wall clock.
The features carry one blob per (crop, joint) so that nearly every winner is inside and the window pass really runs.
--predict: whole captured predict() with dark on against off (flip test on, post_process off in both), W48 (384 x 288) and
PoseResNet-50 (256 x 192)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def taps(k):
    sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8
    i = torch.arange(k, dtype=torch.float64) - (k - 1) // 2
    g = torch.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


def head_case(Cc, h, w, k, n):
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator().manual_seed(Cc)
    wt = (0.2 * torch.randn((17, Cc), generator=g))
    f = 0.25 * torch.randn((2 * n, h, w, Cc), generator=g)
    cy = 8 + torch.rand((2 * n, 17), generator=g) * (h - 17); cx = 8 + torch.rand((2 * n, 17), generator=g) * (w - 17)
    yy, xx = torch.arange(h).float()[:, None], torch.arange(w).float()[None, :]
    for i in range(2 * n):
        for j in range(17):
            f[i] += 3.0 * torch.exp(-((yy - cy[i, j]) ** 2 + (xx - cx[i, j]) ** 2) / 8.0)[:, :, None] * torch.sign(wt[j])
    f = f.permute(0, 3, 1, 2).to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wt = wt.to(dev); b = (torch.randn(17, generator=g) + (60.0 if Cc == 256 else 30.0)).to(dev)
    view_of = torch.zeros(n, dtype=torch.int32, device=dev); slot_of = torch.arange(n, dtype=torch.int32, device=dev)
    boxes = torch.tensor([[10.0, 20.0, 100.0, 200.0]] * n, dtype=torch.float32, device=dev)
    det = torch.zeros((1, n, 17, 3), dtype=torch.float64, device=dev)
    scratch = torch.empty((int(lib.pam_head_decode_dark_scratch_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    hm = torch.empty((n, h, w, 17), dtype=torch.float32, device=dev)
    P = h * w
    gk = taps(k).to(dev)
    R = (k - 1) // 2

    def dark(flags):
        assert lib.pam_head_decode_dark(st(), n, n, h, w, p(f), Cc, p(wt), p(b), 17, flags, k, None, p(view_of), p(slot_of), p(boxes), n, p(det), None, p(scratch)) == 0

    def quarter(flags):
        assert lib.pam_head_decode_flip(st(), n, n, h, w, p(f), Cc, p(wt), p(b), 17, flags, None, p(view_of), p(slot_of), p(boxes), n, p(det), None, p(scratch)) == 0

    def composed():
        """The plain form (flags 0) without the fused kernel: maps to memory, blur of the whole map, log, and 13 gathers to the host."""
        assert lib.pam_head_heatmaps(st(), n * P, p(f), Cc, p(wt), p(b), 17, p(hm)) == 0
        m = hm.permute(0, 3, 1, 2).double().reshape(n * 17, 1, h, w)
        idx = m.reshape(n * 17, -1).argmax(1)
        mp = torch.nn.functional.pad(m, (R, R, 0, 0))
        bl = sum(gk[t] * mp[..., :, t:t + w] for t in range(k))
        mp = torch.nn.functional.pad(bl, (0, 0, R, R))
        bl = sum(gk[t] * mp[..., t:t + h, :] for t in range(k))
        L = torch.log(torch.clamp(bl, min=1e-10)).reshape(n * 17, h, w).cpu().numpy()
        idx = idx.cpu().numpy()
        out = np.zeros((n * 17, 2))
        for q in range(n * 17):
            py, px = divmod(int(idx[q]), w)
            out[q] = (py, px)
            if 1 < px < w - 2 and 1 < py < h - 2:
                l = L[q]
                dx = 0.5 * (l[py, px + 1] - l[py, px - 1]); dy = 0.5 * (l[py + 1, px] - l[py - 1, px])
                dxx = 0.25 * (l[py, px + 2] - 2 * l[py, px] + l[py, px - 2]); dyy = 0.25 * (l[py + 2, px] - 2 * l[py, px] + l[py - 2, px])
                dxy = 0.25 * (l[py + 1, px + 1] - l[py - 1, px + 1] - l[py + 1, px - 1] + l[py - 1, px - 1])
                dt = dxx * dyy - dxy * dxy
                if dt != 0:
                    out[q] += (-(dxx * dy - dxy * dx) / dt, -(dyy * dx - dxy * dy) / dt)
        return out
    dark(0); torch.cuda.synchronize()
    got = det[0, :, :, :2].cpu().numpy().reshape(n * 17, 2)
    want = composed()
    bx = boxes[0].cpu().numpy().astype(np.float64)
    want = np.stack([want[:, 0] / h * bx[3] + bx[1], want[:, 1] / w * bx[2] + bx[0]], 1)
    worst = float(np.abs(got - want).max())                            # frame pixels; the composed path blurs the float32 map in float64 as well
    forms = {'dark_0': lambda: dark(0), 'dark_3': lambda: dark(3), 'quarter_4': lambda: quarter(4), 'quarter_7': lambda: quarter(7)}
    graphs = {name: graph_of(fn, args.iters) for name, fn in forms.items()}
    t = {name: [] for name in list(forms) + ['composed_0']}
    for _ in range(args.rounds):
        for name in forms:
            t[name].append(us(graphs[name], args.iters))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            composed()
        t['composed_0'].append((time.perf_counter() - t0) / 3 * 1e6)
    m = {name: median(v) for name, v in t.items()}
    print(json.dumps(dict(bench='head', C=Cc, map=[h, w], k=k, boxes=n, us={a: round(v, 2) for a, v in m.items()},
                          dark_over_quarter_plain=round(m['dark_0'] / m['quarter_4'], 3), dark_over_quarter_merged=round(m['dark_3'] / m['quarter_7'], 3),
                          dark_over_composed=round(m['dark_0'] / m['composed_0'], 4), composed_max_abs_diff_px=worst)), flush=True)


def predict_case(name, kw, res, n):
    nets = {dark: hrnet.HRNetPose(*kw['args'], resolution=res, max_dets=8, max_crops=2 * n, flip_test=True, dark=dark,
                                  **{a: v for a, v in kw.items() if a != 'args'}) for dark in (False, True)}
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (776, 1032, 3), dtype=np.uint8)).to(dev) for _ in range(5)]
    pbl = [[dict(bbox=[40.0 + 60 * s, 50.0 + 30 * v, 180.0, 420.0], data=frames[v]) for s in range(n // 5)] for v in range(5)]
    t = {False: [], True: []}

    def run(net, iters):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(iters):
            net.predict(pbl, batch_size=n)
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    for dark in nets:
        run(nets[dark], 3)
    for _ in range(args.rounds):
        for dark in nets:
            t[dark].append(run(nets[dark], args.iters))
    off, on = median(t[False]), median(t[True])
    print(json.dumps(dict(bench='predict', net=name, boxes=n, flip_test=True, ms_off=round(off, 3), ms_on=round(on, 3),
                          on_over_off=round(on / off, 3))), flush=True)


head_case(48, 96, 72, 17, args.boxes)
head_case(256, 64, 48, 11, args.boxes)
if args.predict:
    predict_case('hrnet_w48_384x288', dict(args=(48, 17, None)), (384, 288), args.boxes)
    predict_case('pose_resnet50_256x192', dict(args=(50, 17, None), model_name='PoseResNet'), (256, 192), args.boxes)
