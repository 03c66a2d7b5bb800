#!/usr/bin/env python3
"""HRNet-W32 (256 x 192) vs HRNet-W48 (384 x 288) in ONE process, interleaved: the captured (hipGraph) feature forward of W32 with the
fused 32-channel blocks (k_bblock2_32), of W48, and of W32 with the 32-channel blocks as two k_conv3x3<32> launches, per crop count,
repeated rounds; ms per forward and W32's share of the bf16 MFMA peak.  --facade also times the ivclabpose facade built from
configs/Shelf/model_configs_w32.yaml on Shelf-like synthetic frames (pose + tracker per frame).  One JSON line per result."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pam  # noqa: E402,F401
from pam import hrnet  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA peak (public spec, 2.5 PFLOP/s)

ap = argparse.ArgumentParser()
ap.add_argument('--crops', default='1,5,20,60')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--only-w32', action='store_true', help='W32 forwards only (for a kernel trace)')
ap.add_argument('--facade', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def variants():
    w32 = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_crops=64)
    v = [('w32_fused', w32, 'w32_fused')]
    if not args.only_w32:
        w32u = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_crops=64)
        w32u.config_for = lambda n: 'w32_unfused'
        w48 = hrnet.HRNetPose(48, 17, None, resolution=(384, 288), use_graph=True, max_crops=64)
        v += [('w48', w48, None), ('w32_unfused', w32u, 'w32_unfused')]
    return v


crops = [int(q) for q in args.crops.split(',')]
vs = variants()
flops = {32: hrnet.count_flops(32, 17, 256, 192), 48: hrnet.count_flops(48, 17, 384, 288)}
inputs = {}
for name, net, _ in vs:
    for n in crops:
        x = net.input_buffer(n)
        x.copy_(torch.randn(x.shape, generator=torch.Generator().manual_seed(n)).to(x.dtype).to(dev))
        inputs[(name, n)] = x
        net.features(x)                                           # capture
        torch.cuda.synchronize()
res = {}
for r in range(args.rounds):
    for n in crops:
        for name, net, _ in vs:
            x = inputs[(name, n)]
            net.features(x)
            res.setdefault((name, n), []).append(timed(lambda: net.features(x), args.iters))
for n in crops:
    for name, net, _ in vs:
        ms = sorted(res[(name, n)])
        med = ms[len(ms) // 2]
        w = net.width
        print(json.dumps(dict(variant=name, width=w, crops=n, ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_all=[round(q, 4) for q in ms],
                              config=net.hip.config_name, tflops=round(flops[w] * n / med / 1e9, 1),
                              mfma_peak_share=round(flops[w] * n / med / 1e9 / PEAK_BF16_TFLOPS, 4))), flush=True)

if args.facade:
    from pam import synth
    from pam.dataset import GetConfig
    from pam.ivclabpose import ivclabpose
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_w32.yaml'))
    pose = dict(cfg.POSE_MODELS.HRPOSE, CHECKPOINT_FILE='')
    seq = synth.make_sequence('S2', n_frames=60, seed=7)
    mcfg = dict(synth.MATCHER_CFG['Shelf']); conf = mcfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, pose, dict(mcfg, NAME='Iterative'), conf)
    meta = synth.SIZES['S2']
    model.GetCameraParameters(seq['calib'], meta['w'], meta['h'])
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (meta['h'], meta['w'], 3), dtype=np.uint8)).to(dev) for _ in range(meta['C'])]
    t0, n_crops = None, 0
    for t, views in enumerate(seq['frames']):
        if t == 10:
            torch.cuda.synchronize(); t0 = time.perf_counter(); n_crops = 0
        pbl, _ = synth.to_dump_results(views)
        for v, persons in enumerate(pbl):
            for p in persons:
                p['data'] = frames[v]
        n_crops += sum(len(p) for p in pbl)
        dump = model.PersonPoseDetect(imagelist=None, person_bbox_list=pbl, batch_size=20)
        model.PersonTrack_Project3DPose(t, pbl, dump, 'SVD')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nf = len(seq['frames']) - 10
    print(json.dumps(dict(facade='w32', size='S2', cameras=meta['C'], frames=nf, crops_per_frame=round(n_crops / nf, 2),
                          fps=round(nf / dt, 2), ms_per_frame=round(1e3 * dt / nf, 3))), flush=True)
