#!/usr/bin/env python3
"""PoseResNet-50 / 101 / 152 (256 x 192), PoseResNet-50 (384 x 288) and, for reference, HRNet-W32 (256 x 192) and HRNet-W48 (384 x 288) in
ONE process, interleaved over rounds: the captured (hipGraph) feature forward per crop count, median ms, and each model's share of the
bf16 MFMA peak from counted FLOPs.  --facade also times the ivclabpose facade built from configs/Shelf/model_configs_poseresnet50.yaml on
Shelf-like synthetic frames (pose + tracker per frame).  --models R50 -> that model alone (for a kernel trace).  One JSON line per result."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import pam  # noqa: E402,F401
from pam import hrnet, poseresnet  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16 MFMA peak (public spec, 2.5 PFLOP/s)
MODELS = {
    'R50': ('PoseResNet', 50, (256, 192)), 'R101': ('PoseResNet', 101, (256, 192)), 'R152': ('PoseResNet', 152, (256, 192)),
    'R50@384': ('PoseResNet', 50, (384, 288)), 'W32': ('HRNet', 32, (256, 192)), 'W48': ('HRNet', 48, (384, 288)),
}

ap = argparse.ArgumentParser()
ap.add_argument('--crops', default='1,5,20,60')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--models', default=','.join(MODELS))
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


def flops_of(family, c, res):
    return poseresnet.count_flops(c, res) if family == 'PoseResNet' else hrnet.count_flops(c, 17, res[0], res[1])


crops = [int(q) for q in args.crops.split(',')]
names = [q for q in args.models.split(',') if q]
nets, flops, inputs = {}, {}, {}
for name in names:
    family, c, res = MODELS[name]
    nets[name] = hrnet.HRNetPose(c, 17, None, model_name=family, resolution=res, use_graph=True, max_crops=max(crops))
    flops[name] = flops_of(family, c, res)
    for n in crops:
        x = nets[name].input_buffer(n)
        x.zero_()
        x[:, :3].copy_(torch.randn((n, 3) + res, generator=torch.Generator().manual_seed(n)).to(x.dtype).to(dev))
        inputs[(name, n)] = x
        nets[name].features(x)                                  # capture
        torch.cuda.synchronize()
res_ms = {}
for r in range(args.rounds):
    for n in crops:
        for name in names:
            x, net = inputs[(name, n)], nets[name]
            net.features(x)
            res_ms.setdefault((name, n), []).append(timed(lambda: net.features(x), args.iters))
for n in crops:
    for name in names:
        ms = sorted(res_ms[(name, n)])
        med = ms[len(ms) // 2]
        tf = flops[name] * n / med / 1e9
        print(json.dumps(dict(model=name, crops=n, ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_all=[round(q, 4) for q in ms],
                              gflop_per_crop=round(flops[name] / 1e9, 3), config=nets[name].hip.config_name, tflops=round(tf, 1),
                              mfma_peak_share=round(tf / PEAK_BF16_TFLOPS, 4))), flush=True)

if args.facade:
    from pam import synth
    from pam.dataset import GetConfig
    from pam.ivclabpose import ivclabpose
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_poseresnet50.yaml'))
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
    print(json.dumps(dict(facade='poseresnet50', size='S2', cameras=meta['C'], frames=nf, crops_per_frame=round(n_crops / nf, 2),
                          fps=round(nf / dt, 2), ms_per_frame=round(1e3 * dt / nf, 3))), flush=True)
