#!/usr/bin/env python3
"""What the pose checkpoints' box transform costs in the crop launch and in a frame.  One process, every form warmed,
forms interleaved, medians over rounds.

(i)  microseconds per crop launch (device events round `--calls` back-to-back launches) of the stretch form (pam_preprocess_crops_ex)
     and of the affine form (pam_preprocess_crops_affine) on the SAME raw boxes, 384 x 288 x 8-channel output: 20 crops from 1032 x 776
     frames (S2's rig), plain bilinear, and 35 crops from 1920 x 1080 frames with antialias (HD boxes, down-scaled).  The affine form
     samples an area 1.25^2 x the aspect-fixed box: with the same 2 x 2 reads per output pixel, but other addresses.
(ii) frames/s of the S2 FramePipeline over `--frames` frames (seeded keypoints through write_local, as bench.py): off (box_transform=
     'stretch': today's step), on ('affine' on the same network), off again (the spread).

usage: bench_affine_crop.py [--frames 200] [--rounds 7] [--calls 200] [--out FILE.json] [--no-hd] [--no-pipeline]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (384, 288)


def person_boxes(n, views, fh, fw, tall, seed):
    """n person-like boxes (taller than wide, h around `tall` pixels), some hanging over a frame edge, dealt out over the views."""
    rng = np.random.default_rng([seed, n, fh, fw])
    h = rng.uniform(0.6, 1.4, n) * tall
    w = h * rng.uniform(0.3, 0.6, n)
    x = rng.uniform(-0.2, 1.0, n) * (fw - w)
    y = rng.uniform(-0.1, 1.0, n) * (fh - h)
    return np.stack([x, y, w, h], 1).astype(np.float32), (np.arange(n) % views).astype(np.int32)


def per_launch(torch, n, views, fh, fw, tall, antialias, calls, rounds):
    from pam import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream(dev)
    rng = np.random.default_rng([3, fh, fw])
    frames = torch.from_numpy(rng.integers(0, 256, (views, fh, fw, 3), dtype=np.uint8)).to(dev)
    ptrs = torch.tensor([frames[v].data_ptr() for v in range(views)], dtype=torch.int64, device=dev)
    boxes, view_of = person_boxes(n, views, fh, fw, tall, 5)
    b_dev, v_dev = torch.from_numpy(boxes).to(dev), torch.from_numpy(view_of).to(dev)
    H, W = RES
    out = torch.empty((n, H, W, 8), dtype=torch.bfloat16, device=dev)
    eff = torch.empty((n, 4), dtype=torch.float32, device=dev)

    def stretch():
        return lib.pam_preprocess_crops_ex(C.c_void_p(st.cuda_stream), n, n, C.c_void_p(ptrs.data_ptr()), fh, fw, C.c_void_p(v_dev.data_ptr()),
                                           C.c_void_p(b_dev.data_ptr()), H, W, 8, C.c_void_p(out.data_ptr()), antialias)

    def affine():
        return lib.pam_preprocess_crops_affine(C.c_void_p(st.cuda_stream), n, n, 0, C.c_void_p(ptrs.data_ptr()), fh, fw,
                                               C.c_void_p(v_dev.data_ptr()), C.c_void_p(b_dev.data_ptr()), _lib.BOX_SCALE, H, W, 8,
                                               C.c_void_p(out.data_ptr()), antialias, C.c_void_p(eff.data_ptr()))
    forms = [('stretch', stretch), ('affine', affine), ('stretch_again', stretch)]

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            if fn() != 0:
                raise RuntimeError('the crop launch failed')
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / k
    for _, fn in forms:
        timed(fn, 20)
    us = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, fn in forms:
            us[name].append(timed(fn, calls))
    e = eff.cpu().numpy()
    res = {name: dict(us_per_launch=float(np.median(v)), rounds=[round(x, 2) for x in v]) for name, v in us.items()}
    res.update(crops=n, frame=[fh, fw], antialias=int(antialias), output=list(RES) + [8],
               mean_scale_stretch=[float(np.mean(boxes[:, 2] / W)), float(np.mean(boxes[:, 3] / H))],
               mean_scale_affine=float(np.mean(e[:, 2] / W)),
               affine_over_stretch=float(np.median(us['affine']) / np.median(us['stretch'])),
               spread_stretch=abs(float(np.median(us['stretch']) - np.median(us['stretch_again']))))
    return res


def pipeline_rate(torch, synth, bench, frames, rounds, warm=10):
    from pam.pipeline import FramePipeline
    nF = frames + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    meta = wl['meta']
    fh, fw, md = meta['h'], meta['w'], 8
    pipe = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True)
    dev = pipe.device
    inp = bench.build_inputs(torch, synth, wl['seq'], 'S2', md, 1, 0, 'views', dev, nF)
    pf = inp['per_frame']
    fr = torch.stack(inp['frames']).contiguous()
    ptrs = torch.tensor([fr[v].data_ptr() for v in range(fr.shape[0])], dtype=torch.int64, device=dev)

    def step(t):
        # the tracker gets the seeded keypoints in either form (the network's weights are random), so both forms track the same people:
        # the difference is the crop launch and the table the decode reads
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
    forms = [('off', 'stretch'), ('on', 'affine'), ('off_again', 'stretch')]

    def run(mode):
        pipe.results(strict=False)                      # nothing in flight reads the network's setting while it changes
        pipe.net.box_transform = mode
        pipe.reset()
        for t in range(warm):
            step(t)
        pipe.results(strict=False)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(warm, nF):
            step(t)
        rec = pipe.results(strict=False)
        b.record(); torch.cuda.synchronize()
        return frames / (a.elapsed_time(b) * 1e-3), rec
    step(0); pipe.results(strict=False)
    for _, mode in forms:                               # every form once, unrecorded: captures, first launches
        run(mode)
    fps, ids = {name: [] for name, _ in forms}, {}
    for _ in range(rounds):
        for name, mode in forms:
            f, rec = run(mode)
            fps[name].append(f)
            ids[name] = [t['track_id'] for t in rec['tracks'] if t['emitted']]
    pipe.net.box_transform = 'stretch'
    out = {name: dict(frames_per_s=float(np.median(v)), rounds=[round(x, 1) for x in v], final_ids=ids[name]) for name, v in fps.items()}
    out['spread_off'] = abs(out['off']['frames_per_s'] - out['off_again']['frames_per_s'])
    out['frames'] = frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-hd', action='store_true')
    ap.add_argument('--no-pipeline', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_affine_crop.py needs a GPU: nothing is measured without one')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_ac', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    import pam  # noqa: F401
    from pam import synth
    res = {'per_launch': {'20_of_776x1032': per_launch(torch, 20, 5, 776, 1032, 300.0, 0, args.calls, args.rounds)}}
    if not args.no_hd:
        res['per_launch']['35_of_1080x1920_antialias'] = per_launch(torch, 35, 5, 1080, 1920, 650.0, 1, args.calls, args.rounds)
    if not args.no_pipeline:
        res['pipeline_S2'] = pipeline_rate(torch, synth, bench, args.frames, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
