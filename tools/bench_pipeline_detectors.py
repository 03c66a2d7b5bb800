#!/usr/bin/env python3
"""The S2 FramePipeline rate with each person detector attached in turn, in one process (development tool): bench.py's own workload,
pipeline, inputs and full-pipeline run (images -> detector -> crops -> HRNet-W48 -> tracker, frames resident in HBM; serial = the
reference's order, overlapped = frame t + 1's detection under frame t's conv stack, FramePipeline.attach_detector).  bench.py builds
that run round `pam.yolov3.YOLOv3` with Darknet-53; here its `full_pipeline_runs` is called once per network and round with that name
bound to a constructor of the wanted detector (yolov3.YOLOv3 for the v3 names, yolov4.YOLOv4 for 'yolov4' / 'yolov4-tiny').  Random
weights, seeded boxes, as in bench.py.  One line per network and round, the boxes-given rate of the same pipeline first."""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist
import pam  # noqa: F401
from pam import synth, yolov3, yolov4
from pam.pipeline import FramePipeline

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=100); ap.add_argument('--warmup', type=int, default=10); ap.add_argument('--rounds', type=int, default=2)
ap.add_argument('--arch', default='yolov3,yolov3-tiny,yolov4,yolov4-tiny', help='comma-separated: %s' % ', '.join(sorted(yolov4.ARCHS4)))
args = ap.parse_args()
spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
bargs = b.parse_args(['--gpus', '1', '--steps', str(args.steps), '--warmup', str(args.warmup)])

dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
K, W = args.steps, args.warmup
wl = b.setup_workload(synth, 'S2', K + W)
meta = wl['meta']
C, fw, fh = meta['C'], meta['w'], meta['h']
pipe = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=8, max_tracks=16, device=0, world=1, rank=0, use_graph=True,
                     shard='crops', overlap_tracker=True, exchange='torch', pose_streams=bargs.pose_streams, autotune=True)
inp = b.build_inputs(torch, synth, wl['seq'], 'S2', 8, 1, 0, 'crops', dev, K + W)
torch.cuda.synchronize()
elapsed, _, final = b.timed_run(torch, dist, pipe, b.make_step(pipe, inp, 'crops'), inp, K, W, 1, dev)
ref = [t['track_id'] for t in final['tracks'] if t['emitted']]
print('boxes given (no detector): %.1f frames/s' % (K / elapsed))

plain = yolov3.YOLOv3
for r in range(args.rounds):
    for arch in args.arch.split(','):
        cls = plain if arch in yolov3.ARCHS else yolov4.YOLOv4
        yolov3.YOLOv3 = lambda *a, _cls=cls, _arch=arch, **k: _cls(*a, arch=_arch, **k)      # what full_pipeline_runs imports and constructs
        try:
            pipe.handle.reset()
            full = b.full_pipeline_runs(torch, dist, pipe, inp, K, W, C, fh, fw, dev, ref)
        finally:
            yolov3.YOLOv3 = plain
        print('round %d %-11s detector alone %.3f ms  serial %.1f frames/s  overlapped %.1f frames/s  two frames per detection %.1f frames/s  tracks equal %s' % (
            r, arch, full['detector']['ms'], full['serial']['value'], full['overlapped']['value'], full['overlapped_two_frames_per_detection']['value'],
            full['serial']['final_tracks_equal'] and full['overlapped']['final_tracks_equal']))
