#!/usr/bin/env python3
"""GPU timing of the person detector (resize -> Darknet-53, YOLOv3-tiny, YOLOv3-SPP, YOLOv4 or YOLOv4-tiny -> decode + NMS) on n views (development tool;
the v3 networks through yolov3.YOLOv3, the two v4 names through yolov4.YOLOv4).
--arch takes a comma-separated list: every network is built and timed in the same process, one line each."""
import os, sys, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import pam
from pam import yolov3, yolov4

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=5); ap.add_argument('--h', type=int, default=776); ap.add_argument('--w', type=int, default=1032)
ap.add_argument('--iters', type=int, default=20); ap.add_argument('--no-graph', action='store_true')
ap.add_argument('--arch', default='yolov3',
                help="comma-separated: %s (used when --cfg is not given)" % ', '.join(sorted(yolov4.ARCHS4)))
ap.add_argument('--cfg', default=None); ap.add_argument('--weights', default=None)
args = ap.parse_args()
frames = torch.randint(0, 256, (args.n, args.h, args.w, 3), dtype=torch.uint8, device='cuda:0')
for arch in args.arch.split(','):
    if args.cfg is None and arch not in yolov4.ARCHS4:
        ap.error('--arch %s: expected one of %s' % (arch, ', '.join(sorted(yolov4.ARCHS4))))
    cls = yolov3.YOLOv3 if arch in yolov3.ARCHS and args.cfg is None else yolov4.YOLOv4
    det = cls(args.cfg, args.weights, None, score_thresh=0.5, nms_thresh=0.4, use_graph=not args.no_graph, arch=arch)
    det.net.count = dict(bytes=0, flops=0, launches=0)
    det.use_graph, g = False, det.use_graph
    det.detect_dev(frames); torch.cuda.synchronize()
    work = dict(det.net.count); det.net.count = None
    det.use_graph = g; det._graphs.clear()
    buf = det.frame_buffer(args.n, args.h, args.w); buf.copy_(frames)
    det.detect_dev(buf); buf = det.frame_buffer(args.n, args.h, args.w); buf.copy_(frames)
    for _ in range(3): det.detect_dev(buf)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(args.iters): boxes, count = det.detect_dev(buf)
    b.record(); torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.iters
    print('%s views=%d %dx%d  %.3f ms/frame-set  %.1f TFLOP/s  %.2f TB/s algorithmic  launches=%d  boxes=%s' % (
        args.cfg or arch, args.n, args.w, args.h, ms, work['flops'] / ms / 1e9, work['bytes'] / ms / 1e9, work['launches'] + 2, count[:args.n].tolist()))
