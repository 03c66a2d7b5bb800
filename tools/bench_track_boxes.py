#!/usr/bin/env python3
"""What person boxes from the tracks cost and buy.  One process, every form warmed, forms interleaved, medians over rounds.

(i)  microseconds per call of pam_track_boxes + pam_crop_table (device events round `--calls` back-to-back pairs) on S2 (5 views, 4
     tracks) and S4 (31 views, 7 tracks), next to one replay of the YOLOv3 detector on the same views.
(ii) frames/s of the S2 FramePipeline over `--frames` frames (seeded keypoints through write_local, as bench.py), five forms:
     a   host tables (today's form)            a'  track boxes on every frame, no detector (what the wait for k_frame costs)
     b   detector on every frame, device table c   detect_every = 5                           b2  b again (the spread)
     Condition: c does strictly less GPU work than b, so c must not be slower than b by more than |b - b2|.

usage: bench_track_boxes.py [--frames 200] [--rounds 7] [--calls 200] [--out FILE.json] [--no-s4]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_call(torch, synth, bench, size, calls, rounds, with_detector=True):
    from pam import _lib
    from pam.pipeline import FramePipeline
    wl = bench.setup_workload(synth, size, 12)
    meta = wl['meta']
    C, fh, fw, md = meta['C'], meta['h'], meta['w'], 8
    pipe = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, hrnet=False)
    dev = pipe.device
    n_det, det = synth.pack_frames(wl['seq']['frames'], md)
    for t in range(12):
        pipe.track_step(t, torch.tensor(n_det[t], dtype=torch.int32, device=dev), torch.tensor(det[t], dtype=torch.float64, device=dev))
    rec = pipe.results()
    pipe._box_buffers()
    T, st = pipe._tables[0], torch.cuda.current_stream(dev)

    def pair():
        b, c, _ = pipe.track_boxes(12)
        _lib.crop_table(st.cuda_stream, b, c, fw, fh, md, T['view_of'], T['slot_of'], T['xywh'], T['n_det'], T['info'])

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    res = dict(views=C, tracks=rec['n_tracks'], crop_rows=None)
    det_fn = None
    if with_detector:
        from pam.yolov3 import YOLOv3
        yolo = YOLOv3(None, None, None, score_thresh=0.7, nms_thresh=0.45, device=dev.index or 0, seed=0, max_det=md)
        frames = torch.randint(0, 256, (C, fh, fw, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1234)).to(dev)
        yolo.detect_dev(frames); torch.cuda.synchronize()
        buf = yolo.frame_buffer(C, fh, fw); buf.copy_(frames)
        det_fn = lambda: yolo.detect_dev(buf)
        timed(det_fn, 3)
    timed(pair, 20)
    us_pair, us_det = [], []
    for _ in range(rounds):
        us_pair.append(timed(pair, calls))
        if det_fn is not None:
            us_det.append(timed(det_fn, 10))
    res['crop_rows'] = int(T['info'].cpu()[0])
    res['us_track_boxes_plus_crop_table'] = float(np.median(us_pair))
    res['us_pair_rounds'] = [round(x, 2) for x in us_pair]
    if us_det:
        res['us_detector_replay'] = float(np.median(us_det))
        res['us_detector_rounds'] = [round(x, 1) for x in us_det]
    return res


def pipeline_rate(torch, synth, bench, frames, rounds, warm=10, cap=20):
    from pam.pipeline import FramePipeline
    from pam.yolov3 import YOLOv3
    nF = frames + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    meta = wl['meta']
    C, fh, fw, md = meta['C'], meta['h'], meta['w'], 8
    # crop_cap = the workload's crops per frame (5 views x 4 persons): every form's forward then has the 20 rows of form a
    pipe = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True, crop_cap=cap)
    dev = pipe.device
    inp = bench.build_inputs(torch, synth, wl['seq'], 'S2', md, 1, 0, 'views', dev, nF)
    pf = inp['per_frame']
    yolo = YOLOv3(None, None, None, score_thresh=0.7, nms_thresh=0.45, device=dev.index or 0, seed=0, max_det=md)
    fr = torch.stack(inp['frames']).contiguous()
    yolo.detect_dev(fr); torch.cuda.synchronize()
    buf = yolo.frame_buffer(C, fh, fw); buf.copy_(fr)
    ptrs = torch.tensor([buf[v].data_ptr() for v in range(C)], dtype=torch.int64, device=dev)
    pipe.attach_detector(yolo, frames=buf, n_crops=cap)
    pipe._box_buffers()

    def step_a(t):
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])

    def step_tracks(t):
        e = pf[t]
        with pipe.frame():
            b, c, _ = pipe.track_boxes(t)
            pipe.pose_step_boxes(ptrs, b, c, views=pipe._mine_dev)
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])

    def step_auto(t):
        e = pf[t]
        with pipe.frame():
            pipe.pose_step_auto(t, ptrs, buf, next_frames=buf)
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
    forms = [('a_host_tables', step_a, 1), ('a1_track_boxes_every_frame', step_tracks, 1), ('b_detector_every_frame', step_auto, 1),
             ('c_detect_every_5', step_auto, 5), ('b2_detector_every_frame_again', step_auto, 1)]

    def run(step, every):
        pipe.reset(); pipe.detect_every = every
        for t in range(warm):
            step(t)
        pipe.results(strict=False)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(warm, nF):
            step(t)
        rec = pipe.results(strict=False)                # waits for the pose, tracker and detector work of the last frame
        b.record(); torch.cuda.synchronize()
        return frames / (a.elapsed_time(b) * 1e-3), rec
    fps = {name: [] for name, _, _ in forms}
    tracks = {}
    for name, step, every in forms:                     # every form once, unrecorded: captures, first launches
        run(step, every)
    for _ in range(rounds):
        for name, step, every in forms:
            f, rec = run(step, every)
            fps[name].append(f)
            tracks[name] = ([t['track_id'] for t in rec['tracks'] if t['emitted']], rec.get('crop_table'))
    out = {name: dict(frames_per_s=float(np.median(v)), rounds=[round(x, 1) for x in v], final_ids=tracks[name][0], crop_table=tracks[name][1])
           for name, v in fps.items()}
    b, b2, c = (out[k]['frames_per_s'] for k in ('b_detector_every_frame', 'b2_detector_every_frame_again', 'c_detect_every_5'))
    out['condition'] = dict(spread_b=abs(b - b2), c_minus_slower_b=c - min(b, b2), holds=bool(c >= min(b, b2) - abs(b - b2)))
    out['frames'], out['crop_cap'], out['det_overlaps'] = frames, cap, bool(pipe.det_overlaps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-s4', action='store_true')
    ap.add_argument('--no-pipeline', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_track_boxes.py needs a GPU: nothing is measured without one')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_tb', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    import pam  # noqa: F401
    from pam import synth
    res = {'per_call': {'S2': per_call(torch, synth, bench, 'S2', args.calls, args.rounds)}}
    if not args.no_s4:
        res['per_call']['S4'] = per_call(torch, synth, bench, 'S4', args.calls, args.rounds)
    if not args.no_pipeline:
        res['pipeline_S2'] = pipeline_rate(torch, synth, bench, args.frames, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
