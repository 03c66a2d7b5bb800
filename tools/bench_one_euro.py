#!/usr/bin/env python3
"""What the One-Euro filter behind the frame step costs.  One process, every form warmed, forms interleaved, medians over
rounds.

(i)  microseconds per launch of pam_one_euro (device events round `--calls` back-to-back launches) on a 5-view rig with 16 persons in a
     handle of 16 track slots, and with 32 persons in a handle of 64 slots (the kernel's store loop runs over the handle's capacity):
     `repeat` = the launch on a frame it has consumed already (every row read and written, no arithmetic -- the calls are idempotent,
     so they can be issued back to back), `step` = frames of the sequence with the launch behind each frame step minus the same frames
     without it (every live track consumes a sample).
(ii) frames/s of the S2 FramePipeline over `--frames` frames (seeded keypoints through write_local, as bench.py): off (today's step),
     on (one_euro=True: the launch behind k_frame and its two buffers in front of the record's fetch), off again (the spread).
     Condition: off issues the launches it issued before the option existed.

usage: bench_one_euro.py [--frames 200] [--rounds 7] [--calls 200] [--out FILE.json] [--no-pipeline]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def per_launch(torch, synth, persons, max_tracks, calls, rounds, n_frames=40):
    from pam import _lib
    from oracle import cpu_ref as O
    name = 'B5_%d' % persons
    synth.SIZES[name] = dict(C=5, P=persons, w=1920, h=1080, f=1000.0)
    synth.SIZE_TO_DATASET[name] = 'Panoptic'
    seq = synth.make_sequence(name, n_frames=n_frames, seed=3)
    cfg = dict(synth.MATCHER_CFG['Panoptic']); conf = cfg.pop('CONF_THRESHOLD')
    cams = O.make_cameras(seq['calib'])
    md = max(8, persons)
    h = _lib.Handle(5, _lib.make_params(cfg, conf), max_dets=md, max_tracks=max_tracks, n_scenes=1)
    h.set_cameras(np.stack([c.P for c in cams]), np.stack([c.F for c in cams]), np.stack([c.RK_INV for c in cams]),
                  np.stack([c.position for c in cams]))
    h.set_one_euro(True)
    nd, dd = synth.pack_frames(seq['frames'], md)
    dev = torch.device('cuda:0')
    nd_t = [torch.tensor(nd[t], dtype=torch.int32, device=dev) for t in range(n_frames)]
    dd_t = [torch.tensor(dd[t], dtype=torch.float64, device=dev) for t in range(n_frames)]
    pose, meta = h.one_euro_buffers()
    st = torch.cuda.current_stream(dev).cuda_stream

    def frames(with_filter):
        h.reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(n_frames):
            h.frame_dev(st, t, nd_t[t].data_ptr(), dd_t[t].data_ptr())
            if with_filter:
                h.one_euro(st, t, pose, meta)
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n_frames

    def repeat(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            h.one_euro(st, n_frames - 1, pose, meta)
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    frames(True); frames(False); repeat(20)
    on, off, rep = [], [], []
    for _ in range(rounds):
        off.append(frames(False)); on.append(frames(True)); rep.append(repeat(calls))
    n_tracks = int(meta.cpu()[0, 0])
    h.close()
    return dict(views=5, persons=persons, max_tracks=max_tracks, n_tracks=n_tracks, us_repeat=float(np.median(rep)),
                us_step=float(np.median(on) - np.median(off)), us_frame_off=float(np.median(off)), us_frame_on=float(np.median(on)),
                repeat_rounds=[round(x, 2) for x in rep], frame_on_rounds=[round(x, 2) for x in on], frame_off_rounds=[round(x, 2) for x in off])


def pipeline_rate(torch, synth, bench, frames, rounds, warm=10):
    from pam.pipeline import FramePipeline
    nF = frames + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    meta = wl['meta']
    fh, fw, md = meta['h'], meta['w'], 8
    off = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True)
    on = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True, net=off.net, one_euro=True)
    dev = off.device
    inp = bench.build_inputs(torch, synth, wl['seq'], 'S2', md, 1, 0, 'views', dev, nF)
    pf = inp['per_frame']
    fr = torch.stack(inp['frames']).contiguous()
    ptrs = torch.tensor([fr[v].data_ptr() for v in range(fr.shape[0])], dtype=torch.int64, device=dev)

    def step(pipe, t):
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
    forms = [('off', off), ('on', on), ('off_again', off)]

    def run(pipe):
        pipe.reset()
        for t in range(warm):
            step(pipe, t)
        pipe.results(strict=False)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(warm, nF):
            step(pipe, t)
        rec = pipe.results(strict=False)
        b.record(); torch.cuda.synchronize()
        return frames / (a.elapsed_time(b) * 1e-3), rec
    for _, pipe in forms:                               # every form once, unrecorded: captures, first launches
        run(pipe)
    fps, ids = {name: [] for name, _ in forms}, {}
    for _ in range(rounds):
        for name, pipe in forms:
            f, rec = run(pipe)
            fps[name].append(f)
            ids[name] = [t['track_id'] for t in rec['tracks'] if t['emitted']]
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
    ap.add_argument('--no-pipeline', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_one_euro.py needs a GPU: nothing is measured without one')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_oe', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    import pam  # noqa: F401
    from pam import synth
    res = {'per_launch': {'5x16': per_launch(torch, synth, 16, 16, args.calls, args.rounds),
                          '5x64': per_launch(torch, synth, 32, 64, args.calls, args.rounds)}}
    if not args.no_pipeline:
        res['pipeline_S2'] = pipeline_rate(torch, synth, bench, args.frames, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
