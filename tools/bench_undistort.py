#!/usr/bin/env python3
"""What the lens step behind the decode costs.  One process, every form warmed, forms interleaved, medians over rounds.

(i)  microseconds per call of pam_undistort_keypoints (device events round `--calls` back-to-back calls; a call is the 8-byte memset of
     its two info words and the kernel) at 5 views x 8 slots (S2's rig, 20 real rows) and at 31 views x 16 slots (S4's rig, 217 rows), on
     the sequence's poses pushed through the HD-like lens (k1 -0.286, k2 0.195, p1 -0.0004, p2 0.0006, k3 0.018) on the rig's K.
(ii) frames/s of the S2 FramePipeline over `--frames` frames (seeded keypoints through write_local, as bench.py): off (today's step), on
     (the same step with lens=: the launch behind the decode), off again (the spread).  Condition: off issues the launches it issued
     before the option existed.

usage: bench_undistort.py [--frames 200] [--rounds 7] [--calls 200] [--out FILE.json] [--no-s4] [--no-pipeline]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD_LIKE = (-0.286, 0.195, -0.0004, 0.0006, 0.018)


def rig_lens(_lib, calib):
    K = np.asarray(calib['K']).astype(np.float32).astype(np.float64)
    return _lib.lens_table(K, np.tile(np.asarray(HD_LIKE), (len(K), 1)))


def per_launch(torch, synth, size, md, calls, rounds):
    from pam import _lib, lens
    seq = synth.make_sequence(size, n_frames=1, seed=3)
    views = seq['frames'][0]
    table = rig_lens(_lib, seq['calib'])
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream(dev)
    V = len(views)
    det = np.zeros((V, md, 17, 3))
    for v, d in enumerate(views):
        d = d[:md]
        det[v, :len(d)] = d[:, :, [1, 0, 2]]
        det[v, :len(d), :, 1], det[v, :len(d), :, 0] = lens.distort_uw(table[v], d[:, :, 0], d[:, :, 1])
    t_src = torch.from_numpy(det).to(dev)
    t_det = t_src.clone()
    n_in = torch.tensor([min(len(d), md) for d in views], dtype=torch.int32, device=dev)
    t_lens = torch.from_numpy(table).to(dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)

    def launch():
        _lib.undistort_keypoints(st.cuda_stream, t_det, n_in, t_lens, info)

    def timed(n):
        # (the call works in place: from the second call on it inverts points that are ideal already -- the same 8 steps on every lane,
        # there is no data-dependent exit)
        t_det.copy_(t_src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            launch()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n
    t_det.copy_(t_src); launch(); torch.cuda.synchronize()
    first = [int(x) for x in info.cpu()]
    moved = float((t_det - t_src).abs().max().cpu())
    timed(20)
    us = [timed(calls) for _ in range(rounds)]
    return dict(views=V, slots=md, rows=int(n_in.sum().cpu()), info_of_the_first_call=first, largest_move_px=round(moved, 2),
                us_per_call=float(np.median(us)), us_rounds=[round(x, 2) for x in us])


def pipeline_rate(torch, synth, bench, frames, rounds, warm=10):
    from pam import _lib
    from pam.pipeline import FramePipeline
    nF = frames + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    meta = wl['meta']
    fh, fw, md = meta['h'], meta['w'], 8
    off = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True)
    on = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True, net=off.net,
                       lens=rig_lens(_lib, wl['seq']['calib']))
    dev = off.device
    inp = bench.build_inputs(torch, synth, wl['seq'], 'S2', md, 1, 0, 'views', dev, nF)
    pf = inp['per_frame']
    fr = torch.stack(inp['frames']).contiguous()
    ptrs = torch.tensor([fr[v].data_ptr() for v in range(fr.shape[0])], dtype=torch.int64, device=dev)

    def step_off(pipe, t):
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])

    def step_on(pipe, t):
        # the launch runs on what the (random-weight) network decoded; the tracker then gets the seeded (ideal) keypoints of the off
        # form, so both forms track the same people: the difference is the launch
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'], n_det=e['nd'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
    forms = [('off', off, step_off), ('on', on, step_on), ('off_again', off, step_off)]

    def run(pipe, step):
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
    for name, pipe, step in forms:                      # every form once, unrecorded: captures, first launches
        run(pipe, step)
    fps, ids = {name: [] for name, _, _ in forms}, {}
    for _ in range(rounds):
        for name, pipe, step in forms:
            f, rec = run(pipe, step)
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
    ap.add_argument('--no-s4', action='store_true')
    ap.add_argument('--no-pipeline', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_undistort.py needs a GPU: nothing is measured without one')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_ln', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    import pam  # noqa: F401
    from pam import synth
    res = {'per_call': {'5x8': per_launch(torch, synth, 'S2', 8, args.calls, args.rounds)}}
    if not args.no_s4:
        res['per_call']['31x16'] = per_launch(torch, synth, 'S4', 16, args.calls, args.rounds)
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
