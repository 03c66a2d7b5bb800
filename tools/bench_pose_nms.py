#!/usr/bin/env python3
"""What the OKS-NMS behind the decode costs.  One process, every form warmed, forms interleaved, medians over rounds.

(i)  microseconds per launch of pam_pose_nms (device events round `--calls` back-to-back launches) on S2 (5 views x 8 slots, 20 real rows)
     and S4 (31 views x 16 slots, 217 rows), each once on the sequence's poses as they are (no duplicates) and once with every row
     doubled (copies 1 px to the right behind the real rows: every copy dies).
(ii) frames/s of the S2 FramePipeline over `--frames` frames (seeded keypoints through write_local, as bench.py): off (host tables,
     today's step), on (the same step with pose_nms=True: the launch behind the decode and the keep table in the record's fetch), off
     again (the spread).  Condition: off issues the launches it issued before the option existed, so it must read the rate of the tree
     before within the spread of two runs of that tree (`--off-only --root <that tree>` measures the same form there).

usage: bench_pose_nms.py [--frames 200] [--rounds 7] [--calls 200] [--out FILE.json] [--no-s4] [--no-pipeline] [--off-only] [--root DIR]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def per_launch(torch, synth, size, md, calls, rounds):
    from pam import _lib
    seq = synth.make_sequence(size, n_frames=1, seed=3)
    views = seq['frames'][0]
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream(dev)
    res = {}
    for form in ('no_duplicates', 'every_row_doubled'):
        rows = []
        for d in views:
            d = d[:md // 2 if form == 'every_row_doubled' else md]
            if form == 'every_row_doubled':
                c = d.copy(); c[:, :, 0] += 1.0; c[:, :, 2] *= 0.97
                d = np.concatenate([d, c])
            rows.append(d)
        V = len(rows)
        det = np.zeros((V, md, 17, 3))
        view_of, slot_of, xywh = [], [], []
        for v, d in enumerate(rows):
            det[v, :len(d)] = d[:, :, [1, 0, 2]]
            for s, it in enumerate(synth.to_dump_results([d])[0][0]):
                view_of.append(v); slot_of.append(s); xywh.append(it['bbox'])
        t_src = torch.from_numpy(det).to(dev)
        t_det = t_src.clone()
        n_in = torch.tensor([len(d) for d in rows], dtype=torch.int32, device=dev)
        tabs = (torch.tensor(view_of, dtype=torch.int32, device=dev), torch.tensor(slot_of, dtype=torch.int32, device=dev),
                torch.tensor(np.array(xywh, dtype=np.float32), device=dev))
        n_out = torch.zeros(V, dtype=torch.int32, device=dev)
        keep = torch.zeros((V, md), dtype=torch.int32, device=dev)
        score = torch.zeros((V, md), dtype=torch.float64, device=dev)

        def launch():
            _lib.pose_nms(st.cuda_stream, t_det, n_in, tabs[0], tabs[1], tabs[2], n_out, keep, score)

        def timed(n):
            # (the launch filters in place: from the second launch on the rows are the filtered ones and the tail is zero -- the
            # pairs, the exps and the stores are those of the first launch, since the counts are the ORIGINAL ones every time)
            t_det.copy_(t_src)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                launch()
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / n
        t_det.copy_(t_src); launch(); torch.cuda.synchronize()
        first = int(n_out.sum().cpu())
        timed(20)
        us = [timed(calls) for _ in range(rounds)]
        res[form] = dict(views=V, slots=md, rows=int(n_in.sum().cpu()), kept_by_the_first_launch=first, us_per_launch=float(np.median(us)),
                         us_rounds=[round(x, 2) for x in us])
    return res


def pipeline_rate(torch, synth, bench, frames, rounds, warm=10, off_only=False):
    from pam.pipeline import FramePipeline
    nF = frames + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    meta = wl['meta']
    fh, fw, md = meta['h'], meta['w'], 8
    off = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True)
    on = None if off_only else FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True,
                                             net=off.net, pose_nms=True)
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
        # the launch runs on what the (random-weight) network decoded; the tracker then gets the seeded keypoints and counts of the
        # off form, so both forms track the same people: the difference is the launch and the keep table's copy
        e = pf[t]
        with pipe.frame():
            pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'], n_det=e['nd'])
            pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
    forms = [('off', off, step_off)] + ([] if off_only else [('on', on, step_on)]) + [('off_again', off, step_off)]

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
    ap.add_argument('--off-only', action='store_true', help='the off form alone (twice): also runs on a tree without the option')
    ap.add_argument('--root', default=ROOT, help='the tree whose package and bench.py are measured')
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_pose_nms.py needs a GPU: nothing is measured without one')
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_pn', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    import pam  # noqa: F401
    from pam import synth
    res = {'root': root}
    if not args.off_only:
        res['per_launch'] = {'S2': per_launch(torch, synth, 'S2', 8, args.calls, args.rounds)}
        if not args.no_s4:
            res['per_launch']['S4'] = per_launch(torch, synth, 'S4', 16, args.calls, args.rounds)
    if not args.no_pipeline:
        res['pipeline_S2'] = pipeline_rate(torch, synth, bench, args.frames, args.rounds, off_only=args.off_only)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
