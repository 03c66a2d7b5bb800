#!/usr/bin/env python3
"""Drawing the tracks from the device-resident state, measured.  One process, the forms interleaved, medians of
--rounds rounds; one JSON line at the end.

  launches   pam_overlay_tracks + pam_overlay_draw_counted per frame set, by HIP events, each alone and as the pair, at 5 views x 4
             tracks (S2: 1032 x 776) and 31 views x 16 tracks (an S4 rig, 1920 x 1080, with 16 people), plus one 640 x 480 3D view each.
  host form  the same drawing through the host table, wall clock from the issue to the end of the draw: fetch the record, decode it,
             visualization.track_rows, overlay_table, upload, pam_overlay_draw -- against the wall clock of the two launches.
  pipeline   an S2 FramePipeline (no network: the keypoints are given) feeding a FrameWriter, frames/s with overlay_step, with the
             same loop drawing through draw_tracks(device=True) from the fetched record, and with no drawing at all.

    python tools/bench_overlay_tracks.py [--rounds 7] [--iters 20] [--frames 150] [--skip-pipeline]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pam import _lib, synth  # noqa: E402
from pam import visualization as V  # noqa: E402
from pam.tracker import TrackView  # noqa: E402

med = statistics.median


def build_state(size, people, n_frames=5):
    """A tracker whose state holds `people` tracks of a synthetic sequence on the rig of `size` -> (model, tracks in the list)."""
    from pam.ivclabpose import ivclabpose
    name = '%s_%d' % (size, people)
    synth.SIZES[name] = dict(synth.SIZES[size], P=people)
    try:
        seq = synth.make_sequence(name, n_frames=n_frames, seed=3, noise_px=0.5, outlier_p=0.0)
    finally:
        del synth.SIZES[name]
    cfg = dict(synth.MATCHER_CFG[synth.SIZE_TO_DATASET[size]]); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=max(8, people), max_tracks=max(16, 2 * people))
    cams = model.GetCameraParameters(seq['calib'], seq['meta']['w'], seq['meta']['h'])
    for t in range(n_frames):
        model.tracker.tracking(t, cams, None, None, [d[:, :, [1, 0, 2]] for d in seq['frames'][t]])
    return model, seq['meta']['w'], seq['meta']['h'], len(model.tracker.last['tracks'])


def timed(call, iters):
    """-> microseconds per call by HIP events (median of iters)."""
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return med(out)


def wall(call, iters):
    """-> microseconds per call, host clock, the device idle before and after."""
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); call(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return med(out)


def launches(size, people, rounds, iters):
    model, w, h, n_tracks = build_state(size, people)
    trk, cams = model.tracker, model.cameras
    handle, lib, n_cam = trk.handle, trk.handle.lib, len(cams)
    dev = torch.device('cuda:0')
    frames = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(n_cam)]
    canvas = torch.zeros((480, 640, 3), dtype=torch.uint8, device=dev)
    extra = torch.from_numpy(V.view3d_camera(cams, (640, 480)).reshape(1, 3, 4)).to(dev)
    both = frames + [canvas]
    n, cap = len(both), _lib.OVERLAY_TRACK_ROWS * handle.max_tracks
    prims = torch.zeros((n, cap, 8), dtype=torch.int32, device=dev)
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    tv, dv = (_lib.PamOverlayTrackView * n)(), (_lib.PamOverlayView * n)()
    for k, f in enumerate(both):
        tv[k].camera, tv[k].extra, tv[k].width, tv[k].height = (k if k < n_cam else -1), 0, f.shape[1], f.shape[0]
        dv[k].dev_bgr, dv[k].width, dv[k].height, dv[k].prim_first, dv[k].prim_count = f.data_ptr(), f.shape[1], f.shape[0], k * cap, cap
    st = torch.cuda.current_stream().cuda_stream
    pal = V.track_palette()
    table = lambda: handle.overlay_tracks(st, tv, pal, prims, count, extra_P=extra, emitted_only=False)
    draw = lambda: lib.pam_overlay_draw_counted(st, n, dv, prims.data_ptr(), n * cap, count.data_ptr())
    pair = lambda: (table(), draw())
    keep, oi, od = handle.pinned_record()

    def host_form():                                                         # the 2D views only: the host path has no 3D view
        handle.fetch(st, oi, od); handle.sync(st)
        rec = handle.decode(0, oi, od)
        V.draw_tracks(frames, cams, [TrackView(r, cams, None) for r in rec['tracks']], emitted_only=False, device=True)
    device_form = lambda: V.draw_tracks_device(handle, frames, emitted_only=False)
    forms = dict(overlay_tracks_us=lambda: timed(table, iters), draw_counted_us=lambda: timed(draw, iters), pair_us=lambda: timed(pair, iters),
                 device_form_wall_us=lambda: wall(device_form, iters), host_table_wall_us=lambda: wall(host_form, iters))
    got = {k: [] for k in forms}
    for r in range(rounds + 1):                                              # round 0 warms every form up and is dropped
        for k, fn in forms.items():
            v = fn()
            if r:
                got[k].append(v)
    torch.cuda.synchronize()
    return dict({k: round(med(v), 1) for k, v in got.items()}, views=n, tracks=n_tracks, rows=int(count.sum().item()))


def pipeline(rounds, n_frames):
    from pam.egress import FrameWriter
    from pam.pipeline import FramePipeline
    size, md = 'S2', 8
    seq = synth.make_sequence(size, n_frames=n_frames, seed=1)
    cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
    from pam.ivclabpose import ivclabpose
    cams = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf).GetCameraParameters(seq['calib'], 1032, 776)
    nd_all, dd_all = synth.pack_frames(seq['frames'], md)
    pipes = dict(none=FramePipeline(cams, cfg, conf, (776, 1032), max_dets=md, max_tracks=16, hrnet=False),
                 host_table=FramePipeline(cams, cfg, conf, (776, 1032), max_dets=md, max_tracks=16, hrnet=False),
                 overlay_step=FramePipeline(cams, cfg, conf, (776, 1032), max_dets=md, max_tracks=16, hrnet=False, overlay=dict(view3d=None)))
    dev = pipes['none'].device
    from PIL import Image                                                    # tools/bench_overlay.py's images: an upscaled noise field
    base = np.asarray(Image.fromarray(np.random.default_rng(0).integers(0, 256, (97, 129, 3), dtype=np.uint8)).resize((1032, 776), Image.BILINEAR))
    clean = [torch.from_numpy(np.roll(base, 7 * c, axis=1).copy()).to(dev) for c in range(5)]
    ring = [[torch.empty_like(f) for f in clean] for _ in range(6)]         # a writer of depth 4 may still be reading four sets
    nd = [torch.tensor(x, dtype=torch.int32, device=dev) for x in nd_all]
    dd = [torch.tensor(x, dtype=torch.float64, device=dev) for x in dd_all]
    fps = {k: [] for k in pipes}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [[os.path.join(tmp, '%d_%d.jpg' % (t, c)) for c in range(5)] for t in range(n_frames)]
        for r in range(rounds + 1):
            for form, p in pipes.items():
                p.reset()
                writer = FrameWriter(0, workers=8, depth=4)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(n_frames):
                    frames = ring[t % len(ring)]
                    for f, c in zip(frames, clean):
                        f.copy_(c)
                    p.write_local(dd[t]); p.track_step(t, nd[t], fetch=form == 'host_table')
                    if form == 'overlay_step':
                        p.overlay_step(frames)
                    elif form == 'host_table':
                        rec = p.results()
                        V.draw_tracks(frames, cams, [TrackView(x, cams, None) for x in rec['tracks']], device=True)
                    writer.submit(t, frames, paths[t])
                writer.close()
                torch.cuda.synchronize()
                if r:
                    fps[form].append(n_frames / (time.perf_counter() - t0))
    return {k: dict(median=round(med(v), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in fps.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--frames', type=int, default=150)
    ap.add_argument('--skip-pipeline', action='store_true')
    a = ap.parse_args()
    res = dict(launches={})
    for name, (size, people) in dict(views5_tracks4=('S2', 4), views31_tracks16=('S4', 16)).items():
        res['launches'][name] = launches(size, people, a.rounds, a.iters)
        print('launches', name, json.dumps(res['launches'][name]), flush=True)
    if not a.skip_pipeline:
        res['pipeline_fps'] = pipeline(a.rounds, a.frames)
        print('pipeline', json.dumps(res['pipeline_fps']), flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
