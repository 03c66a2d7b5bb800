#!/usr/bin/env python3
"""The demo loop's output stage, measured: testmodel's loop on Shelf-like 5 x 1032 x 776 JPEG frames with
VISUALIZATION + SAVE_IMAGE on the host path (PIL drawing, Image.save on the main thread), on the device path (DATASET.DEVICE_OVERLAY:
pam_overlay_draw, pam_jpeg_forward, pam.egress.FrameWriter) and with both keys off; the two kernels per frame set by HIP events; the
host Huffman pass against Image.save; and, with --parent DIR (a built checkout of the parent commit), bench.py's default loop on both
trees.  One process, the forms interleaved, medians of --rounds rounds.

    python tools/bench_overlay.py [--frames 40] [--rounds 7] [--parent DIR] [--skip-loop]"""
import argparse
import io
import json
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import pam  # noqa: E402
from pam import _lib, synth  # noqa: E402
from pam.dataset import GetConfig, LoadFilenames  # noqa: E402


def med(xs):
    return statistics.median(xs)


def make_dataset(root, n_frames):
    """A Shelf-like sequence on disk: 5 cameras of 1032 x 776 JPEGs, the calibration, the precomputed boxes and 2D poses."""
    seq = synth.make_sequence('S2', n_frames=n_frames, seed=1)
    rng = np.random.default_rng(0)
    base = np.asarray(Image.fromarray(rng.integers(0, 256, (97, 129, 3), dtype=np.uint8)).resize((1032, 776), Image.BILINEAR))
    for c in range(5):
        os.makedirs(os.path.join(root, 'Camera%d' % c))
        for t in range(n_frames):
            Image.fromarray(np.roll(base, t * 7 + c, axis=1)).save(os.path.join(root, 'Camera%d' % c, '%04d.jpg' % t), quality=92)
    with open(os.path.join(root, 'camera_parameter.pickle'), 'wb') as f:
        pickle.dump(seq['calib'], f)
    pre = {}
    for t, views in enumerate(seq['frames']):
        _, dr = synth.to_dump_results(views)
        pre[t] = [[dict(bbox=d['bbox'], keypoints=d['keypoints'], keypoints_score=d['keypoints_score']) for d in v] for v in dr]
    with open(os.path.join(root, 'detections.pickle'), 'wb') as f:
        pickle.dump(pre, f)


def loop(root, out, n_frames, form):
    """One run of testmodel's loop -> frames per second from the first frame's end to the return (the writer's drain included)."""
    from pam import testmodel
    cfg = GetConfig(os.path.join(pam.PKG_DIR, 'configs', 'Shelf', 'model_configs.yaml'))
    cfg.DATASET.ROOT = root; cfg.DATASET.TEST_RANGE = [0, n_frames]; cfg.OUTPUT = out
    cfg.PIPELINE_COMBINATION.POSE_MODEL = 'Precomputed'
    cfg.VISUALIZATION = cfg.SAVE_IMAGE = form != 'off'
    cfg.DATASET.DEVICE_OVERLAY = form == 'device'
    stamps = []
    devnull = open(os.devnull, 'w')
    stdout, sys.stdout = sys.stdout, devnull
    try:
        testmodel.test_ivclabpose_PersonTrack_Project3DPose(cfg, LoadFilenames(cfg.DATASET), on_frame=lambda *a: stamps.append(time.perf_counter()))
    finally:
        sys.stdout = stdout
        devnull.close()
    return (len(stamps) - 1) / (time.perf_counter() - stamps[0])


def kernels(n_views, w, h, persons, iters=20):
    """-> (pam_overlay_draw, pam_jpeg_forward) microseconds per frame set of n_views frames, by HIP events."""
    import torch
    from pam import visualization as V
    from pam.egress import coef_words
    lib = _lib.load()
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(n_views)]
    people = []                                                          # a person: 17 joints within a box a third of the frame high
    for _ in range(n_views):
        ppl = []
        for p in range(persons):
            cy, cx = rng.uniform(0.25 * h, 0.75 * h), rng.uniform(0.15 * w, 0.85 * w)
            ppl.append((np.stack([cy + rng.uniform(-h / 6, h / 6, 17), cx + rng.uniform(-h / 12, h / 12, 17), np.ones(17)], axis=1), p))
        people.append(ppl)
    table, ranges = V.overlay_table(people, [(w, h)] * n_views)
    prims = torch.from_numpy(table).cuda()
    views = (_lib.PamOverlayView * n_views)()
    for v, f, (first, count) in zip(views, frames, ranges):
        v.dev_bgr, v.width, v.height, v.prim_first, v.prim_count = f.data_ptr(), w, h, first, count
    tables = np.zeros((2, 64), dtype=np.uint16)
    lib.pam_jpeg_quality_tables(75, tables.ctypes.data)
    quant = torch.from_numpy(tables[[0, 1, 1]].copy()).cuda()
    words = coef_words(w, h, 2, 2)
    coef = torch.empty(n_views * words, dtype=torch.int16, device='cuda')
    images = (_lib.PamJpegFwdImage * n_views)()
    for k, (im, f) in enumerate(zip(images, frames)):
        im.dev_bgr, im.dev_quant, im.dev_coef = f.data_ptr(), quant.data_ptr(), coef.data_ptr() + 2 * k * words
        im.width, im.height, im.h_samp, im.v_samp = w, h, 2, 2
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for call in (lambda: lib.pam_overlay_draw(stream, n_views, views, prims.data_ptr(), len(table)),
                 lambda: lib.pam_jpeg_forward(stream, n_views, images)):
        times = []
        for _ in range(3):
            assert call() == 0
        torch.cuda.synchronize()
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); assert call() == 0; b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        out.append(med(times))
    return out[0], out[1], len(table)


def host_encode(rounds):
    """pam_jpeg_encode of one 1032 x 776 frame's coefficients on one thread against Image.save of the same pixels -> (ms, ms, bytes)."""
    import ctypes as C
    import torch
    from pam.egress import coef_words
    lib = _lib.load()
    rng = np.random.default_rng(0)
    rgb = np.asarray(Image.fromarray(rng.integers(0, 256, (97, 129, 3), dtype=np.uint8)).resize((1032, 776), Image.BILINEAR))
    frame = torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).cuda()
    tables = np.zeros((2, 64), dtype=np.uint16)
    lib.pam_jpeg_quality_tables(75, tables.ctypes.data)
    quant = torch.from_numpy(tables[[0, 1, 1]].copy()).cuda()
    words = coef_words(1032, 776, 2, 2)
    coef = torch.empty(words, dtype=torch.int16, device='cuda')
    im = (_lib.PamJpegFwdImage * 1)()
    im[0].dev_bgr, im[0].dev_quant, im[0].dev_coef = frame.data_ptr(), quant.data_ptr(), coef.data_ptr()
    im[0].width, im[0].height, im[0].h_samp, im[0].v_samp = 1032, 776, 2, 2
    assert lib.pam_jpeg_forward(None, 1, im) == 0
    host = coef.cpu().numpy()
    p = _lib.PamJpegEncodeParams(width=1032, height=776, h_samp=2, v_samp=2, quality=75)
    cap = C.c_size_t(0)
    lib.pam_jpeg_encode_bound(1032, 776, 2, 2, C.byref(cap))
    out = np.empty(cap.value, dtype=np.uint8)
    n = C.c_size_t(0)
    ours, pil = [], []
    pil_im = Image.fromarray(rgb)
    for _ in range(rounds):
        t0 = time.perf_counter()
        assert lib.pam_jpeg_encode(host.ctypes.data, host.size, C.byref(p), out.ctypes.data, out.size, C.byref(n)) == 0
        t1 = time.perf_counter()
        buf = io.BytesIO()
        pil_im.save(buf, format='JPEG')
        t2 = time.perf_counter()
        ours.append((t1 - t0) * 1e3); pil.append((t2 - t1) * 1e3)
    assert bytes(out[:n.value]) == buf.getvalue()
    return med(ours), med(pil), n.value


def bench_default(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '100', '--warmup', '10'], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if not lines:
        raise RuntimeError('bench.py in %s printed no result: %s' % (tree, out.stderr[-2000:]))
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: bench.py alternates between it and this tree')
    ap.add_argument('--skip-loop', action='store_true')
    a = ap.parse_args()
    res = {}
    if not a.skip_loop:
        with tempfile.TemporaryDirectory() as tmp:
            root = os.path.join(tmp, 'Shelf')
            make_dataset(root, a.frames)
            fps = {'off': [], 'host': [], 'device': []}
            for r in range(a.rounds + 1):                                # round 0 warms every form up and is dropped
                for form in fps:
                    v = loop(root, os.path.join(tmp, 'out_%s' % form), a.frames, form)
                    if r:
                        fps[form].append(v)
            res['loop_fps'] = {k: dict(median=round(med(v), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in fps.items()}
            print('loop', json.dumps(res['loop_fps']), flush=True)
    res['kernels_us'] = {}
    for name, (n_views, w, h, persons) in {'shelf_4': (5, 1032, 776, 4), 'shelf_8': (5, 1032, 776, 8), 'rig31_4': (31, 1920, 1080, 4),
                                           'rig31_8': (31, 1920, 1080, 8)}.items():
        draw, fwd, n_prims = kernels(n_views, w, h, persons)
        res['kernels_us'][name] = dict(overlay_draw=round(draw, 1), jpeg_forward=round(fwd, 1), primitives=n_prims)
    print('kernels', json.dumps(res['kernels_us']), flush=True)
    ours, pil, nbytes = host_encode(max(a.rounds, 7))
    res['host_encode_ms'] = dict(pam_jpeg_encode=round(ours, 2), image_save=round(pil, 2), file_bytes=nbytes)
    print('encode', json.dumps(res['host_encode_ms']), flush=True)
    if a.parent:
        vals = {'this': [], 'parent': []}
        for r in range(3):
            for name, tree in (('this', ROOT), ('parent', os.path.abspath(a.parent))):
                vals[name].append(bench_default(tree).get('value'))
        res['bench_default'] = vals
        print('bench', json.dumps(vals), flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
