#!/usr/bin/env python3
"""What decoding baseline JPEG frames on the device (FrameLoader(device_decode=True)) costs and gains, against the Pillow
path, in ONE process with the two forms interleaved and medians over rounds.  One JSON line.

  --host      (no GPU needed) single-thread ms per image of a worker's work: `pam_jpeg_probe` + `pam_jpeg_entropy` into a preallocated
              buffer, against Pillow's full decode plus the channel-flipped copy (what `_decode_pinned` does), on tools/bench_ingest.py's
              1032 x 776 images at quality 92 and on a quality-75 and a quality-95 set.
  (default)   on a GPU: Shelf frame sets/s to the device at 1 / 4 / 8 / 16 workers for both paths, us per `pam_jpeg_reconstruct` launch
              pair over one Shelf frame set (5 x 1032 x 776, 4:2:0), and -- unless --no-pipeline -- frames/s of an S2 FramePipeline with
              boxes given, fed from the loader both ways.
usage: bench_jpeg.py [--host] [--rounds 7] [--sets 120] [--no-pipeline] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, CAMS = 1032, 776, 5


def write_sets(directory, n_sets, quality, size=(W, H)):
    """tools/bench_ingest.py's images: an upscaled 129 x 97 noise field, rolled per camera and frame.  -> list over sets of file names."""
    from PIL import Image
    base = np.random.default_rng(0).integers(0, 256, (97, 129, 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(base).resize(size, Image.BILINEAR))
    frames = []
    for t in range(n_sets):
        fs = []
        for c in range(CAMS):
            p = os.path.join(directory, 'q%d_c%d_%03d.jpg' % (quality, c, t))
            Image.fromarray(np.roll(img, t * 7 + c, axis=1)).save(p, quality=quality)
            fs.append(p)
        frames.append(fs)
    return frames


def host_pass(rounds):
    from PIL import Image
    from pam import _lib
    lib = _lib.load()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for q in (92, 75, 95):
            files = [f for fs in write_sets(tmp, 6, q) for f in fs]
            datas = [open(f, 'rb').read() for f in files]
            info = _lib.PamJpegInfo()
            assert lib.pam_jpeg_probe(datas[0], len(datas[0]), info) == 0 and not info.unsupported
            coef = np.empty(int(info.coef_words), dtype=np.int16)
            flipped = np.empty((H, W, 3), dtype=np.uint8)

            def entropy():
                for d in datas:
                    i = _lib.PamJpegInfo()
                    lib.pam_jpeg_probe(d, len(d), i)
                    assert lib.pam_jpeg_entropy(d, len(d), i, coef.ctypes.data, coef.size) == 0

            def pillow(copy):
                for f in files:
                    with Image.open(f) as im:
                        rgb = np.asarray(im.convert('RGB'))
                    if copy:
                        np.copyto(flipped, rgb[:, :, ::-1])

            forms = [('entropy_ms', entropy), ('pillow_decode_ms', lambda: pillow(False)), ('pillow_worker_ms', lambda: pillow(True))]
            ms = {k: [] for k, _ in forms}
            for r in range(rounds + 1):
                for k, fn in forms:
                    t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                    if r:                                              # round 0 warms the page cache and the buffers
                        ms[k].append(dt * 1e3 / len(files))
            out['q%d' % q] = dict({k: round(float(np.median(v)), 3) for k, v in ms.items()},
                                  bytes_per_file=int(np.mean([len(d) for d in datas])), images=len(files))
    return out


def loader_rate(torch, frames, workers, device_decode, skip):
    from pam.ingest import FrameLoader
    ld = FrameLoader('Shelf', frames, workers=workers, depth=6, device=torch.device('cuda:0'), device_decode=device_decode)
    n = 0
    for idx, imgs, ts in ld:
        n += 1
        if n == skip:
            torch.cuda.synchronize(); t0 = time.perf_counter()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ld.close()
    assert ld.fallbacks == 0 and ld.device_decoded == (CAMS * n if device_decode else 0)
    return (n - skip) / dt


def ingest(torch, rounds, n_sets):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        sets = write_sets(tmp, 40, 92)
        for workers in (1, 4, 8, 16):
            n = max(40, n_sets // 3) if workers == 1 else n_sets
            frames = (sets * ((n + 39) // 40 + 1))[:n + 20]             # the first 20 sets (staging buffers are allocated on the way) are not timed
            rates = {'pillow': [], 'device': []}
            for r in range(rounds + 1):
                for name in ('pillow', 'device'):
                    v = loader_rate(torch, frames, workers, name == 'device', 20)
                    if r:
                        rates[name].append(v)
            out['workers_%d' % workers] = {k: dict(sets_per_s=round(float(np.median(v)), 1), rounds=[round(x, 1) for x in v]) for k, v in rates.items()}
    return out


def launch_pair(torch, rounds, calls=50):
    """us per pam_jpeg_reconstruct over one Shelf frame set, coefficients resident on the device (HIP events round `calls` calls)."""
    from pam import _lib
    lib = _lib.load()
    with tempfile.TemporaryDirectory() as tmp:
        files = write_sets(tmp, 1, 92)[0]
        images = (_lib.PamJpegImage * CAMS)()
        keep = []
        for im, f in zip(images, files):
            d = open(f, 'rb').read()
            info = _lib.PamJpegInfo()
            assert lib.pam_jpeg_probe(d, len(d), info) == 0 and not info.unsupported
            host = np.zeros(256 + int(info.coef_words), dtype=np.int16)
            host[:192].view(np.uint16)[:] = np.ctypeslib.as_array(info.quant).reshape(-1)
            assert lib.pam_jpeg_entropy(d, len(d), info, host[256:].ctypes.data, int(info.coef_words)) == 0
            coef = torch.from_numpy(host).cuda()
            planes = torch.empty(int(info.coef_words), dtype=torch.uint8, device='cuda:0')
            out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device='cuda:0')
            im.dev_quant, im.dev_coef, im.dev_planes, im.dev_out = coef.data_ptr(), coef.data_ptr() + 512, planes.data_ptr(), out.data_ptr()
            im.width, im.height, im.n_comp, im.h_samp, im.v_samp = info.width, info.height, info.n_comp, info.h_samp[0], info.v_samp[0]
            keep.append((coef, planes, out))
    stream = torch.cuda.current_stream().cuda_stream
    us = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            lib.pam_jpeg_reconstruct(stream, CAMS, images)
        b.record(); torch.cuda.synchronize()
        if r:
            us.append(a.elapsed_time(b) * 1e3 / calls)
    bytes_moved = sum(c.numel() * 2 + 2 * p.numel() + o.numel() for c, p, o in keep)     # coef in, planes out and in, frame out
    return dict(us_per_frame_set=round(float(np.median(us)), 1), rounds=[round(x, 1) for x in us], algorithmic_bytes=int(bytes_moved))


def pipeline(torch, rounds, frames_timed=200, warm=10):
    """S2 FramePipeline, boxes given, frames from the loader: Pillow path, device path, Pillow path again."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod_jpeg', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    from pam import synth
    from pam.ingest import FrameLoader
    from pam.pipeline import FramePipeline
    nF = frames_timed + warm
    wl = bench.setup_workload(synth, 'S2', nF)
    fh, fw, md = wl['meta']['h'], wl['meta']['w'], 8
    pipe = FramePipeline(wl['cams'], wl['cfg'], wl['conf'], (fh, fw), max_dets=md, max_tracks=16, overlap_tracker=True)
    dev = pipe.device
    pf = bench.build_inputs(torch, synth, wl['seq'], 'S2', md, 1, 0, 'views', dev, nF)['per_frame']
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        sets = write_sets(tmp, 40, 92, size=(fw, fh))
        files = (sets * (nF // 40 + 1))[:nF]

        def run(device_decode):
            pipe.reset()
            ld = FrameLoader('Shelf', files, workers=16, depth=6, device=dev, device_decode=device_decode)
            for t, (idx, imgs, ts) in enumerate(ld):
                if t == warm:
                    pipe.results(strict=False); torch.cuda.synchronize(); t0 = time.perf_counter()
                ptrs = torch.tensor([x.data_ptr() for x in imgs], dtype=torch.int64, device=dev)
                e = pf[t]
                with pipe.frame():
                    pipe.pose_step(ptrs, e['vl'], e['sl'], e['bx'])
                    pipe.write_local(e['dd']); pipe.track_step(t, e['nd'])
            pipe.results(strict=False); torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ld.close()
            return frames_timed / dt
        forms = [('pillow', False), ('device', True), ('pillow_again', False)]
        fps = {k: [] for k, _ in forms}
        for r in range(rounds + 1):
            for k, dd in forms:
                v = run(dd)
                if r:
                    fps[k].append(v)
        out = {k: dict(frames_per_s=round(float(np.median(v)), 1), rounds=[round(x, 1) for x in v]) for k, v in fps.items()}
        out['frame'] = [fh, fw]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--sets', type=int, default=120)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--no-ingest', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pam  # noqa: F401
    if args.host:
        res = {'host_pass_ms_per_image': host_pass(args.rounds)}
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit('bench_jpeg.py needs a GPU for everything but --host')
        res = {'launch_pair': launch_pair(torch, args.rounds)}
        if not args.no_ingest:
            res['ingest_sets_per_s'] = ingest(torch, args.rounds, args.sets)
        if not args.no_pipeline:
            res['pipeline_S2'] = pipeline(torch, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
