#!/usr/bin/env python3
"""What the UDP protocol (box_transform='udp') costs beside the affine one it replaces.  One process, every form warmed,
forms interleaved, medians over rounds.

(i)  microseconds per crop launch (device events round `--calls` back-to-back launches) of pam_preprocess_crops_affine and of
     pam_preprocess_crops_udp on the SAME raw boxes, 256 x 192 x 8-channel output (ViTPose's input): 20 crops from 1032 x 776 frames,
     plain bilinear, and 35 crops from 1920 x 1080 frames with antialias.  The UDP grid's pitch is out_w / (out_w - 1) of the affine
     one: the same taps per output pixel over an area 1 % larger.
(ii) microseconds per decode (head pass + finish kernel) of pam_head_decode_dark and of pam_head_decode_udp at C = 48, 96 x 72, k = 17
     and at C = 256, 64 x 48, k = 11, plain (flags 0, 20 rows) and merged (flags 1, 20 + 20 rows), on features whose maps peak anywhere,
     border cells included (dark_ref's random-blob batch): the UDP window is 19^2 cells against DARK's 21^2, but DARK writes a border
     winner as it is while every UDP winner takes the full step.  pam_head_decode_udp at blur 0 (the plain arg-max through the UDP
     mapping) is timed too.

usage: bench_udp.py [--rounds 7] [--calls 200] [--out FILE.json] [--no-hd]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (256, 192)


def timed(torch, fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        if fn() != 0:
            raise RuntimeError('a launch failed')
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def interleaved(torch, forms, calls, rounds):
    for _, fn in forms:
        timed(torch, fn, 20)
    us = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, fn in forms:
            us[name].append(timed(torch, fn, calls))
    return us


def crop_launch(torch, n, views, fh, fw, tall, antialias, calls, rounds):
    from bench_affine_crop import person_boxes
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

    def form(fn):
        return lambda: fn(C.c_void_p(st.cuda_stream), n, n, 0, C.c_void_p(ptrs.data_ptr()), fh, fw, C.c_void_p(v_dev.data_ptr()),
                          C.c_void_p(b_dev.data_ptr()), _lib.BOX_SCALE, H, W, 8, C.c_void_p(out.data_ptr()), antialias, C.c_void_p(eff.data_ptr()))
    forms = [('affine', form(lib.pam_preprocess_crops_affine)), ('udp', form(lib.pam_preprocess_crops_udp)),
             ('affine_again', form(lib.pam_preprocess_crops_affine))]
    us = interleaved(torch, forms, calls, rounds)
    res = {name: dict(us_per_launch=float(np.median(v)), rounds=[round(x, 2) for x in v]) for name, v in us.items()}
    res.update(crops=n, frame=[fh, fw], antialias=int(antialias), output=list(RES) + [8],
               mean_pitch_affine=float(np.mean(eff.cpu().numpy()[:, 2] / W)), mean_pitch_udp=float(np.mean(eff.cpu().numpy()[:, 2] / (W - 1))),
               udp_over_affine=float(np.median(us['udp']) / np.median(us['affine'])),
               spread_affine=abs(float(np.median(us['affine']) - np.median(us['affine_again']))))
    return res


def decode(torch, Cc, h, w, k, n, calls, rounds):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import dark_ref as D
    from pam import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    feat, wt, b, boxes, _ = D.dark_inputs(Cc, h, w, n)
    f = torch.from_numpy(feat[:2 * n]).to(dev).to(torch.bfloat16).contiguous()
    wt_d, b_d, bx = torch.from_numpy(wt).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(boxes).to(dev)
    view_of = torch.zeros(n, dtype=torch.int32, device=dev)
    slot_of = torch.arange(n, dtype=torch.int32, device=dev)
    det = torch.empty((1, n, 17, 3), dtype=torch.float64, device=dev)
    scratch = torch.empty((int(lib.pam_head_decode_udp_scratch_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def form(fn, flags, kk):
        return lambda: fn(st(), n, n, h, w, p(f), Cc, p(wt_d), p(b_d), 17, flags, kk, None, p(view_of), p(slot_of), p(bx), n, p(det), None, p(scratch))
    out = {}
    for tag, flags in (('plain', 0), ('merged', 1)):
        forms = [('dark', form(lib.pam_head_decode_dark, flags, k)), ('udp', form(lib.pam_head_decode_udp, flags, k)),
                 ('udp_blur0', form(lib.pam_head_decode_udp, flags, 0)), ('dark_again', form(lib.pam_head_decode_dark, flags, k))]
        us = interleaved(torch, forms, calls, rounds)
        r = {name: dict(us_per_decode=float(np.median(v)), rounds=[round(x, 2) for x in v]) for name, v in us.items()}
        r.update(udp_over_dark=float(np.median(us['udp']) / np.median(us['dark'])),
                 spread_dark=abs(float(np.median(us['dark']) - np.median(us['dark_again']))))
        out[tag] = r
    out.update(C=Cc, map=[h, w], k=k, crops=n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-hd', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_udp.py needs a GPU: nothing is measured without one')
    import pam  # noqa: F401
    res = {'crop_launch': {'20_of_776x1032': crop_launch(torch, 20, 5, 776, 1032, 300.0, 0, args.calls, args.rounds)}}
    if not args.no_hd:
        res['crop_launch']['35_of_1080x1920_antialias'] = crop_launch(torch, 35, 5, 1080, 1920, 650.0, 1, args.calls, args.rounds)
    res['decode'] = {'C48_96x72_k17': decode(torch, 48, 96, 72, 17, 20, args.calls, args.rounds),
                     'C256_64x48_k11': decode(torch, 256, 64, 48, 11, 20, args.calls, args.rounds)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
