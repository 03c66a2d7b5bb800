#!/usr/bin/env python3
"""Generate tests/golden/one_euro.npz by RUNNING THE REFERENCE's OneEuroFilter class (loaded from /root/reference/src/tracking) on
seeded sequences.  Development-time only: the reference is read-only and does not exist on the GPU box; the fixture is committed.  It
holds data only: per sequence the configuration, the time stamps, the samples and what the class returned.

Usage (from the repo root):  python tools/make_one_euro_goldens.py [--out tests/golden/one_euro.npz]

Layout (flat arrays, one row of `seq` per sequence):
  seq   (S, 8) float64   n, K, start frame, frame rate, freq, mincutoff, beta, dcutoff
  t     (sum n,)         time stamps, frame / frame rate, sequence after sequence
  x     (sum n * K,)     samples, row-major (n, K) per sequence, |x| <= 10
  out   (sum n * K,)     the class's outputs, one new OneEuroFilter(freq, mincutoff, beta, dcutoff) per column
"""
import argparse
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = '/root/reference/src/tracking/OneEuroFilter.py'

CFG_3D = dict(freq=25, mincutoff=0.8, beta=0.4, dcutoff=0.4)      # IterativeTracker.py:225-230
CFG_2D = dict(freq=25, mincutoff=1.7, beta=0.3, dcutoff=0.4)      # IterativeTracker.py:219-224


def load_class():
    spec = importlib.util.spec_from_file_location('ref_one_euro', REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.OneEuroFilter


def plan():
    """(n, K, start frame, frame rate, config) per sequence."""
    rows = [(4, 300, 0, 25, CFG_3D), (10, 51, 297, 25, CFG_3D), (10, 51, 0, 25, CFG_2D), (1, 1, 0, 25, CFG_3D), (1, 51, 297, 25, CFG_2D)]
    rng = np.random.default_rng(20261019)
    for i in range(30):
        cfg = dict((CFG_3D, CFG_2D, dict(CFG_3D, beta=0.0))[i % 3])
        rate = (25, 30, 12.5)[(i // 3) % 3]
        cfg['freq'] = rate
        rows.append((int(rng.integers(2, 45)), 1, (0, 297, 1, 5)[i % 4], rate, cfg))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'one_euro.npz'))
    args = ap.parse_args()
    OneEuroFilter = load_class()
    rng = np.random.default_rng(7)
    seq, ts, xs, outs = [], [], [], []
    for n, K, start, rate, cfg in plan():
        frames = start + np.concatenate([[0], np.cumsum(rng.integers(1, 8, size=n - 1))])          # gaps of 1 to 7 frames
        t = frames.astype(np.float64) / float(rate)
        # a walk of up to 1.5 units per second with 5 mm noise, from a random place, clipped to |x| <= 10
        x0, v = rng.uniform(-8, 8, size=K), rng.uniform(-1.5, 1.5, size=K)
        x = np.clip(x0[None] + v[None] * (t - t[0])[:, None] + rng.normal(0, 0.005, size=(n, K)), -10.0, 10.0)
        out = np.zeros_like(x)
        for k in range(K):
            f = OneEuroFilter(**cfg)
            for i in range(n):
                out[i, k] = f(float(x[i, k]), float(t[i]))
        seq.append([n, K, start, rate, cfg['freq'], cfg['mincutoff'], cfg['beta'], cfg['dcutoff']])
        ts.append(t); xs.append(x.ravel()); outs.append(out.ravel())
    np.savez(args.out, seq=np.array(seq, dtype=np.float64), t=np.concatenate(ts), x=np.concatenate(xs), out=np.concatenate(outs))
    print('%s: %d sequences, %d samples, %d bytes' % (args.out, len(seq), sum(len(a) for a in xs), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
