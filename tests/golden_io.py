"""Readers for tests/golden/*.npz (written by tools/make_goldens.py from the reference)."""
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIZES = ('S1', 'S2', 'S3', 'S4')
RESCORED = ('S1s', 'S2s', 'S3s')        # trace_<S>s.npz: stress sequences of <S> with redrawn scores (synth.rescore_frames), on <S>'s rig


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def ops(size):
    """dict op -> list of record dicts."""
    z = load('ops_%s.npz' % size)
    out = {}
    for k in z.files:
        parts = k.split('.')
        if parts[1] == 'count':
            out.setdefault(parts[0], [dict() for _ in range(int(z[k]))])
    for k in z.files:
        parts = k.split('.')
        if parts[1] != 'count':
            out[parts[0]][int(parts[1])][parts[2]] = z[k]
    return out


def cameras(size):
    return load('cameras_%s.npz' % (size[:-1] if size in RESCORED else size))


def camera_variants(size):
    """The reference's camera set-up on each of MKL's kernel paths: cameras_<S>.npz (AVX-512, Intel), cameras_<S>_mkl_avx2.npz (AVX2,
    Intel without AVX-512) and cameras_<S>_mkl_compatible.npz (MKL's baseline path, the one it runs on other vendors' CPUs, e.g. AMD
    EPYC).  Their float32 3x3 products round differently; only F differs."""
    return [cameras(size), load('cameras_%s_mkl_avx2.npz' % size), load('cameras_%s_mkl_compatible.npz' % size)]


def trace_frames(tr):
    """list[frame][view] -> (n,17,3) arrays in the dump layout (x, y, score)."""
    n_det = tr['in.n_det']
    dets = tr['in.dets']
    frames, pos = [], 0
    for t in range(n_det.shape[0]):
        views = []
        for c in range(n_det.shape[1]):
            n = int(n_det[t, c])
            views.append(dets[pos:pos + n].reshape(n, 17, 3))
            pos += n
        frames.append(views)
    return frames
