"""The One-Euro filter of include/pam.h (pam_one_euro) restated in plain Python floats: the step on one scalar channel, a track's 51
channels behind one shared header, and the per-id book-keeping of the device-side launch (restart, idempotence, hold).  Self-contained:
it does not import the package, and the filter uses no NumPy, so every operation is a Python float operation in the order written.

tests/test_one_euro_ref.py pins ``run`` to the outputs of the reference's own class (tests/golden/one_euro.npz) with ``==``."""
import math

PI = 3.141592653589793
ONE_EURO_3D = dict(freq=25.0, mincutoff=0.8, beta=0.4, dcutoff=0.4)        # IterTrack.__init__'s 3D filters
ONE_EURO_2D = dict(freq=25.0, mincutoff=1.7, beta=0.3, dcutoff=0.4)        # ... and its 2D ones


def alpha(freq, cutoff):
    te = 1.0 / freq
    tau = 1.0 / (2 * PI * cutoff)
    return 1.0 / (1.0 + tau / te)


class Header(object):
    """What the channels of one filter group share: samples taken, the sampling frequency, the last time stamp."""

    def __init__(self, freq):
        self.n, self.freq, self.t_last = 0, float(freq), 0.0

    def freq_for(self, t):
        """The frequency a sample at time t is filtered with: a time stamp of 0.0 counts as none (the class's truthiness test)."""
        if self.n > 0 and self.t_last != 0.0 and t != 0.0:
            return 1.0 / (t - self.t_last)
        return self.freq

    def advance(self, t):
        self.freq = self.freq_for(t)
        self.t_last = t
        self.n += 1


class Channel(object):
    def __init__(self):
        self.x_prev = self.x_hat = self.dx_hat = 0.0

    def step(self, cfg, hdr, t, x):
        """One sample; hdr is the header BEFORE the sample (the caller advances it once all its channels have stepped)."""
        freq = hdr.freq_for(t)
        if hdr.n == 0:
            edx = 0.0
        else:
            dx = (x - self.x_prev) * freq
            ad = alpha(freq, cfg['dcutoff'])
            edx = ad * dx + (1.0 - ad) * self.dx_hat
        cut = cfg['mincutoff'] + cfg['beta'] * math.fabs(edx)
        if hdr.n == 0:
            out = x
        else:
            ax = alpha(freq, cut)
            out = ax * x + (1.0 - ax) * self.x_hat
        self.dx_hat, self.x_prev, self.x_hat = edx, x, out
        return out


def config(cfg=None):
    out = dict(ONE_EURO_3D)
    out.update({k.lower(): float(v) for k, v in (cfg or {}).items()})
    return out


class Group(object):
    """K channels behind one header (a track: K = 51)."""

    def __init__(self, cfg, K):
        self.cfg, self.hdr, self.ch = cfg, Header(cfg['freq']), [Channel() for _ in range(K)]

    def step(self, t, xs):
        out = [c.step(self.cfg, self.hdr, t, float(x)) for c, x in zip(self.ch, xs)]
        self.hdr.advance(t)
        return out

    def held(self):
        return [c.x_hat for c in self.ch]


def run(cfg, t, x):
    """t: n time stamps, x: n rows of K samples -> n rows of K outputs, every column through a new filter (pam_op_one_euro)."""
    cfg = config(cfg)
    g = Group(cfg, len(x[0]) if len(x) else 0)
    return [g.step(float(ti), row) for ti, row in zip(t, x)]


class Bank(object):
    """The filters of a scene, keyed by track id, under the rules of pam_one_euro.  A dead track's filters are never asked for again (ids
    are not reused between resets), so keeping them by id is what the device does by slot."""

    def __init__(self, cfg=None):
        self.cfg = config(cfg)
        self.reset()

    def reset(self):
        self.groups, self.last_frame, self.restarts = {}, {}, 0

    def frame(self, frame_id, tracks):
        """tracks: [(id, last_time, raw pose as 51 floats)] in list order -> [(pose as 51 floats, fresh, samples)] in that order."""
        t = float(frame_id) / self.cfg['freq']
        rows = []
        for tid, last_time, raw in tracks:
            raw = [float(v) for v in raw]
            g = self.groups.get(tid)
            if last_time != frame_id:                                       # not fresh: the held output, or the raw pose without state
                rows.append((g.held(), False, g.hdr.n) if g is not None else (raw, False, 0))
                continue
            if g is not None and self.last_frame[tid] == frame_id:          # consumed already
                rows.append((g.held(), True, g.hdr.n))
                continue
            if g is None or frame_id < self.last_frame[tid]:                # new, or time went back
                self.restarts += g is not None
                g = self.groups[tid] = Group(self.cfg, len(raw))
            rows.append((g.step(t, raw), True, g.hdr.n))
            self.last_frame[tid] = frame_id
        return rows


def golden_sequences():
    """tests/golden/one_euro.npz (tools/make_one_euro_goldens.py: the reference's own class on seeded sequences) -> a list of dict(cfg, n,
    K, start, rate, t (n,), x (n, K), out (n, K)) with NumPy arrays."""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'one_euro.npz'))
    seqs, pt, px = [], 0, 0
    for row in z['seq']:
        n, K = int(row[0]), int(row[1])
        seqs.append(dict(n=n, K=K, start=int(row[2]), rate=float(row[3]),
                         cfg=dict(freq=float(row[4]), mincutoff=float(row[5]), beta=float(row[6]), dcutoff=float(row[7])),
                         t=z['t'][pt:pt + n].copy(), x=z['x'][px:px + n * K].reshape(n, K).copy(),
                         out=z['out'][px:px + n * K].reshape(n, K).copy()))
        pt, px = pt + n, px + n * K
    assert pt == len(z['t']) and px == len(z['x']) == len(z['out'])
    return seqs
