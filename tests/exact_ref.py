"""Exact references for the conv-stack kernels on integer-valued data (CPU only; the GPU side is tests/test_gpu_exact.py).

Operands are bf16 and accumulators fp32.  When every activation, weight, bias and residual is a small integer, every product and every
partial sum is an exact integer while it stays below 2^24, whatever the tile, slab, K order or wave count; the only inexact step is the
bf16 store (one round-to-nearest-even).  The right answer is then unique, and a kernel must reproduce it bit for bit.

This module holds
  * the arithmetic: ``rne_bf16`` / ``trunc_bf16`` / ``leaky32`` and a direct float64 convolution (unfold + matmul, ``conv_direct``);
  * ``Run``: one evaluation of a family's chain -- it records every convolution's raw sums, the exactness bound and the sharp / tie
    statistics of every compared output, and can carry ONE planted fault (``FAULTS``), applied to the reference and never to a kernel;
  * ``Data``: the seeded integer generator with its per-regime densities;
  * one reference per kernel family (``REFS``), with the operation order and rounding points of the kernels;
  * the case tables the GPU tests launch (``CASES``), so that tests/test_exact_ref.py can walk them without a GPU.

Regimes.  An output element is *sharp* when the value stored is a non-zero integer of magnitude <= 256 that came through an exact
activation branch (v > 0 under ReLU / leaky, any v for a linear output): it is stored without rounding, so a unit error in it shows.
A chain of k stages runs k regimes ``sharp-i`` -- stage i has dense weights (density 0.5) and a dense input, the stages before it get a
thinned head input and thinned weights, the stages after it thinned weights, each density taken from the mean square of that stage's
reference input and a target sigma (``SIGMA``) -- and one regime ``rounding``: the head input and the first stage's weights are dense
and their signs mostly follow their channel's (zero-mean products of |x| <= 3 and |w| <= 1 would leave a 48-channel sum at sigma ~ 45,
inside 256; ``COHERENCE`` < 1 keeps the weights from being rank one, so a channel mix-up still shows), and short sums draw larger
activations (``Data._scale``), so in EVERY case the sums spread well past 256 and the single rounding, ties included, is exercised; the later stages of a chain, which read
those large sums, get the weight density that keeps their own sums near ``SIGMA_ROUNDING`` -- dense weights there would push them to
10^5 .. 10^6, where hardly any value is a tie."""
import zlib

import torch
import torch.nn.functional as F

ROUND_W = 0.75               # rounding regime: weight density of the first stage
COHERENCE = 0.85             # ... a sign follows its channel's with probability (1 + COHERENCE) / 2: the sums get a mean, the weights keep structure
SIGMA_ROUNDING = 600.0       # ... of the later stages of a chain in the rounding regime
SIGMA = 40.0                 # target standard deviation of a sharp stage's pre-activation sums
EX2 = 14.0 / 3.0             # mean square of a non-zero activation drawn uniformly from {1, 2, 3} (either sign)
DENSE_W = 0.5
LIMIT = float(2 ** 24)       # fp32 significand: integer sums below it are exact in any order
SHARP_ACT, SHARP_LINEAR = 0.35, 0.9
ROUNDING_BIG, ROUNDING_TIES = 0.25, 100


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    """float32 magnitude bits (int64) and sign of t (float64 / float32 holding float32-representable values)."""
    f = t.to(torch.float32)
    assert bool((f.to(torch.float64) == t.to(torch.float64)).all()), 'value is not a float32'
    return f.abs().view(torch.int32).to(torch.int64), torch.where(torch.signbit(f), -1.0, 1.0).to(torch.float32)


def _from_bits(b, sign):
    return b.to(torch.int32).view(torch.float32) * sign


def rne_bf16(t):
    """The bf16 value (as float32) nearest to t, ties to the even bf16: what f32_to_bf16 / pack_bf16x2 store."""
    b, s = _bits(t)
    b = (b + 0x7fff + ((b >> 16) & 1)) & ~0xffff
    return _from_bits(b, s)


def trunc_bf16(t):
    """The bf16 value towards zero (planted fault f)."""
    b, s = _bits(t)
    return _from_bits(b & ~0xffff, s)


def is_tie(t):
    """True where t lies exactly halfway between two neighbouring bf16 values."""
    b, _ = _bits(t)
    return (b & 0xffff) == 0x8000


def leaky32(v):
    """Leaky ReLU as the kernels compute it: ``v > 0 ? v : 0.1f * v``, one float32 multiply."""
    v = v.to(torch.float32)
    return torch.where(v > 0, v, torch.tensor(0.1, dtype=torch.float32) * v)


def conv_direct(x, w, stride, pad):
    """Direct convolution in float64: the patches of x (N, Cin, H, W) unfolded to columns, one matrix product with w (Cout, Cin, k, k).
    Integer operands give the exact integer sums (float64 holds integers to 2^53)."""
    n, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    xp = F.pad(x.to(torch.float64), (pad, pad, pad, pad))
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    cols = F.unfold(xp, k, stride=stride)                                # (N, Cin k k, Ho Wo), rows ordered (cin, ky, kx)
    return (w.to(torch.float64).reshape(cout, cin * k * k) @ cols).reshape(n, cout, ho, wo)


def up_nearest(t, shift):
    return t.repeat_interleave(1 << shift, 2).repeat_interleave(1 << shift, 3)


# ---- planted faults --------------------------------------------------------------------------------------------------------------------------
# name -> (what it is, the regime in which it must show).  a, b, c live in one convolution's sums; d, e, h in its epilogue; f, g in the
# bf16 stores.  `stage` says which stage of a chain carries the fault (a-e, h); f hits the compared stores, g the intermediates.
FAULTS = {
    'a': ('one tap (the centre one) is skipped at the last output column', 'sharp'),
    'b': ('two input channels are swapped inside the last 8-channel group', 'sharp'),
    'c': ('the last 32-channel chunk of K (last tap) is dropped for the last 16 output channels', 'sharp'),
    'd': ('the bias is added after the activation', 'sharp'),
    'e': ('the residual is added after the bf16 rounding', 'rounding'),
    'f': ('truncation instead of round-to-nearest-even', 'rounding'),
    'g2': ('an intermediate is rounded twice: the raw sum, then the biased and activated value', 'rounding'),
    'g0': ('an intermediate is not rounded at all', 'rounding'),
    'h': ('relu_from is off by one 16-channel slab', 'sharp'),
}


class Run(object):
    """One evaluation of a family's reference.  The clean run (fault None) records the raw sums of every convolution; a faulted run
    given that clean run as `base` reuses the sums of the convolutions before the faulted stage."""

    def __init__(self, fault=None, stage=0, base=None):
        self.fault, self.stage, self.base = fault, stage, base
        self.raw = {}                    # convolution name -> raw sums
        self.bound = {}                  # epilogue name -> max|x| * max_cout sum|w| + |b| + |res| (exactness condition)
        self.outs = {}                   # compared output name -> dict(ref=bf16 values as float32, sharp, big, ties, vmax, ...)
        self.vals = {}                   # every store's name -> its bf16 values (float32)
        self.inter = set()               # stores that a later stage reads back (the intermediates of a chain)
        self.applied = False             # the fault found something to act on
        self._dirty = fault in ('f', 'g2', 'g0')
        self._xw = {}

    # -- convolution sums ---------------------------------------------------------------------------------------------------------------
    def conv(self, name, stage, x, w, stride, pad, tap=None):
        """tap: the (ky, kx) fault a skips -- default the centre tap, the one that never reads padding."""
        hit = self.stage == stage and self.fault in ('a', 'b', 'c')
        if self.base is not None and not self._dirty and name in self.base.raw:
            s = self.base.raw[name]
        else:
            s = conv_direct(x, w, stride, pad)
        self._xw[name] = float(x.abs().max()) * float(w.abs().sum((1, 2, 3)).max())
        if hit:
            s = s + self._delta(x, w, stride, pad, s.shape, tap or (w.shape[2] // 2, w.shape[2] // 2))
            self.applied = True
            self._dirty = True
        elif self.stage == stage and self.fault in ('d', 'e', 'h'):
            self._dirty = True                               # the epilogue of this stage changes: everything after it is recomputed
        self.raw[name] = s
        return s

    def _delta(self, x, w, stride, pad, shape, tap):
        """What the planted fault adds to the clean sums, computed on the few channels / columns it touches."""
        cout, cin, k, _ = w.shape
        d = torch.zeros(shape, dtype=torch.float64)
        if self.fault == 'a':
            # tap (ky, kx) is skipped at output column Wo - 1: minus its products there
            ox, (ky, kx) = shape[3] - 1, tap
            xp = F.pad(x.to(torch.float64), (pad, pad, pad, pad))
            col = xp[:, :, ky:, ox * stride + kx]                                                  # input column of tap kx
            rows = col[:, :, 0:(shape[2] - 1) * stride + 1:stride]                                 # (N, Cin, Ho)
            d[:, :, :, ox] = -torch.einsum('oc,nch->noh', w[:, :, ky, kx].to(torch.float64), rows)
        elif self.fault == 'b':
            # the pair of the last 8-channel group whose planes differ most (two all-zero post-ReLU planes would swap unseen)
            lo = max(0, cin - 8)
            last = x[:, lo:].to(torch.float64)
            dist = (last[:, :, None] - last[:, None, :]).abs().sum((0, 3, 4))
            c1, c2 = lo + int(dist.argmax()) // (cin - lo), lo + int(dist.argmax()) % (cin - lo)
            x2 = x[:, [c1, c2]].to(torch.float64)
            d = conv_direct(x2[:, [1, 0]] - x2, w[:, [c1, c2]], stride, pad)
        else:
            ck = min(32, cin)
            wl = torch.zeros((16, ck, k, k), dtype=torch.float64)
            wl[:, :, k - 1, k - 1] = w[-16:, -ck:, k - 1, k - 1].to(torch.float64)
            d[:, -16:] = -conv_direct(x[:, -ck:], wl, stride, pad)
        return d

    # -- epilogue: bias, residual, activation, the bf16 store -----------------------------------------------------------------------------
    def store(self, name, stage, sums, bias, res=None, act='relu', res_after=False, relu_from=0, final=True, conv_names=(), feeds=False,
              post=None):
        """out = rne(act(sum of `sums` + bias [+ res])), or rne(act(...) + res) with res_after (Darknet's shortcut); the activation
        applies to channels >= relu_from.  final: a compared output (statistics are kept); feeds (or not final): an intermediate of a
        chain, which the next stage reads as stored.  post: a monotone map applied before the store (the max-pool of k_resnet_stem: it
        commutes with the rounding, so where the kernel rounds relative to it cannot show).
        The clean value is ``epilogue`` followed by ``rne_bf16``, nothing else; a planted fault replaces one of the two."""
        inter = feeds or not final
        if inter:
            self.inter.add(name)
        s = sums[0]
        for t in sums[1:]:
            s = s + t
        b = bias.to(torch.float64).reshape(1, -1, 1, 1)
        r = res.to(torch.float64) if res is not None else None
        assert post is None or (r is None and relu_from == 0)
        # which fault, if any, acts on THIS store
        mine = self.stage == stage
        fault = self.fault
        if not ((fault == 'd' and mine and act != 'linear') or (fault == 'e' and mine and r is not None) or
                (fault == 'h' and mine and relu_from > 0) or (fault in ('g2', 'g0') and inter) or (fault == 'f' and final)):
            fault = None
        self.applied = self.applied or fault is not None
        if fault in FAULTY_EPILOGUES:
            z = FAULTY_EPILOGUES[fault](s, b, r, act, res_after, relu_from, post)
        else:
            z, v = epilogue(s, b, r, act, res_after, relu_from, post)
        out = trunc_bf16(z) if fault == 'f' else (z.to(torch.float32) if fault == 'g0' else rne_bf16(z))
        self.vals[name] = out
        if self.fault is None:
            self.bound[name] = sum(self._xw[c] for c in conv_names) + float(bias.abs().max()) + (float(r.abs().max()) if r is not None else 0.0)
            if final:
                exact_branch = (v > 0) | (torch.arange(v.shape[1]).reshape(1, -1, 1, 1) < relu_from) | (act == 'linear')
                az = z.abs()
                self.outs[name] = dict(ref=out, linear=act == 'linear', numel=out.numel(),
                                       sharp=float(((az > 0) & (az <= 256) & exact_branch).double().mean()),
                                       big=float((v.abs() > 256).double().mean()), ties=int(is_tie(z).sum()), vmax=float(v.abs().max()))
        elif final:
            self.outs[name] = dict(ref=out)
        return out


def activate(v, act, relu_from):
    if act == 'linear':
        return v
    a = torch.relu(v) if act == 'relu' else leaky32(v).to(torch.float64)
    return torch.cat([v[:, :relu_from], a[:, relu_from:]], 1) if relu_from else a


def add32(u, t):
    """One float32 addition (exact for integers; it rounds a leaky product + residual)."""
    return (u.to(torch.float32) + t.to(torch.float32)).to(torch.float64)


def epilogue(s, b, r, act, res_after, relu_from, post=None):
    """The kernels' epilogue up to the store -> (z, v): v = s + b [+ r] is the pre-activation value, z = act(v), or act(v) + r in
    float32 when the residual comes after the activation; `post` (a max-pool) maps both."""
    v = s + b
    if r is not None and not res_after:
        v = v + r
    z = activate(v, act, relu_from)
    if r is not None and res_after:
        z = add32(z, r)
    if post is not None:
        z, v = post(z), post(v)
    return z, v


def _bias_after_activation(s, b, r, act, res_after, relu_from, post):
    z = add32(activate(s + r if (r is not None and not res_after) else s, act, relu_from), b.expand_as(s))
    if r is not None and res_after:
        z = add32(z, r)
    return post(z) if post is not None else z


def _residual_after_rounding(s, b, r, act, res_after, relu_from, post):
    z = add32(rne_bf16(activate(s + b, act, relu_from)), r)
    return z if res_after else activate(z, act, relu_from)               # a residual meant to enter before the activation: act again


FAULTY_EPILOGUES = {
    'd': _bias_after_activation,
    'e': _residual_after_rounding,
    'g2': lambda s, b, r, act, res_after, relu_from, post: epilogue(rne_bf16(s).to(torch.float64), b, r, act, res_after, relu_from, post)[0],
    'h': lambda s, b, r, act, res_after, relu_from, post: epilogue(s, b, r, act, res_after, relu_from + 16, post)[0],
}


# ---- data -------------------------------------------------------------------------------------------------------------------------------------
def stage_of(regime):
    return None if regime == 'rounding' else int(regime.split('-')[1])


def regimes(case):
    return ['sharp-%d' % i for i in range(len(STAGE_K[case['family']](case)))] + ['rounding']


class Data(object):
    """Seeded integer tensors of one (case, regime), generated on first request in the order the reference asks for them and kept, so
    that a faulted run sees the very same data.  Weights {-1, 0, 1}, activations [-3, 3] (non-negative where the kernel is fed
    post-ReLU tensors; up to [-96, 96] in the rounding regime of short sums, see _scale), biases [-8, 8], residuals [-3, 3]."""

    def __init__(self, case, regime):
        self.case, self.regime = case, regime
        self.i = stage_of(regime)
        self.K = STAGE_K[case['family']](case)
        self.g = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (case['id'], regime)).encode()))
        self.t = {}
        self.dens = {}

    def _rand(self, shape):
        return torch.rand(shape, generator=self.g)

    def _mag(self, shape, scale=1):
        return torch.randint(1, 3 * scale + 1, shape, generator=self.g).to(torch.float64)

    def _scale(self, stage):
        """Rounding regime: head activations are drawn from [1, 3 m] (either sign), m the smallest power of two at which the mean |sum|
        of the stage, K * ROUND_W * (1.5 m + 0.5) * COHERENCE^2, reaches 400.  m = 1 from K = 384 on; the short sums (27 <= K <= 288:
        first layers, 64-channel pointwise layers, the 7x7 stem) need m = 2 .. 32, i.e. |x| <= 96 -- still exact bf16 integers, and
        the 2^24 bound is asserted as everywhere."""
        m = 1
        while self.K[stage] * ROUND_W * (1.5 * m + 0.5) * COHERENCE ** 2 < 400.0:
            m *= 2
        return m

    def _var_goal(self, stage):
        """Variance asked of a stage BEFORE the sharp one: its ReLU'd output (mean square about half the variance) feeds a stage
        with dense weights that should land on SIGMA."""
        return max(1.0, 2.0 * SIGMA ** 2 / (DENSE_W * self.K[stage + 1]))

    def head(self, name, shape, stage, nonneg=False):
        """An input tensor read by stage `stage`."""
        if name in self.t:
            return self.t[name]
        k = self.K[stage]
        if self.i is None:
            dens = 1.0
        elif stage == self.i:
            dens = min(1.0, max(0.5, 60.0 ** 2 / (k * DENSE_W * EX2)))           # dense, but a long K stays near the target sigma
        elif stage < self.i:
            dens = min(1.0, self._var_goal(stage) / (k * DENSE_W * EX2))
        else:
            dens = 1.0
        x = self._mag(shape, self._scale(stage) if self.i is None else 1) * (self._rand(shape) < dens)
        if not nonneg:
            if self.i is None:
                p = COHERENCE
                sc = torch.where(self._rand((1, shape[1], 1, 1)) < 0.5, -1.0, 1.0)
                x = x * sc * torch.where(self._rand(shape) < (1 + p) / 2, 1.0, -1.0)
            else:
                x = x * torch.where(self._rand(shape) < 0.5, -1.0, 1.0)
            self.t[name + '.sign'] = sc if self.i is None else None
        self.t[name] = x
        self.dens[name] = dens
        return x

    def weight(self, name, stage, cout, cin, k, xin, sign_of=None, sign_off=0):
        """Weights of a convolution of stage `stage` whose reference input is xin (its mean square sets a thinned density).
        sign_of: the head tensor whose per-channel signs the rounding regime's weights follow (None: a non-negative input), from its
        channel sign_off on."""
        if name in self.t:
            return self.t[name]
        shape = (cout, cin, k, k)
        if self.i is None and stage == 0:
            dens = ROUND_W
        elif self.i is None:
            # a later stage of a chain reads sums that already passed 256: dense weights would push its own sums to 10^4 .. 10^6, where
            # a tie is one value in 64 or fewer; SIGMA_ROUNDING keeps them where the rounding has most to decide
            ms = max(float((xin.to(torch.float64) ** 2).mean()), 1e-3)
            dens = min(DENSE_W, max(SIGMA_ROUNDING ** 2 / (self.K[stage] * ms), 8.0 / self.K[stage]))     # and >= 8 products per sum
        elif stage == self.i:
            dens = DENSE_W
        else:
            ms = max(float((xin.to(torch.float64) ** 2).mean()), 1e-3)
            goal = SIGMA ** 2 if stage > self.i else self._var_goal(stage)
            dens = min(DENSE_W, goal / (self.K[stage] * ms))
        w = (self._rand(shape) < dens).to(torch.float64)
        if self.i is None and stage == 0:
            p = COHERENCE
            sc = self.t.get(sign_of + '.sign') if sign_of else None
            so = torch.where(self._rand((cout, 1, 1, 1)) < 0.5, -1.0, 1.0)
            w = w * so * torch.where(self._rand(shape) < (1 + p) / 2, 1.0, -1.0)
            if sc is not None:
                w = w * sc.reshape(1, -1, 1, 1)[:, sign_off:sign_off + cin]
        else:
            w = w * torch.where(self._rand(shape) < 0.5, -1.0, 1.0)
        self.t[name] = w
        self.dens[name] = dens
        return w

    def bias(self, name, cout):
        if name not in self.t:
            self.t[name] = torch.randint(-8, 9, (cout,), generator=self.g).to(torch.float64)
        return self.t[name]

    def res(self, name, shape, nonneg=False):
        if name not in self.t:
            self.t[name] = torch.randint(0 if nonneg else -3, 4, shape, generator=self.g).to(torch.float64)
        return self.t[name]


# ---- the references, one per kernel family ------------------------------------------------------------------------------------------------
def out_hw(h, w, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1


def ref_conv(D, R, c):
    """One convolution with its epilogue (pam_conv2d_nhwc_bf16_ex and the kernels behind it, k_down48, k_down_s, k_pw1):
    out = act(conv(x) + b [+ res]) or act(conv(x) + b) + res; x may be a channel slice of a wider tensor; the activation may start at
    relu_from; output channels past `cout_real` are zero filters with a zero bias (PackedConv's pad_cout_to)."""
    n, h, w, cin, cout, k, stride = c['n'], c['h'], c['w'], c['cin'], c['cout'], c['k'], c['stride']
    wide, off = c.get('wide', cin), c.get('off', 0)
    real = c.get('cout_real', cout)
    xw = D.head('x', (n, wide, h, w), 0, nonneg=c.get('nonneg', False))
    x = xw[:, off:off + cin]
    wt = D.weight('w', 0, real, cin, k, x, sign_of=None if c.get('nonneg') else 'x', sign_off=off)
    b = D.bias('b', real)
    if real < cout:
        wt = torch.cat([wt, torch.zeros((cout - real, cin, k, k), dtype=torch.float64)], 0)
        b = torch.cat([b, torch.zeros(cout - real, dtype=torch.float64)])
    s = R.conv('c0', 0, x, wt, stride, k // 2)
    res = D.res('res', s.shape) if c.get('res', 'none') != 'none' else None
    R.store('y', 0, [s], b, res, c.get('act', 'relu'), c.get('res', 'none') == 'after', c.get('relu_from', 0), True, ('c0',))


def ref_block(D, R, c):
    """BasicBlock (k_bblock2_32 / _48 / _96 and the two-launch form): t = bf16(relu(conv1(x) + b1)) -- the kernels' LDS copy of the
    intermediate --, y = relu(conv2(t) + b2 + x)."""
    ch = c['c']
    x = D.head('x', (c['n'], ch, c['h'], c['w']), 0, nonneg=c.get('nonneg', False))
    sign = None if c.get('nonneg') else 'x'
    s1 = R.conv('c0', 0, x, D.weight('w1', 0, ch, ch, 3, x, sign_of=sign), 1, 1)
    t = R.store('t', 0, [s1], D.bias('b1', ch), None, 'relu', final=False, conv_names=('c0',))
    s2 = R.conv('c1', 1, t, D.weight('w2', 1, ch, ch, 3, t), 1, 1)
    R.store('y', 1, [s2], D.bias('b2', ch), x, 'relu', final=True, conv_names=('c1',))


def _tail(D, R, c, y2, st, sign):
    """X = relu(conv3(y2) [+ downsample(x0), kept in fp32] [+ res]); Y = relu(conv1_next(bf16(X))) (k_pw2, and the tail of k_bneck)."""
    n, h, w = c['n'], c['h'], c['w']
    nonneg = c['family'] == 'bneck'
    sums = [R.conv('c%d' % st, st, y2, D.weight('w3', st, 256, 64, 1, y2, sign_of=sign), 1, 0)]
    b, names = D.bias('b3', 256), ['c%d' % st]
    if c['first']:
        x0 = D.head('x0', (n, 64, h, w), st, nonneg=nonneg)
        sums.append(R.conv('down', -1, x0, D.weight('wd', st, 256, 64, 1, x0, sign_of=None if nonneg else 'x0'), 1, 0))
        b = b + D.bias('bd', 256)
        names.append('down')
    res = D.res('res', (n, 256, h, w), nonneg=nonneg) if c['res'] else None
    X = R.store('X', st, sums, b, res, 'relu', final=True, conv_names=names, feeds=c['second'])
    if c['second']:
        s = R.conv('c%d' % (st + 1), st + 1, X, D.weight('w1n', st + 1, 64, 256, 1, X), 1, 0)
        R.store('Y', st + 1, [s], D.bias('b1n', 64), None, 'relu', final=True, conv_names=('c%d' % (st + 1),))


def ref_pw2(D, R, c):
    y2 = D.head('y2', (c['n'], 64, c['h'], c['w']), 0)
    _tail(D, R, c, y2, 0, 'y2')


def ref_bneck(D, R, c):
    """k_bneck: t2 = bf16(relu(conv2 3x3 (y1) + b2)), then the pointwise tail; every input is a post-ReLU tensor."""
    y1 = D.head('y1', (c['n'], 64, c['h'], c['w']), 0, nonneg=True)
    s = R.conv('c0', 0, y1, D.weight('w2', 0, 64, 64, 3, y1), 1, 1)
    t2 = R.store('t2', 0, [s], D.bias('b2', 64), None, 'relu', final=False, conv_names=('c0',))
    _tail(D, R, c, t2, 1, None)


def ref_stem(D, R, c):
    """k_stem_fused / the two-launch stem: a = bf16(relu(conv1 3x3 s2 (x))), x0 = bf16(relu(conv2 3x3 s2 (a))), y1 = relu(pw(x0)).
    x has 8 channels of which 3 are real (the others zero, and conv1's filters are zero-padded by PackedConv's pad_cin_to)."""
    n, h, w = c['n'], c['h'], c['w']
    x = D.head('x', (n, 3, h, w), 0)
    s = R.conv('c0', 0, x, D.weight('w1', 0, 64, 3, 3, x, sign_of='x'), 2, 1)
    a = R.store('a', 0, [s], D.bias('b1', 64), None, 'relu', final=False, conv_names=('c0',))
    s = R.conv('c1', 1, a, D.weight('w2', 1, 64, 64, 3, a), 2, 1)
    x0 = R.store('x0', 1, [s], D.bias('b2', 64), None, 'relu', final=True, conv_names=('c1',), feeds=True)
    s = R.conv('c2', 2, x0, D.weight('wp', 2, 64, 64, 1, x0), 1, 0)
    R.store('y1', 2, [s], D.bias('bp', 64), None, 'relu', final=True, conv_names=('c2',))


def ref_fuse(D, R, c):
    """k_fuse_sum: y = relu(base + plain terms + sum_s up_s(bf16(conv1x1_s(src_s) + b_s))) -- every product is rounded to bf16 before
    it is up-sampled and summed, as the separate 1x1 launches it replaces store theirs."""
    n, h, w, ch = c['n'], c['h'], c['w'], c['c']
    base = D.res('base', (n, ch, h, w))
    total = base
    for i in range(c['nplain']):
        total = total + D.res('plain%d' % i, (n, ch, h, w))
    for j, sh in enumerate(c['shifts']):
        src = D.head('src%d' % j, (n, ch << sh, h >> sh, w >> sh), 0)
        s = R.conv('c0' if j == 0 else 'src%d' % j, 0 if j == 0 else -1, src, D.weight('w%d' % j, 0, ch, ch << sh, 1, src, sign_of='src%d' % j), 1, 0)
        t = R.store('t%d' % j, 0 if j == 0 else -1, [s], D.bias('b%d' % j, ch), None, 'linear', final=False, conv_names=('c0' if j == 0 else 'src%d' % j,))
        total = total + up_nearest(t.to(torch.float64), sh)
    R._xw['sum'] = float(total.abs().max())                          # the sum of the terms: integers, exact below 2^24
    R.store('y', -1, [total], torch.zeros(ch, dtype=torch.float64), None, 'relu', final=True, conv_names=('sum',))


def ref_rstem(D, R, c):
    """k_resnet_stem: max-pool 3x3 s2 p1 of relu(conv 7x7 s2 p3 (x) + b), 3 real input channels of 8."""
    x = D.head('x', (c['n'], 3, c['h'], c['w']), 0)
    s = R.conv('c0', 0, x, D.weight('w', 0, 64, 3, 7, x, sign_of='x'), 2, 3)
    R.store('y', 0, [s], D.bias('b', 64), None, 'relu', final=True, conv_names=('c0',), post=lambda t: F.max_pool2d(t, 3, 2, 1))


def deconv_as_conv(x):
    """ConvTranspose2d(4, stride 2, padding 1) as a direct convolution: returns x with a zero between neighbouring samples; convolving
    it at stride 1, padding 2 with kernels (Cout, Cin, 4, 4) that are the transposed convolution's flipped ones (``deconv_weight``
    turns them back) gives the transposed convolution."""
    n, cin, h, w = x.shape
    up = torch.zeros((n, cin, 2 * h - 1, 2 * w - 1), dtype=torch.float64)
    up[:, :, ::2, ::2] = x
    return up


def deconv_weight(wd):
    """The (Cin, Cout, 4, 4) weight of the nn.ConvTranspose2d that deconv_as_conv's direct form computes."""
    return wd.flip(2, 3).permute(1, 0, 2, 3).contiguous()


def ref_deconv(D, R, c):
    """k_deconv4x4s2: act(ConvTranspose2d(Cin, Cout, 4, 2, 1)(x) + b).  Every output sums 4 of the 16 taps."""
    x = D.head('x', (c['n'], c['cin'], c['h'], c['w']), 0)
    wd = D.weight('w', 0, c['cout'], c['cin'], 4, x, sign_of='x')
    s = R.conv('c0', 0, deconv_as_conv(x), wd, 1, 2, tap=(1, 1))     # tap (1, 1) reads a real sample at the odd last row / column
    R.store('y', 0, [s], D.bias('b', c['cout']), None, c['act'], final=True, conv_names=('c0',))


REFS = dict(rstem=ref_rstem, deconv=ref_deconv, conv=ref_conv, block=ref_block, pw2=ref_pw2, bneck=ref_bneck, stem=ref_stem, fuse=ref_fuse)

# K of every stage of a family's chain (what the densities are scaled by)
STAGE_K = dict(
    rstem=lambda c: [147],
    deconv=lambda c: [4 * c['cin']],
    conv=lambda c: [c['cin'] * c['k'] ** 2],
    block=lambda c: [9 * c['c'], 9 * c['c']],
    pw2=lambda c: [64 * (2 if c['first'] else 1)] + ([256] if c['second'] else []),
    bneck=lambda c: [576, 64 * (2 if c['first'] else 1)] + ([256] if c['second'] else []),
    stem=lambda c: [27, 576, 64],
    fuse=lambda c: [sum(c['c'] << s for s in c['shifts'])],
)


def evaluate(case, regime, fault=None, stage=0, base=None, data=None):
    """-> (Data, Run) of one case in one regime; a faulted evaluation passes the clean one's Data and Run."""
    D = data or Data(case, regime)
    R = Run(fault, stage, base)
    REFS[case['family']](D, R, case)
    return D, R


def applicable_faults(case):
    """(fault, stage) pairs a case must discriminate: a-d per stage; e where a stage has a residual; g for chains; h with relu_from."""
    fam = case['family']
    nst = len(STAGE_K[fam](case))
    out = []
    for st in range(nst):
        out += [('a', st), ('b', st), ('c', st)]
    if fam in ('rstem', 'deconv'):
        if fam == 'rstem' or case['act'] != 'linear':
            out.append(('d', 0))
    elif fam == 'conv':
        if case.get('act', 'relu') != 'linear':
            out.append(('d', 0))
        if case.get('res', 'none') != 'none':
            out.append(('e', 0))
        if case.get('relu_from', 0) > 0:
            out.append(('h', 0))
    elif fam == 'fuse':
        out += [('g2', 0), ('g0', 0)]
    else:
        out += [('d', st) for st in range(nst)]
        if fam == 'block':
            out.append(('e', 1))
        if fam in ('pw2', 'bneck') and case['res']:
            out.append(('e', nst - (2 if case['second'] else 1)))
        if fam != 'pw2' or case['second']:            # something is stored and read again
            out += [('g2', 0), ('g0', 0)]
    out.append(('f', 0))
    return out


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
def _conv(id, n, h, w, cin, cout, k=3, stride=1, res='none', act='relu', launch='hip', **kw):
    return dict(id=id, family='conv', n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, res=res, act=act, launch=launch, **kw)


# pam_conv_last_kernel() codes (include/pam.h): a variant's `kernel` is the code (or codes) the launch must report
K_IGEMM, K_3X3, K_3X3S, K_GS, K_STEM = 0, 1, 2, 3, 4

ALL_TILES = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]


def tile_refused(c, tile):
    """(case, tile) pairs pam_conv2d_nhwc_bf16_ex refuses with PAM_E_ARG before launching (tests/test_gpu_conv.py checks the refusals)."""
    use_res, cout = c.get('res', 'none') != 'none', c['cout']
    if tile in (10, 11, 12):
        return bool(use_res or cout % 48)
    if tile == 9:
        return bool(use_res or cout % 96)
    nb = cout // (48 if cout % 48 == 0 else 64)
    return bool((tile in (1, 3) and nb % 2) or (tile in (5, 7) and nb % 3) or (tile == 6 and nb % 4))


def _tiles(c):
    return [dict(tile_cfg=t) for t in ALL_TILES if not tile_refused(c, t)]


CONV_CASES = [
    # 3x3 stride 1
    _conv('c3-48-ragged', 2, 25, 18, 48, 48, res='before'),
    _conv('c3-96-tiny', 1, 7, 5, 96, 96),
    _conv('c3-48-96-wide', 3, 31, 72, 48, 96),
    _conv('c3-384-192-lin', 2, 9, 12, 384, 192, res='before', act='linear'),
    _conv('c3-64', 2, 24, 18, 64, 64, res='before'),
    # stride 2
    _conv('s2-8-64', 2, 13, 11, 8, 64, stride=2),
    _conv('s2-64', 2, 20, 16, 64, 64, stride=2),
    _conv('s2-48-96-lin', 2, 16, 12, 48, 96, stride=2, res='before', act='linear'),
    _conv('s2-48-144', 2, 20, 16, 48, 144, stride=2),
    _conv('s2-96-288', 2, 13, 11, 96, 288, stride=2),
    # 1x1
    _conv('p-64-256', 2, 16, 12, 64, 256, k=1, res='before'),
    _conv('p-256-64', 2, 16, 12, 256, 64, k=1),
    _conv('p-384-48-lin', 2, 12, 8, 384, 48, k=1, act='linear'),
    # streamed k_conv3x3s
    _conv('cs-192', 3, 16, 12, 192, 192),
    _conv('cs-192-64-lin', 2, 40, 6, 192, 64, res='before', act='linear'),
    _conv('cs-384-128-ragged', 2, 25, 18, 384, 128, res='before'),
    _conv('cs-192-small', 5, 3, 3, 192, 192, res='before'),
]
for _c in CONV_CASES:
    _c['variants'] = _tiles(_c)
    if _c['id'].startswith('cs-'):
        _c['variants'][0]['kernel'] = K_3X3S       # the library's own choice (tile_cfg -1) for these shapes is the streamed kernel

CONV_CASES += [
    # 96 -> 96 with c96_slab 0 (k_conv3x3) and 48 (k_conv3x3s)
    _conv('c96-ragged', 2, 25, 18, 96, 96, res='before', variants=[dict(tile_cfg=-1, c96_slab=0, kernel=K_3X3), dict(tile_cfg=-1, c96_slab=48, kernel=K_3X3S)]),
    _conv('c96-tiny', 3, 7, 5, 96, 96, res='before', variants=[dict(tile_cfg=-1, c96_slab=0, kernel=K_3X3), dict(tile_cfg=-1, c96_slab=48, kernel=K_3X3S)]),
    _conv('slab32-384', 5, 6, 5, 384, 384, res='before', variants=[dict(tile_cfg=-1, slab32=False), dict(tile_cfg=-1, slab32=True, kernel=K_3X3S, image=('s32', 32))]),
    _conv('slab32-384-lin', 5, 6, 5, 384, 384, act='linear', variants=[dict(tile_cfg=-1, slab32=True, kernel=K_3X3S, image=('s32', 32))]),
    # 540 tiles on 512 persistent workgroups
    _conv('c3-48-rounds', 180, 25, 18, 48, 48, res='before', variants=[dict(tile_cfg=-1)]),
    # channel-sliced inputs and a partial ReLU (test_channel_sliced_operands_and_partial_relu)
    _conv('slice-48-192', 2, 24, 18, 48, 192, stride=2, wide=192, off=96, launch='plain', variants=[{}]),
    _conv('slice-48-48', 2, 24, 18, 48, 48, stride=2, wide=192, off=144, launch='plain', variants=[{}]),
    _conv('slice-96-144-rf96', 2, 24, 18, 96, 144, stride=2, wide=192, off=0, relu_from=96, launch='plain', variants=[{}]),
    _conv('slice-96-96-p-rf48', 2, 24, 18, 96, 96, k=1, wide=192, off=48, relu_from=48, launch='plain', variants=[{}]),
]

DARKNET_CASES = [
    _conv('dk-64-128', 2, 26, 26, 64, 128, act='leaky', res='after', launch='plain', variants=[{}]),
    _conv('dk-32-64', 1, 52, 52, 32, 64, act='leaky', res='after', launch='plain', variants=[{}]),
    _conv('dk-512-1024', 2, 13, 13, 512, 1024, act='leaky', res='after', launch='plain', variants=[{}]),
    _conv('dk-first-s1', 2, 31, 23, 8, 32, act='leaky', launch='plain', variants=[dict(kernel=K_STEM)]),
    _conv('dk-first-s2', 2, 31, 23, 8, 32, stride=2, act='relu', launch='plain', variants=[dict(kernel=K_STEM)]),
    _conv('dk-head-255', 2, 13, 13, 64, 256, k=1, act='linear', cout_real=255, launch='plain', variants=[{}]),
    _conv('dk-48-before', 2, 24, 18, 48, 48, act='leaky', res='before', launch='plain', variants=[{}]),
    _conv('dk-384-256', 2, 13, 13, 384, 256, act='leaky', launch='hip',
          variants=[dict(tile_cfg=-1, kernel=(K_IGEMM, K_3X3, K_GS))]),     # leaky: not k_conv3x3s, which this shape takes with ReLU
]

DOWN48_CASES = [
    _conv('d48-odd', 2, 31, 23, 48, 96, stride=2, wide=144, off=48, launch='down48', variants=[dict(d48_tile=(5, 4, 1))]),
    _conv('d48-tiny-res', 3, 7, 5, 48, 48, stride=2, res='before', launch='down48', variants=[dict(d48_tile=None)]),
    _conv('d48-384', 2, 48, 36, 48, 384, stride=2, act='linear', wide=96, off=24, launch='down48', variants=[dict(d48_tile=(12, 6, 2))]),
    _conv('d48-rf48-res', 2, 96, 72, 48, 96, stride=2, res='before', relu_from=48, launch='down48', variants=[dict(d48_tile=None)]),
]

DOWN_S_CASES = [
    _conv('ds-odd', 2, 31, 23, 96, 192, stride=2, launch='down_s', variants=[{}]),
    _conv('ds-tiny-rf64', 3, 7, 5, 192, 192, stride=2, relu_from=64, launch='down_s', variants=[{}]),
    _conv('ds-256x192', 2, 32, 24, 96, 192, stride=2, act='linear', launch='down_s', variants=[{}]),
    _conv('ds-288-rf192', 2, 24, 18, 96, 288, stride=2, relu_from=192, launch='down_s', variants=[{}]),
    _conv('ds-slice', 2, 24, 18, 96, 384, stride=2, act='linear', wide=288, off=96, launch='down_s', variants=[{}]),
    _conv('ds-192-384', 3, 24, 18, 192, 384, stride=2, launch='down_s', variants=[{}]),
]

PW1_CASES = [
    _conv('pw1-ragged', 3, 7, 11, 64, 64, k=1, launch='pw1', variants=[{}]),
    _conv('pw1-tiny', 1, 5, 3, 64, 64, k=1, launch='pw1', variants=[{}]),
    _conv('pw1-96x72', 2, 96, 72, 64, 64, k=1, launch='pw1', variants=[{}]),
]


def _block(id, c, n, h, w, tiles, **kw):
    return dict(id=id, family='block', c=c, n=n, h=h, w=w, variants=[dict(tile=t) for t in tiles], **kw)


BLOCK_CASES = [
    _block('b48-odd', 48, 2, 33, 41, [(11, 13)]),
    _block('b48-tiny', 48, 3, 7, 5, [None]),
    _block('b48-ragged-rows', 48, 2, 50, 72, [(16, 36)]),
    _block('b48-ragged-cols', 48, 2, 96, 70, [(16, 36)]),
    _block('b48-small-tiles', 48, 3, 96, 72, [(8, 18)]),
    _block('b96-odd', 96, 2, 21, 29, [(7, 11)]),
    _block('b96-tiny', 96, 3, 7, 5, [None]),
    _block('b96-ragged-rows', 96, 2, 27, 36, [(6, 36)]),
    _block('b96-ragged-cols', 96, 2, 48, 34, [(6, 18)]),
    _block('b96-kpb2', 96, 2, 40, 60, [(4, 60)]),
    _block('b96-widest', 96, 2, 6, 124, [(1, 124)]),
    _block('b32', 32, 1, 64, 48, [None, (5, 7), (10, 44), (3, 48), (1, 1), (17, 5)], nonneg=True),
]

FUSE_CASES = [
    dict(id='fs-48-ragged', family='fuse', n=2, h=40, w=24, c=48, shifts=(1, 2, 3), nplain=0, variants=[dict(tile=(2, 2))]),
    dict(id='fs-48-full', family='fuse', n=3, h=96, w=72, c=48, shifts=(1, 2, 3), nplain=0, variants=[dict(tile=(1, 1))]),
    dict(id='fs-96', family='fuse', n=2, h=48, w=36, c=96, shifts=(1, 2), nplain=1, variants=[dict(tile=(0, 0))]),
    dict(id='fs-192', family='fuse', n=2, h=24, w=18, c=192, shifts=(1,), nplain=2, variants=[dict(tile=(0, 0))]),
    dict(id='fs-96-lone', family='fuse', n=2, h=24, w=16, c=96, shifts=(2,), nplain=2, variants=[dict(tile=(0, 0))]),
]

PW2_CASES = [dict(id='pw2-%s%s-%dx%dx%d' % ('d' if first else ('r' if res else 'n'), '2' if second else '', n, h, w), family='pw2',
                  n=n, h=h, w=w, first=first, res=res, second=second, variants=[dict(tile_cfg=t) for t in (0, 1, 2, 3)])
             for (n, h, w) in ((3, 7, 11), (1, 5, 3)) for (first, res) in ((False, True), (True, False), (False, False))
             for second in (True, False)]

BNECK_CASES = [dict(id='bn-%dx%dx%d-%s%s' % (n, h, w, 'first' if first else 'later', '-next' if second else ''), family='bneck',
                    n=n, h=h, w=w, first=first, res=not first, second=second, variants=[{}])
               for (n, h, w) in ((2, 50, 37), (2, 7, 5), (1, 2, 3), (3, 64, 48)) for first in (True, False) for second in (True, False)]

STEM_CASES = [dict(id='stem-%dx%dx%d' % s, family='stem', n=s[0], h=s[1], w=s[2], variants=[{}])
              for s in ((1, 384, 288), (3, 256, 192), (2, 100, 60), (2, 67, 45), (1, 4, 4))]

RESNET_CASES = [
    dict(id='rstem-256x192', family='rstem', n=1, h=256, w=192, variants=[{}]),
    dict(id='rstem-384x288', family='rstem', n=1, h=384, w=288, variants=[{}]),
    dict(id='dc-256', family='deconv', n=1, h=16, w=12, cin=256, cout=256, act='relu', variants=[{}]),
    dict(id='dc-256-lin', family='deconv', n=1, h=16, w=12, cin=256, cout=256, act='linear', variants=[{}]),
    dict(id='dc-2048', family='deconv', n=1, h=8, w=6, cin=2048, cout=256, act='relu', variants=[{}]),
]

CASES = RESNET_CASES + CONV_CASES + DARKNET_CASES + DOWN48_CASES + DOWN_S_CASES + PW1_CASES + BLOCK_CASES + FUSE_CASES + PW2_CASES + BNECK_CASES + STEM_CASES
assert len({c['id'] for c in CASES}) == len(CASES)


def gflop(case):
    """Reference work of one regime of a case (2 flops per product)."""
    fam = case['family']
    n, h, w = case['n'], case['h'], case['w']
    if fam == 'conv':
        ho, wo = out_hw(h, w, case['k'], case['stride'])
        return 2e-9 * n * ho * wo * case['cout'] * case['cin'] * case['k'] ** 2
    if fam == 'rstem':
        return 2e-9 * n * (h // 2) * (w // 2) * 64 * 147
    if fam == 'deconv':
        return 2e-9 * n * 4 * h * w * case['cout'] * 16 * case['cin']            # the direct form multiplies the stuffed zeros too
    if fam == 'block':
        return 2e-9 * 2 * n * h * w * 9 * case['c'] ** 2
    if fam == 'fuse':
        return 2e-9 * sum(n * (h >> s) * (w >> s) * case['c'] * (case['c'] << s) for s in case['shifts'])
    if fam == 'stem':
        h1, w1 = out_hw(h, w, 3, 2)
        h2, w2 = out_hw(h1, w1, 3, 2)
        return 2e-9 * n * (h1 * w1 * 64 * 27 + h2 * w2 * 64 * (576 + 64))
    s = 2 if case['first'] else 1
    return 2e-9 * n * h * w * ((64 * 576 if fam == 'bneck' else 0) + 256 * 64 * s + (64 * 256 if case['second'] else 0))
