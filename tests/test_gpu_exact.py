"""GPU: every MFMA kernel of the conv stack pinned to exact bits.  The operands are small integers (tests/exact_ref.py), so every
product and partial sum is exact in fp32 in any order and the only inexact step is the bf16 store; the reference is a float64
unfold-and-matmul convolution on the CPU that shares no code with the kernels, the packing or torch's GPU convolutions.  The one
assertion is ``torch.equal(y.float(), ref)`` -- no tolerance anywhere in this file.  Every kernel is launched through the engine entry
point it already has, with the ``Packed*`` classes taking ``nn.Conv2d`` modules that hold the integer weights and biases.

A test is one case of exact_ref.CASES: all its regimes (``sharp-i`` per stage of the chain, then ``rounding``) times all its launch
variants (tile codes, slab widths, item sizes).  A mismatch reports the number of differing elements, the first (n, c, y, x) with got
and want, and the sets of c // 16, rows and columns that differ -- which tile edge or slab is wrong.  One ``EXACT {json}`` line per
case and regime carries the sharp share, max |v| and the tie count of every compared output.

Memory (tests/guarded_mem.py).  Every output of every launch is carved from a GuardArena: it starts out as the sentinel, a positive bf16
NaN, and lies between sentinel bands; every input, residual and intermediate handed to a kernel sits at a 256-byte-aligned address
between two poison bands.  A variant is packed and its inputs are built once; it is then launched once per fill of guarded_mem.FILLS
(NaN, +1.7e38, -1.7e38: the input bands refilled in place, the arena reset), and after each launch and synchronise a damaged band or an
output element that still holds the sentinel fails the variant like a differing value does.  The CPU reference is still evaluated once
per regime.  The EXACT line carries ``fills``, ``band_violations`` and ``unwritten``; a mismatch says how many of its elements were
never written.

Measured (the CPU reference's figures, as the GPU run's EXACT lines repeat them; tests/test_exact_ref.py asserts their bounds; MI355X run:
102 cases, 599 launches x 3 fills = 1797, 0 differing, 0 damaged bands, 0 unwritten elements; 8.6 s for the file where the unguarded
single-fill form took 6.8 s), min .. max over the cases of a family:
  family (cases, launches)     sharp share in the sharp regimes           ties per case, max |v| in `rounding`
  conv, all tiles (23, 284)    0.47 .. 0.51 act, 0.986 .. 0.993 linear    513 .. 996912, 517 .. 4163
  Darknet / sliced (11, 22)    0.44 .. 0.83 act, 0.965 .. 0.965 linear    2116 .. 39069, 572 .. 5416
  k_down48 (4, 8)              0.49 .. 0.74 act, 0.987 .. 0.987 linear    301 .. 159771, 539 .. 625
  k_down_s (6, 12)             0.50 .. 0.83 act, 0.991 .. 0.991 linear    747 .. 20535, 1100 .. 2138
  k_pw1 (3, 6)                 0.45 .. 0.48                               247 .. 140796, 705 .. 798
  k_bblock2_48 (5, 15)         0.42 .. 0.56                               618 .. 120729, 1614 .. 3219
  k_bblock2_96 (6, 18)         0.39 .. 0.54                               920 .. 33660, 4153 .. 7833
  k_bblock2_32 (1, 18)         0.49 .. 0.60                               6610 .. 6610, 3362 .. 3362
  k_fuse_sum (5, 10)           0.47 .. 0.50                               9197 .. 148111, 514 .. 880
  k_pw2 (12, 120)              0.45 .. 0.53                               399 .. 15220, 631 .. 3354
  k_bneck (16, 56)             0.37 .. 0.61                               176 .. 226638, 1589 .. 11814
  stems (5, 20)                0.35 .. 0.54                               15 .. 91090, 1600 .. 12606
  k_resnet_stem (2, 4)         0.99 .. 1.00                               35675 .. 68969, 768 .. 829
  k_deconv4x4s2 (3, 6)         0.49 .. 0.50 act, 0.991 .. 0.991 linear    457 .. 29521, 1309 .. 9404
Every case meets the rounding conditions (a quarter of each output's sums past 256, 100 ties) but stem-1x4x4, whose 128 outputs hold
fewer ties; short sums (K <= 288) get there with activations of up to 96 in magnitude (exact_ref.Data._scale)."""
import json

import pytest
import torch
import torch.nn as nn

import pam
import exact_ref as E
import guarded_mem as G

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
IDS = [c['id'] for c in E.CASES]


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------------
ARENA_BYTES = 64 << 20       # the outputs of ONE launch with their bands (the largest: c3-48-rounds, 7.8 MB; the stem's five, 6.2 MB)
_arena = []
POISON = []                  # the handles of the inputs built since the last clear: their bands are refilled per fill


def arena():
    """The GuardArena every engine of this file carves its outputs from (one per session, reset before every launch)."""
    if not _arena:
        _arena.append(G.GuardArena(DEV, ARENA_BYTES))
    return _arena[0]


def cl(t):
    """An integer-valued float64 NCHW tensor as the kernels read it: bf16 (exact: |t| <= 256 or already a bf16 value), channels-last,
    256-byte aligned between two bands of G.GUARD poison elements (guarded_mem.poisoned)."""
    b = t.to(torch.bfloat16)
    assert torch.equal(b.double(), t.double())
    view, handle = G.poisoned(b.to(DEV).contiguous(memory_format=torch.channels_last), G.FILLS[0])
    POISON.append(handle)
    return view


def module(w, b, stride=1):
    """nn.Conv2d holding the integer weights (Cout, Cin, k, k) and biases."""
    cout, cin, k, _ = w.shape
    m = nn.Conv2d(cin, cout, k, stride, k // 2, bias=True)
    with torch.no_grad():
        m.weight.copy_(w.float()); m.bias.copy_(b.float())
    return m


def hip_engine(**attrs):
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipHRNet.__new__(hrnet_hip.HipHRNet)
    e.lib = _lib.load(); e.device = DEV; e.tile_cfg = -1; e._keep = []; e.arena = arena()
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


def plain_engine():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.ConvEngine()
    e.lib = _lib.load(); e.device = DEV; e.arena = arena()
    return e


def mismatch(got, want):
    """None when got (bf16 device tensor) holds exactly `want` (float32 CPU tensor of bf16 values); else the report, which says how
    many of the differing elements still hold the arena's sentinel: never written, as opposed to a wrong value."""
    g = got.float().cpu()
    if tuple(g.shape) != tuple(want.shape):
        return 'shape %s, want %s' % (tuple(g.shape), tuple(want.shape))
    if torch.equal(g, want):
        return None
    bad = g != want
    idx = bad.nonzero()
    n, c, y, x = [int(v) for v in idx[0]]
    short = lambda v: sorted(set(int(i) for i in v))[:40]
    never = int(((got.view(torch.int16).cpu() == G.as_i16(G.SENTINEL)) & bad).sum())
    return ('%d of %d elements differ (%d of them still hold the sentinel: never written); first (n, c, y, x) = (%d, %d, %d, %d): got %r, '
            'want %r; c // 16 in %s; rows %s; columns %s'
            % (int(bad.sum()), bad.numel(), never, n, c, y, x, float(g[n, c, y, x]), float(want[n, c, y, x]),
               short(idx[:, 1] // 16), short(idx[:, 2]), short(idx[:, 3])))


# ---- one launcher per family: (case, data, variant) -> run, and run() -> {output name: device tensor} -----------------------------------
# A launcher packs the weights and builds the (poisoned) inputs ONCE; run() issues the launch, and is called once per fill of G.FILLS.
def launch_conv(c, D, v):
    from pam import hrnet_hip
    real = c.get('cout_real', c['cout'])
    conv = module(D.t['w'], D.t['b'], c['stride'])
    xw = cl(D.t['x'])
    off = c.get('off', 0)
    x = xw[:, off:off + c['cin']] if c.get('wide', c['cin']) != c['cin'] else xw
    res = cl(D.t['res']) if 'res' in D.t else None
    act, rf = c.get('act', 'relu'), c.get('relu_from', 0)
    kind = c['launch']
    if kind == 'pw1':
        assert act == 'relu'
        e, pw = plain_engine(), hrnet_hip.PackedPointwise64(conv, DEV)
        return lambda: dict(y=e.pointwise64(pw, x))
    op = hrnet_hip.PackedConv(conv, DEV, pad_cout_to=c['cout'] if real < c['cout'] else None)
    if kind == 'down48':
        e = hip_engine(d48_tile=v.get('d48_tile'))
        return lambda: dict(y=e.conv_down48(op, x, res=res, relu=act == 'relu', relu_from=rf))
    if kind == 'down_s':
        e = hip_engine()
        assert e.lib.pam_conv3x3s2_slab(c['h'], c['w'], c['cin'], c['cout']) in (48, 64)
        return lambda: dict(y=e.conv_down_s(op, x, relu=act == 'relu', relu_from=rf))
    if kind == 'plain':
        e = plain_engine()
    else:
        e = hip_engine(**{k: a for k, a in v.items() if k not in ('kernel', 'image')})
        e.down48 = e.tile_cfg == -1              # a stated tile keeps the strided 48-channel layers on the generic kernels

    def run():
        y = e.conv(op, x, res=res, relu=act, res_after_act=c.get('res') == 'after', relu_from=rf)
        if 'kernel' in v:                            # the case is named after a kernel: it must be the one that ran
            want = v['kernel'] if isinstance(v['kernel'], tuple) else (v['kernel'],)
            assert e.lib.pam_conv_last_kernel() in want, (c['id'], v, e.lib.pam_conv_last_kernel())
        if 'image' in v:
            assert v['image'] in op._images, (c['id'], v, list(op._images))
        return dict(y=y)
    return run


def launch_block(c, D, v):
    from pam import hrnet_hip
    op = hrnet_hip.PackedBlock(module(D.t['w1'], D.t['b1']), module(D.t['w2'], D.t['b2']), DEV)
    e, x = hip_engine(), cl(D.t['x'])
    return lambda: dict(y=e.basic_block2(op, x, v['tile']))


def launch_fuse(c, D, v):
    from pam import hrnet_hip
    ch, n, h, w = c['c'], c['n'], c['h'], c['w']
    convs = [module(D.t['w%d' % j], D.t['b%d' % j]) for j in range(len(c['shifts']))]
    op = hrnet_hip.PackedUp(convs, c['shifts'], DEV)
    # the plain terms are channel slices of a wider tensor, as the merged strided heads hand them over
    wide = torch.zeros((n, 2 * ch + 16, h, w), dtype=torch.float64)
    for i in range(c['nplain']):
        wide[:, 8 + i * ch:8 + (i + 1) * ch] = D.t['plain%d' % i]
    wide = cl(wide)
    plain = [wide[:, 8 + i * ch:8 + (i + 1) * ch] for i in range(c['nplain'])]
    srcs = [cl(D.t['src%d' % j]) for j in range(len(c['shifts']))]
    e, base = hip_engine(), cl(D.t['base'])
    return lambda: dict(y=e.fuse_sum(op, base, plain, srcs, relu=True, tile=v['tile']))


def _tail_op(c, D):
    from pam import hrnet_hip
    conv3 = module(D.t['w3'], D.t['b3'])
    down = module(D.t['wd'], D.t['bd']) if c['first'] else None
    conv1 = module(D.t['w1n'], D.t['b1n']) if c['second'] else None
    return hrnet_hip.PackedTail(conv3, down, conv1, DEV)


def launch_pw2(c, D, v):
    e, op = plain_engine(), _tail_op(c, D)
    y2, x0, res = cl(D.t['y2']), cl(D.t['x0']) if c['first'] else None, cl(D.t['res']) if c['res'] else None

    def run():
        X, Y = e.bottleneck_tail(op, y2, x0, res, v['tile_cfg'])
        return dict(X=X, Y=Y) if c['second'] else dict(X=X)
    return run


def launch_bneck(c, D, v):
    from pam import hrnet_hip
    op = hrnet_hip.PackedBneck(module(D.t['w2'], D.t['b2']), _tail_op(c, D), DEV)
    e = hip_engine(c96_slab=48)
    y1, res, x0 = cl(D.t['y1']), cl(D.t['res']) if c['res'] else None, cl(D.t['x0']) if c['first'] else None

    def run():
        X, Y = e.bottleneck_fused(op, y1, res, x0)
        return dict(X=X, Y=Y) if c['second'] else dict(X=X)
    return run


def launch_stem(c, D, v):
    """The fused stem AND the three launches it replaces, each against the reference (and so against each other); the intermediates
    of the three-launch form come from the arena too, so they are banded inputs of the launch that reads them."""
    from pam import hrnet_hip
    c1, c2, pw = module(D.t['w1'], D.t['b1'], 2), module(D.t['w2'], D.t['b2'], 2), module(D.t['wp'], D.t['bp'])
    P1, P2, Pp = hrnet_hip.PackedConv(c1, DEV, pad_cin_to=8), hrnet_hip.PackedConv(c2, DEV), hrnet_hip.PackedPointwise64(pw, DEV)
    op = hrnet_hip.PackedStem(P1, c2, Pp, DEV)
    x8 = torch.zeros((c['n'], 8, c['h'], c['w']), dtype=torch.float64)
    x8[:, :3] = D.t['x']
    x8 = cl(x8)
    e = hip_engine()

    def run():
        x0, y1 = e.stem_fused(op, x8)
        a = e.conv(P1, x8, relu=True)
        b = e.conv(P2, a, relu=True)
        return {'x0': x0, 'y1': y1, 'a': a, 'x0 (two launches)': b, 'y1 (two launches)': e.pointwise64(Pp, b)}
    return run


def resnet_engine():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipPoseResNet.__new__(hrnet_hip.HipPoseResNet)
    e.lib = _lib.load(); e.device = DEV; e.count = None; e._keep = []; e.arena = arena()
    return e


def launch_rstem(c, D, v):
    from pam import hrnet_hip
    op = hrnet_hip.PackedResNetStem(module(D.t['w'], D.t['b'], 2), DEV)
    x8 = torch.zeros((c['n'], 8, c['h'], c['w']), dtype=torch.float64)
    x8[:, :3] = D.t['x']
    e, x8 = resnet_engine(), cl(x8)
    return lambda: dict(y=e.resnet_stem(op, x8))


def launch_deconv(c, D, v):
    from pam import hrnet_hip
    ct = nn.ConvTranspose2d(c['cin'], c['cout'], 4, 2, 1, bias=True)
    with torch.no_grad():
        ct.weight.copy_(E.deconv_weight(D.t['w']).float()); ct.bias.copy_(D.t['b'].float())
    e, op, x = resnet_engine(), hrnet_hip.PackedDeconv(ct, DEV), cl(D.t['x'])
    return lambda: dict(y=e.deconv(op, x, relu=c['act'] == 'relu'))


LAUNCH = dict(rstem=launch_rstem, deconv=launch_deconv, conv=launch_conv, block=launch_block, fuse=launch_fuse, pw2=launch_pw2, bneck=launch_bneck, stem=launch_stem)


@pytest.mark.parametrize('case', E.CASES, ids=IDS)
def test_kernel_reproduces_the_exact_reference(case):
    from pam import _lib
    failures = []
    ar = arena()
    for regime in E.regimes(case):
        D, R = E.evaluate(case, regime)
        assert all(b < E.LIMIT for b in R.bound.values())
        stats = {n: dict(sharp=round(o['sharp'], 4), vmax=o['vmax'], ties=o['ties']) for n, o in R.outs.items()}
        nbad = nband = nunwritten = 0
        for v in case['variants']:
            del POISON[:]
            run = None
            for fill in G.FILLS:
                tag = '%s %s %s fill %#06x' % (case['id'], regime, v, fill)
                try:
                    if run is None:
                        run = LAUNCH[case['family']](case, D, v)        # weights packed and inputs built once per variant
                    for hd in POISON:
                        hd.refill(fill)
                    ar.reset()
                    outs = run()
                    torch.cuda.synchronize()
                except _lib.PamError as err:           # the library refused the launch: a failure of this variant, nothing ran
                    nbad += 1
                    failures.append('%s: %s' % (tag, err))
                    break
                except RuntimeError as err:
                    if not any(word in str(err) for word in ('HIP', 'hip', 'CUDA', 'illegal memory access')):
                        raise                          # a plain torch error (shape, stride, ...): this test fails, the others run
                    # a HIP error: nothing more is started on this device
                    pytest.exit('GPU error in %s: %s' % (tag, err), returncode=3)
                lo, hi = ar.buf.data_ptr(), ar.buf.data_ptr() + 2 * ar.buf.numel()
                assert all(lo <= t.data_ptr() < hi for t in outs.values()) and len(ar.allocs) >= len(outs), tag
                damaged, never = ar.violations(), sum(ar.unwritten())
                if damaged or never:                   # a write outside an output / an element no launch wrote: a failure of this variant
                    nband += len(damaged)
                    nunwritten += never
                    failures.append('%s: %s' % (tag, ar.report()))
                for name, got in outs.items():
                    why = mismatch(got, R.vals[name.split(' (')[0]])
                    if why is not None:
                        nbad += 1
                        failures.append('%s %s: %s' % (tag, name, why))
        print('EXACT ' + json.dumps(dict(case=case['id'], family=case['family'], regime=regime, variants=len(case['variants']),
                                         fills=len(G.FILLS), mismatching_launches=nbad, band_violations=nband, unwritten=nunwritten,
                                         outputs=stats)))
    del POISON[:]
    assert not failures, '\n'.join(failures)
