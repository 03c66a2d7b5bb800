"""GPU: the conv stack at the sizes where its 32-bit address arithmetic ends (the frontier table; the CPU side is
tests/test_conv_frontier.py).  Four kinds of case:

  * just below a frontier -- the largest N an entry point accepts, the operand within one image of its frontier: the output must be
    exact.  A guard that is one image too generous fails here.  The plan's families, and the fused entry points (basic block, pointwise,
    bottleneck tail and fused bottleneck, fused stem, ResNet stem, deconvolution), each followed by the refusal one image further.
  * an operand above 2^31 and above 2^32 bytes, for every operand the table says is addressed beyond them (64-bit pointers): the
    implicit GEMM's and k_conv_gs's output, k_conv3x3s's input, the stride-2 kernels' inputs, the tensors of k_upsample_add, k_route,
    k_maxpool, k_upsample_concat, k_spp and k_fuse_sum; and the un-fused
    stem's second convolution at 607 crops, which the executor issues as two slices of N.
  * refusals -- a call on its frontier, every tensor really allocated at that size and every output filled with the sentinel of
    tests/guarded_mem.py: PAM_E_ARG, and the outputs still hold the sentinel everywhere.
  * the network: HipHRNet's stem + layer1 at 607 crops of 384 x 288 (the first count that is sliced) and at 606 (one pass, every fused
    kernel at the largest batch it accepts) against the fp32 module, with the metrics and TOL['head'] of tests/test_gpu_hrnet_modules.py.

Data: the integer-valued operands of tests/exact_ref.py (activations and residuals in [-3, 3], weights in {-1, 0, 1}, biases in [-8, 8]),
drawn on the device because a 4 GiB tensor cannot wait for a CPU generator; every sum stays far below 2^24, so the right answer is unique
and every comparison is bit for bit over EVERY output element.  The 16 bytes at byte 2^31 of every input and residual that reaches them
are non-zero: a padding tap formed as the offset 2^31 then reads eight non-zero values.  The reference is exact_ref.conv_direct (float64
unfold + matmul, on the device) in slices of at most 32 images, or plain torch arithmetic for the sums and routes.

Why every launch here stays inside its allocations (read from the sources before the first run): loads through a buffer resource are
bounds-checked against num_records, which is the tensor's size below 2^32 bytes; every store and every other load goes through a 64-bit
pointer whose index is a pixel or piece count the entry point has checked to fit its int / unsigned.

Left out, each with its reason: the side below the -7 / -8 forms' output guard (2.5 / 3.7 TFLOP, see that test); k_conv3x3s with an
input above 2^32 bytes (2.5 TFLOP) or a residual near 2^32 (192 -> 384 at 24 x 18: 7.4 TFLOP); the refusals of pam_upsample_add and
pam_route_concat (2^31 pieces = 32 GiB per tensor), of pam_conv3x3s2_* (N Ho Wo = 2^31 output pixels, 2^30 items: hundreds of GiB) and
of pam_fuse_sum's plan (N H W = 2^31 pixels: 192 GiB at 48 channels) -- none can be really allocated inside the memory condition;
pam_basic_block2 at C = 32 / 96 (the guard is the one line shared with C = 48, which runs below and on it; C = 96 below it is 3.7 TFLOP).

Peak device memory in use after any test of this file (PAM_TEST_MEM=1): below 24 GiB.  Operands are at most 4 + 4 + 1 GiB (the residual
cases and the sums just above 2^32 bytes) plus one reference slice; the network cases keep every tensor of an eager 607-crop head until
the device is idle (about 16 GiB).  Every test frees what it made before the next."""
import pytest
import torch
import torch.nn as nn

import pam  # noqa: F401
import exact_ref as E
import guarded_mem as G

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENT = G.as_i16(G.SENTINEL)
K_IGEMM, K_3X3, K_3X3S, K_GS, K_STEM = range(5)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def ints(n, c, h, w, seed, lo=-3, hi=3):
    """(n, c, h, w) channels-last bf16 on the device, integers of [lo, hi] drawn there; the 16 bytes at byte 2^31 non-zero."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    flat = torch.empty(n * h * w * c, dtype=torch.bfloat16, device=DEV)
    for i in range(0, flat.numel(), 1 << 28):
        part = flat[i:i + (1 << 28)]
        part.copy_(torch.randint(lo, hi + 1, (part.numel(),), generator=g, device=DEV, dtype=torch.int8))
    if flat.numel() >= (1 << 30) + 8:
        seg = flat[1 << 30:(1 << 30) + 8]
        seg[seg == 0] = 3
        assert bool((seg != 0).all())
    return flat.view(n, h, w, c).permute(0, 3, 1, 2)


def sentinel(n, c, h, w):
    """An output that holds the sentinel everywhere."""
    return torch.full((n * h * w * c,), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16).view(n, h, w, c).permute(0, 3, 1, 2)


def untouched(t):
    return bool((t.permute(0, 2, 3, 1).reshape(-1).view(torch.int16) == SENT).all())


def weights(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, (cout, cin, k, k), generator=g).to(torch.float64), torch.randint(-8, 9, (cout,), generator=g).to(torch.float64))


def module(w, b, stride):
    cout, cin, k, _ = w.shape
    m = nn.Conv2d(cin, cout, k, stride, k // 2, bias=True)
    with torch.no_grad():
        m.weight.copy_(w.float()); m.bias.copy_(b.float())
    return m


def engine(**attrs):
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipHRNet.__new__(hrnet_hip.HipHRNet)
    e.lib = _lib.load(); e.device = DEV; e.tile_cfg = -1; e._keep = []; e.arena = None
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


def sentinel_outputs(e):
    """Every output e allocates from now on starts out as the sentinel; returns the list they are collected in."""
    made = []

    def new(n, c, h, w, device):
        made.append(sentinel(n, c, h, w))
        return made[-1]
    e._new = new
    return made


# ---- the reference, in slices ---------------------------------------------------------------------------------------------------------------
def differing(got, want_of, step):
    """Compares every element of got (N, C, H, W) with want_of(i, j) -> float32 values of images i .. j.  None, or the report."""
    total, first, where = 0, None, set()
    for i in range(0, got.shape[0], step):
        j = min(i + step, got.shape[0])
        bad = got[i:j].float() != want_of(i, j)
        nb = int(bad.sum())
        if nb:
            idx = bad.nonzero()
            if first is None:
                n, c, y, x = [int(v) for v in idx[0]]
                first = (i + n, c, y, x)
            total += nb
            where |= {(int(a) + i) for a in idx[:, 0].unique()[:8]}
            rows, cols = sorted(int(a) for a in idx[:, 2].unique()[:12]), sorted(int(a) for a in idx[:, 3].unique()[:12])
    if not total:
        return None
    return '%d of %d elements differ; first (n, c, y, x) = %s; images %s ...; rows %s; columns %s (last differing slice)' % (
        total, got.numel(), first, sorted(where)[:12], rows, cols)


def conv_differs(y, x, w, b, res, stride, act):
    """y against rne_bf16(act(conv(x) + b [+ res])) in float64, 32 images at a time (one image: 256 rows of a 1x1 layer at a time)."""
    k = w.shape[2]
    wd, bd = w.to(DEV), b.to(DEV).view(1, -1, 1, 1)

    def want(xs, rs):
        v = E.conv_direct(xs.double(), wd, stride, k // 2) + bd
        if rs is not None:
            v = v + rs.double()
        return E.rne_bf16(torch.relu(v) if act else v)
    if y.shape[0] == 1 and k == 1 and stride == 1:                 # the frontier inside one image: row blocks (a 1x1 layer is per pixel)
        rows_first = lambda t: t[0].permute(1, 0, 2).unsqueeze(2)          # (1, C, H, W) -> (H, C, 1, W): `differing` slices dimension 0
        return differing(rows_first(y), lambda i, j: rows_first(want(x[:, :, i:j], None if res is None else res[:, :, i:j])), 256)
    return differing(y, lambda i, j: want(x[i:j], None if res is None else res[i:j]), 32)


def run_conv(c, direct=False, outputs=None, form=None):
    """One convolution case through ConvEngine.conv -> (y, x, w, b, res, the kernel that ran).  direct: ONE library call whatever N.
    form: a dict that receives the tile code the executor stated."""
    import conv_plan_cases as P
    from pam import hrnet_hip
    e = engine(tile_cfg=c.get('tile', -1), pw64=False, slab32=c.get('slab32', False))   # pw64: no 64 -> 64 layer goes to k_pw1
    if form is not None:
        e.lib = P.ConvSpy(e.lib, lambda query, rc: form.update(tile=query[10], rc=rc, calls=form.get('calls', []) + [(query[0], rc)]))
    if direct:
        e.conv_slice = lambda n, *a, **k: n
    made = sentinel_outputs(e) if outputs is not None else None
    w, b = weights(c['cout'], c['cin'] if c['cin'] != 8 else 3, c['k'], 7)
    x = ints(c['n'], c['cin'], c['h'], c['w'], 11, lo=0 if c.get('nonneg') else -3)
    ho, wo = E.out_hw(c['h'], c['w'], c['k'], c['stride'])
    res = ints(c['n'], c['cout'], ho, wo, 13) if c.get('res') else None
    op = hrnet_hip.PackedConv(module(w, b, c['stride']), DEV, pad_cin_to=8 if c['cin'] == 8 else None)
    try:
        y = e.conv(op, x, res=res, relu=c.get('act', True))
        torch.cuda.synchronize()
    finally:
        if outputs is not None:
            outputs += made
    return y, (x[:, :3] if c['cin'] == 8 else x), w, b, res, e.lib.pam_conv_last_kernel()


def conv_case(id, n, h, w, cin, cout, k, stride, kernel, **kw):
    return pytest.param(dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, kernel=kernel, **kw), id=id)


def check_conv(c, direct=False):
    y, x, w, b, res, kernel = run_conv(c, direct)
    assert kernel == c['kernel'], (kernel, c)
    why = conv_differs(y, x, w, b, res, c['stride'], c.get('act', True))
    assert why is None, why


# ---- just below a frontier: the largest N the plan accepts ---------------------------------------------------------------------------------
# N = first_n - 1 of tests/test_conv_frontier.py: e.g. 606 x 192 x 144 x 64 x 2 = 2^31 - 3.1 MB
BELOW = [
    conv_case('igemm-3x3s2-in', 606, 192, 144, 64, 64, 3, 2, K_IGEMM, tile=-2, nonneg=True),     # the un-fused stem's conv2, classic code
    conv_case('gs-3x3s2-in', 606, 192, 144, 64, 64, 3, 2, K_GS, nonneg=True),                    # the same as the executor issues it
    conv_case('c3-48-in-res', 3236, 96, 72, 48, 48, 3, 1, K_3X3, res=True),                       # input and residual one image below 2^31
    conv_case('c3-48-96-in-res', 3236, 96, 72, 48, 96, 3, 1, K_3X3, res=True),                    # input below 2^31, residual and output one image below 2^32
    conv_case('stem-s2-in', 1213, 384, 288, 8, 64, 3, 2, K_STEM),                                 # input below 2^31, output 4 GiB - 2 MB
    conv_case('igemm-1x1-in', 1213, 96, 72, 256, 64, 1, 1, K_IGEMM, tile=-2),                    # no padding offset: input one image below 2^32
    conv_case('igemm-1x1-res', 1213, 96, 72, 64, 256, 1, 1, K_IGEMM, tile=-2, res=True),         # residual and output one image below 2^32
    conv_case('gs-1x1-res', 1213, 96, 72, 64, 256, 1, 1, K_GS, tile=8, res=True),
    conv_case('igemm-1x1-one-image', 1, 4096, 4096, 64, 64, 1, 1, K_IGEMM, tile=-2),             # 2^31 bytes exactly, the frontier inside the image
]


@pytest.mark.parametrize('c', BELOW)
def test_conv_families_one_image_below_their_frontier(c):
    check_conv(c, direct=True)


# ---- operands the table says are addressed beyond 2^31 and 2^32 bytes -----------------------------------------------------------------------
ABOVE = [
    conv_case('igemm-out-2^31', 607, 96, 72, 64, 256, 1, 1, K_IGEMM, tile=-2),                   # output 2.001 GiB
    conv_case('igemm-out-2^32', 1214, 96, 72, 64, 256, 1, 1, K_IGEMM, tile=-2),                  # output 4.001 GiB
    conv_case('gs-out-2^32', 1214, 96, 72, 64, 256, 1, 1, K_GS, tile=8),                         # k_conv_gs's output, 4.001 GiB
    conv_case('igemm-res-2^31', 607, 96, 72, 64, 256, 1, 1, K_IGEMM, tile=-2, res=True),         # the sentinel offset lies inside the residual
    conv_case('gs-falls-to-igemm-in-2^31', 607, 96, 72, 256, 64, 1, 1, K_IGEMM),                 # k_conv_gs's int offsets end; the implicit GEMM takes over
    conv_case('c3s-in-res-2^31', 2428, 96, 72, 64, 64, 3, 1, K_3X3S, res=True),                   # k_conv3x3s: 64-bit input pointers, 2.001 GiB
]


@pytest.mark.parametrize('c', ABOVE)
def test_conv_operands_beyond_2_31_and_2_32(c):
    check_conv(c, direct=True)


def test_unfused_stem_conv2_at_607_crops_runs_as_two_slices():
    """The first row of the issue's table: 607 x 192 x 144 x 64 is 2.001 GiB of input under padding taps.  The library refuses it; the
    executor issues 304 + 303 images, and every element is right -- the image borders and the slices' seam included."""
    import conv_plan_cases as P
    from pam import hrnet_hip
    calls = []
    e = engine()
    e.lib = P.ConvSpy(e.lib, lambda query, rc: calls.append((query[0], rc)))
    w, b = weights(64, 64, 3, 7)
    x = ints(607, 64, 192, 144, 11, lo=0)
    op = hrnet_hip.PackedConv(module(w, b, 2), DEV)
    y = e.conv(op, x, relu=True)
    torch.cuda.synchronize()
    assert calls == [(304, 0), (303, 0)], calls
    why = conv_differs(y, x, w, b, None, 2, True)
    assert why is None, why


def test_unfused_bottleneck_conv3_with_a_residual_of_2_32_bytes_runs_as_two_slices():
    """What HipPoseResNet._layer1 and the un-fused HRNet head lean on above their fused kernels' guard: 64 -> 256 1x1 + residual at 1214
    images of 96 x 72 (residual and output 4.001 GiB) is refused by the library and issued by the executor as 607 + 607."""
    form = {}
    c = dict(n=1214, h=96, w=72, cin=64, cout=256, k=1, stride=1, res=True, tile=-2)
    y, x, w, b, res, kernel = run_conv(c, direct=False, form=form)
    assert kernel == K_IGEMM and form['calls'] == [(607, 0), (607, 0)], form
    why = conv_differs(y, x, w, b, res, 1, True)
    assert why is None, why


def _down(kind, n, h, w, cin, cout):
    from pam import hrnet_hip
    e = engine()
    wt, b = weights(cout, cin, 3, 5)
    x = ints(n, cin, h, w, 17)
    op = hrnet_hip.PackedConv(module(wt, b, 2), DEV)
    if kind == 'down_s':
        assert e.lib.pam_conv3x3s2_slab(h, w, cin, cout) > 0
        y = e.conv_down_s(op, x, relu=True)
    else:
        y = e.conv_down48(op, x, relu=True)
    torch.cuda.synchronize()
    why = conv_differs(y, x, wt, b, None, 2, True)
    assert why is None, why


# pam_conv3x3s2_*: 64-bit input pointers; smallest network maps, narrowest widths; N just above 2^31 / 2^32 bytes of input
@pytest.mark.parametrize('kind,n,h,w,cin,cout', [('down48', 3237, 96, 72, 48, 96), ('down48', 6473, 96, 72, 48, 96),
                                                 ('down_s', 6473, 48, 36, 96, 192), ('down_s', 12946, 48, 36, 96, 192)],
                         ids=['k_down48-2^31', 'k_down48-2^32', 'k_down_s-2^31', 'k_down_s-2^32'])
def test_stride_2_kernels_with_inputs_beyond_2_31_and_2_32(kind, n, h, w, cin, cout):
    _down(kind, n, h, w, cin, cout)


@pytest.mark.parametrize('n', [3237, 6473], ids=['2^31', '2^32'])
def test_upsample_add_beyond_2_31_and_2_32(n):
    """k_upsample_add: 32-bit piece index (checked below 2^31 pieces), size_t byte offsets.  Base and output of n x 96 x 72 x 48."""
    e = engine()
    base, term = ints(n, 48, 96, 72, 21), ints(n, 48, 48, 36, 22)
    y = e.upsample_add(base, [term], [1], True)
    torch.cuda.synchronize()
    why = differing(y, lambda i, j: torch.relu(base[i:j].float() + E.up_nearest(term[i:j].float(), 1)), 256)
    assert why is None, why


@pytest.mark.parametrize('n', [6205, 12410], ids=['2^31', '2^32'])
def test_route_concat_beyond_2_31_and_2_32(n):
    """k_route: 32-bit piece index, size_t byte offsets.  A 32-channel slice of a 64-channel 52 x 52 layer beside a nearest-x2 source of
    32 channels, padded with zeros to 72 channels."""
    e = engine()
    a, b = ints(n, 64, 52, 52, 23), ints(n, 32, 26, 26, 24)
    y = e.route([(a, 32, 32, False), (b, 0, 32, True)], 72)
    torch.cuda.synchronize()
    why = differing(y, lambda i, j: torch.cat([a[i:j, 32:64].float(), E.up_nearest(b[i:j].float(), 1),
                                               torch.zeros((j - i, 8, 52, 52), device=DEV)], 1), 256)
    assert why is None, why


# ---- the fused entry points one image below their guard, and on it ----------------------------------------------------------------------------
def _block_want(x, w1, b1, w2, b2):
    t = E.rne_bf16(torch.relu(E.conv_direct(x.double(), w1, 1, 1) + b1)).double()
    return E.rne_bf16(torch.relu(E.conv_direct(t, w2, 1, 1) + b2 + x.double()))


def test_basic_block2_48_below_and_on_its_guard():
    """pam_basic_block2 (C = 48, 96 x 72): 3236 images run (2^31 - 0.2 MB), 3237 are refused with the output untouched."""
    from pam import _lib, hrnet_hip
    (w1, b1), (w2, b2) = weights(48, 48, 3, 31), weights(48, 48, 3, 32)
    # thinned second-stage weights keep the sums of the block's second convolution small (exact_ref's sharp regime does the same)
    w2 = w2 * (torch.rand(w2.shape, generator=torch.Generator().manual_seed(33)) < 0.25)
    op = hrnet_hip.PackedBlock(module(w1, b1, 1), module(w2, b2, 1), DEV)
    dev = [t.to(DEV) for t in (w1, b1.view(1, -1, 1, 1), w2, b2.view(1, -1, 1, 1))]
    x = ints(3237, 48, 96, 72, 34)
    e = engine()
    y = e.basic_block2(op, x[:3236])
    torch.cuda.synchronize()
    why = differing(y, lambda i, j: _block_want(x[i:j], *dev), 32)
    assert why is None, why
    del y
    made = sentinel_outputs(e)
    with pytest.raises(_lib.PamError):
        e.basic_block2(op, x, (16, 36))
    torch.cuda.synchronize()
    assert len(made) == 1 and untouched(made[0])


def test_pointwise64_below_and_on_its_guard():
    """pam_pointwise64 (k_pw1, buffer resources over n_pixels x 128 bytes): 2427 images of 96 x 72 run, 2428 are refused."""
    from pam import _lib, hrnet_hip
    w, b = weights(64, 64, 1, 41)
    op = hrnet_hip.PackedPointwise64(module(w, b, 1), DEV)
    x = ints(2428, 64, 96, 72, 42)
    e = engine()
    y = e.pointwise64(op, x[:2427])
    torch.cuda.synchronize()
    why = conv_differs(y, x[:2427], w, b, None, 1, True)
    assert why is None, why
    del y
    made = sentinel_outputs(e)
    with pytest.raises(_lib.PamError):
        e.pointwise64(op, x)
    torch.cuda.synchronize()
    assert len(made) == 1 and untouched(made[0])


def below_and_on(run, n_ok, check, n_outputs):
    """run(n) launches the entry point on the first n images and returns its outputs: n_ok images must be exact (check(outputs) -> None
    or a report), n_ok + 1 must be refused with every output -- all n_outputs of them allocated -- still the sentinel."""
    from pam import _lib
    outs = run(n_ok, None)
    torch.cuda.synchronize()
    why = check(outs)
    assert why is None, why
    del outs
    torch.cuda.empty_cache()
    made = []
    with pytest.raises(_lib.PamError):
        run(n_ok + 1, made)
    torch.cuda.synchronize()
    assert len(made) == n_outputs and all(untouched(t) for t in made), len(made)


def thin(w, seed, keep=0.25):
    """Later stages of a chain read sums, not inputs: thinned weights keep their own sums small (as exact_ref's sharp regimes do)."""
    return w * (torch.rand(w.shape, generator=torch.Generator().manual_seed(seed)) < keep)


def on_dev(*ts):
    return [t.to(DEV).view(1, -1, 1, 1) if t.dim() == 1 else t.to(DEV) for t in ts]


def _tail_want(t2, x0, res, w3, b3, wd, bd, w1n, b1n):
    """exact_ref._tail: X = rne(relu(conv3(t2) + b3 [+ down(x0) + bd] [+ res])), Y = rne(relu(conv1_next(X) + b1n))."""
    v = E.conv_direct(t2.double(), w3, 1, 0) + b3
    if x0 is not None:
        v = v + E.conv_direct(x0.double(), wd, 1, 0) + bd
    if res is not None:
        v = v + res.double()
    X = E.rne_bf16(torch.relu(v))
    return X, E.rne_bf16(torch.relu(E.conv_direct(X.double(), w1n, 1, 0) + b1n))


def _tail_ops(first):
    from pam import hrnet_hip
    (w3, b3), (wd, bd), (w1n, b1n) = weights(256, 64, 1, 51), weights(256, 64, 1, 52), weights(64, 256, 1, 53)
    w1n = thin(w1n, 54)
    op = hrnet_hip.PackedTail(module(w3, b3, 1), module(wd, bd, 1) if first else None, module(w1n, b1n, 1), DEV)
    return op, on_dev(w3, b3, wd, bd, w1n, b1n)


@pytest.mark.parametrize('first', [False, True], ids=['later-block', 'first-block'])
def test_bottleneck_tail_below_and_on_its_guard(first):
    """pam_bottleneck_tail (k_pw2; loads AND stores through buffer resources over n_pixels x 512 bytes, pam_pw.hip:311): 606 images of
    96 x 72 run exactly, 607 are refused."""
    op, W = _tail_ops(first)
    y2, x0, res = ints(607, 64, 96, 72, 55), (ints(607, 64, 96, 72, 56) if first else None), (None if first else ints(607, 256, 96, 72, 57))
    e = engine()

    def run(n, made):
        if made is not None:
            e._new = lambda *a: (made.append(sentinel(*a[:4])), made[-1])[1]
        return e.bottleneck_tail(op, y2[:n], None if x0 is None else x0[:n], None if res is None else res[:n], 0)

    def check(outs):
        X, Y = outs
        want = lambda i, j: _tail_want(y2[i:j], None if x0 is None else x0[i:j], None if res is None else res[i:j], *W)
        return differing(X, lambda i, j: want(i, j)[0], 32) or differing(Y, lambda i, j: want(i, j)[1], 32)
    below_and_on(run, 606, check, 2)


@pytest.mark.parametrize('first', [False, True], ids=['later-block', 'first-block'])
def test_bottleneck_fused_below_and_on_its_guard(first):
    """pam_bottleneck_fused (k_bneck, pam_bneck.hip:264: N H W 512 < 2^31; a store to the sentinel offset would WRITE at byte 2^31):
    606 images of 96 x 72 run exactly, 607 are refused."""
    from pam import hrnet_hip
    tail, W = _tail_ops(first)
    w2, b2 = weights(64, 64, 3, 58)
    op = hrnet_hip.PackedBneck(module(w2, b2, 1), tail, DEV)
    w2d, b2d = on_dev(w2, b2)
    y1, x0, res = ints(607, 64, 96, 72, 59, lo=0), (ints(607, 64, 96, 72, 60, lo=0) if first else None), (None if first else ints(607, 256, 96, 72, 61, lo=0))
    e = engine(c96_slab=48)

    def run(n, made):
        if made is not None:
            e._new = lambda *a: (made.append(sentinel(*a[:4])), made[-1])[1]
        return e.bottleneck_fused(op, y1[:n], None if res is None else res[:n], None if x0 is None else x0[:n])

    def check(outs):
        X, Y = outs

        def want(i, j):
            t2 = E.rne_bf16(torch.relu(E.conv_direct(y1[i:j].double(), w2d, 1, 1) + b2d))
            return _tail_want(t2, None if x0 is None else x0[i:j], None if res is None else res[i:j], *W)
        return differing(X, lambda i, j: want(i, j)[0], 32) or differing(Y, lambda i, j: want(i, j)[1], 32)
    below_and_on(run, 606, check, 2)


def test_stem_fused_below_and_on_its_guard():
    """pam_stem_fused (pam_stem.hip:289: N H W 16 < 2^31 for the 8-channel input): 1213 crops of 384 x 288 run exactly, 1214 are refused."""
    from pam import hrnet_hip
    (w1, b1), (w2, b2), (wp, bp) = weights(64, 3, 3, 62), weights(64, 64, 3, 63), weights(64, 64, 1, 64)
    w2, wp = thin(w2, 65), thin(wp, 66)
    P1, Pp = hrnet_hip.PackedConv(module(w1, b1, 2), DEV, pad_cin_to=8), hrnet_hip.PackedPointwise64(module(wp, bp, 1), DEV)
    op = hrnet_hip.PackedStem(P1, module(w2, b2, 2), Pp, DEV)
    W = on_dev(w1, b1, w2, b2, wp, bp)
    x8 = ints(1214, 8, 384, 288, 67)
    e = engine()

    def run(n, made):
        if made is not None:
            e._new = lambda *a: (made.append(sentinel(*a[:4])), made[-1])[1]
        return e.stem_fused(op, x8[:n])

    def want(i, j):
        a = E.rne_bf16(torch.relu(E.conv_direct(x8[i:j, :3].double(), W[0], 2, 1) + W[1]))
        x0 = E.rne_bf16(torch.relu(E.conv_direct(a.double(), W[2], 2, 1) + W[3]))
        return x0, E.rne_bf16(torch.relu(E.conv_direct(x0.double(), W[4], 1, 0) + W[5]))
    below_and_on(run, 1213, lambda o: differing(o[0], lambda i, j: want(i, j)[0], 32) or differing(o[1], lambda i, j: want(i, j)[1], 32), 2)


def resnet_engine():
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipPoseResNet.__new__(hrnet_hip.HipPoseResNet)
    e.lib = _lib.load(); e.device = DEV; e.count = None; e._keep = []; e.arena = None
    return e


def test_resnet_stem_below_and_on_its_guard():
    """pam_resnet_stem (pam_resnet.hip:107: N H W 16 < 2^31): 2730 crops of 256 x 192 run exactly, 2731 are refused."""
    from pam import hrnet_hip
    w, b = weights(64, 3, 7, 68)
    op = hrnet_hip.PackedResNetStem(module(w, b, 2), DEV)
    wd, bd = on_dev(w, b)
    x8 = ints(2731, 8, 256, 192, 69)
    e = resnet_engine()

    def run(n, made):
        if made is not None:
            e._new = lambda *a: (made.append(sentinel(*a[:4])), made[-1])[1]
        return e.resnet_stem(op, x8[:n])
    want = lambda i, j: E.rne_bf16(torch.nn.functional.max_pool2d(torch.relu(E.conv_direct(x8[i:j, :3].double(), wd, 2, 3) + bd), 3, 2, 1))
    below_and_on(run, 2730, lambda y: differing(y, want, 32), 1)


def test_deconv_below_and_on_its_guard():
    """pam_deconv4x4s2 (pam_resnet.hip:239: input and output below 2^31 bytes): 256 -> 64 channels at 16 x 12, where input and output have
    the same size (98304 bytes per image): 21845 images run exactly, 21846 are refused.  (The kernel is not specialised by width; the
    network's 256 -> 256 layers would be 2.2 TFLOP at this frontier.)"""
    from pam import hrnet_hip
    w, b = weights(64, 256, 4, 70)                                     # the direct form's kernels (Cout, Cin, 4, 4)
    ct = nn.ConvTranspose2d(256, 64, 4, 2, 1, bias=True)
    with torch.no_grad():
        ct.weight.copy_(E.deconv_weight(w).float()); ct.bias.copy_(b.float())
    op = hrnet_hip.PackedDeconv(ct, DEV)
    wd, bd = on_dev(w, b)
    x = ints(21846, 256, 16, 12, 71)
    e = resnet_engine()

    def run(n, made):
        if made is not None:
            e._new = lambda *a: (made.append(sentinel(*a[:4])), made[-1])[1]
        return e.deconv(op, x[:n], relu=True)

    def want(i, j):
        up = torch.zeros((j - i, 256, 31, 23), dtype=torch.float64, device=DEV)     # exact_ref.deconv_as_conv, on the device
        up[:, :, ::2, ::2] = x[i:j].double()
        return E.rne_bf16(torch.relu(E.conv_direct(up, wd, 1, 2) + bd))
    below_and_on(run, 21845, lambda y: differing(y, want, 64), 1)


@pytest.mark.parametrize('c', [
    conv_case('gen-minus-7', 3103, 52, 52, 128, 128, 3, 1, None, tile=-2, act='leaky', stated=-7),   # the executor states -7 for a leaky 3x3 layer
    conv_case('slab32-minus-8', 12946, 24, 18, 192, 192, 3, 1, None, slab32=True, stated=-8)])
def test_stated_streamed_forms_refuse_on_their_output_guard(c):
    """tile_cfg -7 / -8 (c3_out_32bit: output below 2^31 bytes, half of what k_conv3x3s addresses): the first N on the guard is refused
    and nothing is written.  The side below it is not run: 2^30 output elements x 9 Cin x 2 is 2.5 / 3.7 TFLOP at the forms' narrowest
    widths (128 / 192), over this file's bound per case; tests/test_conv_frontier.py holds the plan's answer there."""
    from pam import _lib
    made, form = [], {}
    with pytest.raises(_lib.PamError):
        run_conv(c, direct=True, outputs=made, form=form)
    torch.cuda.synchronize()
    assert form['tile'] == c['stated'], form
    assert len(made) == 1 and untouched(made[0])


# ---- the detector's 64-bit kernels and k_fuse_sum above 2^31 and 2^32 bytes ---------------------------------------------------------------------
@pytest.mark.parametrize('n', [1552, 3103], ids=['2^31', '2^32'])
def test_maxpool_beyond_2_31_and_2_32(n):
    """k_maxpool (size_t index): YOLOv3-tiny's first pool, 16 channels at 416 x 416 -> 208 x 208; the input is n x 5.5 MB."""
    x = ints(n, 16, 416, 416, 72)
    y = engine().maxpool(x, 2, 2)
    torch.cuda.synchronize()
    why = differing(y, lambda i, j: torch.nn.functional.max_pool2d(x[i:j].float(), 2, 2), 64)
    assert why is None, why


@pytest.mark.parametrize('n', [4137, 8273], ids=['2^31', '2^32'])
def test_upsample_concat_beyond_2_31_and_2_32(n):
    """k_upsample_concat (size_t index): 128 channels of 13 x 13 up-sampled beside 256 channels of 26 x 26; the output is n x 519 KB."""
    a, b = ints(n, 128, 13, 13, 73), ints(n, 256, 26, 26, 74)
    y = engine().upsample_concat(a, b)
    torch.cuda.synchronize()
    why = differing(y, lambda i, j: torch.cat([E.up_nearest(a[i:j].float(), 1), b[i:j].float()], 1), 256)
    assert why is None, why


@pytest.mark.parametrize('n', [1453, 2905], ids=['2^31', '2^32'])
def test_spp_concat_beyond_2_31_and_2_32(n):
    """k_spp (one workgroup per view and channel slab, size_t image offsets): 512 channels at 19 x 19 -> 2048; the output is n x 1.48 MB."""
    x = ints(n, 512, 19, 19, 75)
    y = engine().spp(x, (5, 9, 13))
    torch.cuda.synchronize()
    mp = torch.nn.functional.max_pool2d
    why = differing(y, lambda i, j: torch.cat([mp(x[i:j].float(), k, 1, k // 2) for k in (13, 9, 5)] + [x[i:j].float()], 1), 64)
    assert why is None, why


@pytest.mark.parametrize('n', [3237, 6473], ids=['2^31', '2^32'])
def test_fuse_sum_beyond_2_31_and_2_32(n):
    """k_fuse_sum (size_t offsets; pam_fuse_plan.hpp:71 bounds N H W): the 48-channel output at 96 x 72 from its base and the 96-channel
    branch at 48 x 36: y = relu(base + up(rne(conv1x1(src) + b))).  Base and output are n x 663 KB."""
    from pam import hrnet_hip
    w, b = weights(48, 96, 1, 76)
    op = hrnet_hip.PackedUp([module(w, b, 1)], [1], DEV)
    wd, bd = on_dev(w, b)
    base, src = ints(n, 48, 96, 72, 77), ints(n, 96, 48, 36, 78)
    y = engine().fuse_sum(op, base, [], [src], relu=True)
    torch.cuda.synchronize()
    want = lambda i, j: E.rne_bf16(torch.relu(base[i:j].double() + E.up_nearest(E.rne_bf16(E.conv_direct(src[i:j].double(), wd, 1, 0) + bd).double(), 1)))
    why = differing(y, want, 128)
    assert why is None, why


# ---- refusals of the conv plan: on the frontier, really allocated, outputs untouched --------------------------------------------------------
ON = [
    conv_case('igemm-3x3s2-in', 607, 192, 144, 64, 64, 3, 2, None, tile=-2, nonneg=True),
    conv_case('gs-3x3s2-in', 607, 192, 144, 64, 64, 3, 2, None, nonneg=True),
    conv_case('c3-48-in', 3237, 96, 72, 48, 48, 3, 1, None, res=True),
    conv_case('stem-s2-in', 1214, 384, 288, 8, 64, 3, 2, None),
    conv_case('igemm-1x1-in', 1214, 96, 72, 256, 64, 1, 1, None, tile=-2),
    conv_case('igemm-1x1-res', 1214, 96, 72, 64, 256, 1, 1, None, tile=-2, res=True),
    conv_case('gs-stated-one-image', 1, 4096, 4096, 64, 64, 1, 1, None, tile=8),
]


@pytest.mark.parametrize('c', ON)
def test_conv_plan_refuses_on_the_frontier_and_writes_nothing(c):
    from pam import _lib
    made = []
    with pytest.raises(_lib.PamError):
        run_conv(c, direct=True, outputs=made)
    torch.cuda.synchronize()
    assert len(made) == 1 and untouched(made[0])


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
from test_gpu_hrnet_modules import Checker, bf, env, issue  # noqa: E402,F401  (env: the module-scoped executor + fp32 reference fixture)
import hrnet_calibrated as HC  # noqa: E402


@pytest.mark.parametrize('n', [606, 607])
def test_head_at_the_first_sliced_crop_count_and_one_below(env, n):
    """stem + layer1 of HipHRNet, eager, at 384 x 288: 606 crops are one pass in which every fused kernel of the head runs at the largest
    batch its guard accepts (N H W 512 = 2^31 - 3.1 MB); 607 crops are two slices of 304 + 303.  Compared with the fp32 module on the
    first two and last two crops, the two crops either side of the slices' seam, and the crop that holds byte 2^31 of the 256-channel
    output (the last one)."""
    e, hip = env, env.hip
    g = torch.Generator(device=e.dev).manual_seed(600 + n)
    x = torch.randn((n, 3, 384, 288), generator=g, device=e.dev).to(torch.bfloat16)
    x8 = bf(torch.cat([x, torch.zeros((n, 5, 384, 288), dtype=x.dtype, device=x.device)], 1))
    picks = sorted({0, 1, 302, 303, 304, (2 ** 31) // (96 * 72 * 512), n - 2, n - 1} & set(range(n)))
    with torch.no_grad():
        ref = HC.stage_inputs(e.ref, x[picks].float())['layer1']
    hip.stop_after = 'layer1'
    try:
        y = issue(hip, lambda: hip._head(x8))
    finally:
        del hip.stop_after
    assert tuple(y.shape) == (n, 256, 96, 72)
    chk = Checker('head 384x288 n%d' % n)
    chk('head', 'crops %s of %d' % (picks, n), y[picks], ref)
    chk.done()
