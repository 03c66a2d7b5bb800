"""GPU: the HIP Darknet-53 executor (yolov3.HipDarknet) against fp32, launch by launch, on the calibrated detector of
darknet_calibrated.py, at the view counts and input sizes the product runs: the kernel the library picks for a layer depends on
M = views x rows x columns (k_conv_gs pixel tile, k_pw1 from 64 k pixels) and on the row width (k_conv3x3s general-activation tile,
the unfused 3x3 + k_upsample_add of rows wider than 136 columns).

Each step of ``HipDarknet.plan`` runs on its own (``run_step``) and reads the reference's own input to that step as a bf16 tensor, the
same one on both sides.  The reference step is the fp32 torch op on it: the folded conv with its weights rounded to bf16 as PackedConv
rounds them (biases fp32), then leaky 0.1 or linear, then for shortcut layers + the same bf16 skip tensor.  Its output, rounded to bf16,
is the next step's input (the reference forward stores bf16 like the executor).  Per output the relative L2 error is bounded over the
whole tensor, for the worst image, on the four edge strips (first / last row and column) and for the worst 32-channel group; zero-padded
output channels must be exactly 0 and upsample + route steps bitwise equal to the torch route.

Every conv launch records (pam_conv_last_kernel(), pam_conv_last_form()); k_pw1 and k_upsample_add launches are recorded from the
library entry the step called.  test_case_list_reaches_every_detector_form asserts that the cases of this file reach every form the
detector's dispatch can select, so a case list that stops reaching one fails instead of shrinking silently."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import darknet_calibrated as DC
from oracle import yolo_ref as Y

pytestmark = pytest.mark.gpu

# (width, height, views, executor toggles)
CASES = [(416, 416, 1, {}), (416, 416, 2, {}), (416, 416, 5, {}), (416, 416, 10, {}), (416, 416, 31, {}),
         (608, 608, 2, {}), (320, 320, 3, {}), (416, 256, 2, {}),
         (512, 512, 1, {}),                                   # the only sizes whose 256- / 512-channel 3x3 layers take MT = 5 tiles
         ] + [(416, 416, n, {k: False}) for n in (2, 10) for k in ('gen_streamed', 'pw64', 'unfuse_wide')]
CASE_IDS = ['%dx%d-n%d%s' % (w, h, n, ''.join('-no_' + k for k in t)) for w, h, n, t in CASES]

METRICS = ('all', 'img', 'row0', 'rowL', 'col0', 'colL', 'ch32')
# Largest relative L2 error allowed per op family and metric: 2.5 x the largest error the MI355X showed on the 416, 320 and 416 x 256
# cases, rounded up; over every case of this file (512 and 608 included) the largest error is 0.41 of its bound.
# What is left is the bf16 rounding of each output.  Observed maxima over all 1125 compared outputs (all / img / row0 / rowL / col0 /
# colL / ch32, in 1e-3):
#   stem 1.66 1.66 1.68 1.68 1.69 1.66 1.66 | conv1x1 1.68 1.69 1.74 1.73 1.72 1.72 1.74 | conv3x3s2 1.66 1.67 1.68 1.69 1.70 1.68 1.74
#   conv3x3 1.67 1.67 1.69 1.70 1.69 1.70 1.73 | conv3x3+shortcut 1.67 1.67 1.69 1.71 1.69 1.69 1.72
#   unfused3x3+add 1.79 1.80 1.81 1.78 1.82 1.82 1.81 | head1x1 1.71 1.75 1.78 1.85 1.79 1.81 1.83
# Planted faults (not committed) on the 416 x 416 cases at 2 and 5 views, worst metric over its bound:
#   k_conv_gs 64-pixel leaky tile drops the last partial tile   -> conv1x1 (53 outputs), 22 x whole tensor, 159 x last row, NaN in some
#   k_conv3x3s general form adds the shortcut before the leaky -> conv3x3+shortcut (40 outputs), up to 58 x
#   k_pw1 leaky with slope 0.01                                 -> conv1x1 layer 2, 20 x
#   head bias shifted by one channel                            -> head1x1 (all three heads), up to 320 x
#   unfused wide 3x3 drops its k_upsample_add term              -> unfused3x3+add layer 4, 208 x
# Each also failed test_detector_heads_within_the_bf16_floor (head error 2.6-37 x the bf16 floor).
TOL = {
    'stem':              dict(all=0.0042, img=0.0042, row0=0.0042, rowL=0.0042, col0=0.0043, colL=0.0042, ch32=0.0042),
    'conv1x1':           dict(all=0.0042, img=0.0043, row0=0.0044, rowL=0.0043, col0=0.0043, colL=0.0044, ch32=0.0044),
    'conv3x3s2':         dict(all=0.0042, img=0.0042, row0=0.0043, rowL=0.0042, col0=0.0043, colL=0.0043, ch32=0.0044),
    'conv3x3':           dict(all=0.0042, img=0.0043, row0=0.0043, rowL=0.0043, col0=0.0043, colL=0.0043, ch32=0.0044),
    'conv3x3+shortcut':  dict(all=0.0042, img=0.0042, row0=0.0043, rowL=0.0043, col0=0.0042, colL=0.0043, ch32=0.0044),
    'unfused3x3+add':    dict(all=0.0045, img=0.0045, row0=0.0045, rowL=0.0044, col0=0.0045, colL=0.0046, ch32=0.0046),
    'head1x1':           dict(all=0.0044, img=0.0044, row0=0.0045, rowL=0.0045, col0=0.0047, colL=0.0044, ch32=0.0046),
    'add':               dict(all=0.0045, img=0.0045, row0=0.0045, rowL=0.0044, col0=0.0045, colL=0.0046, ch32=0.0046),  # a [shortcut] no conv absorbs
}


def rel(d, r):
    return float(d.norm() / r.norm().clamp_min(1e-30))


def metrics(got, ref):
    g, r = got.float(), ref.float()
    d = g - r
    return dict(all=rel(d, r), img=max(rel(d[i], r[i]) for i in range(r.shape[0])),
                row0=rel(d[:, :, 0], r[:, :, 0]), rowL=rel(d[:, :, -1], r[:, :, -1]),
                col0=rel(d[:, :, :, 0], r[:, :, :, 0]), colL=rel(d[:, :, :, -1], r[:, :, :, -1]),
                ch32=max(rel(d[:, c:c + 32], r[:, c:c + 32]) for c in range(0, r.shape[1], 32)))


class Spy(object):
    """The executor's library with its launch entries recorded: a conv launch as (kernel, form) read right after it returns."""
    LAUNCHES = ('pam_conv2d_nhwc_bf16_ex', 'pam_pointwise64_act_nhwc_bf16', 'pam_upsample_add_nhwc_bf16_ex', 'pam_upsample_concat_nhwc_bf16')

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.LAUNCHES:
            return fn

        def launch(*args):
            rc = fn(*args)
            if name == 'pam_conv2d_nhwc_bf16_ex':
                self.calls.append(form_name(self._lib.pam_conv_last_kernel(), self._lib.pam_conv_last_form()))
            elif name == 'pam_pointwise64_act_nhwc_bf16':
                self.calls.append('k_pw1 act=%d' % args[-1])
            else:
                self.calls.append({'pam_upsample_add_nhwc_bf16_ex': 'k_upsample_add', 'pam_upsample_concat_nhwc_bf16': 'k_upsample_concat'}[name])
            return rc
        return launch


def form_name(kind, form):
    """(pam_conv_last_kernel, pam_conv_last_form) -> label (encoding: include/pam.h)."""
    if kind == 0:
        return 'k_conv_igemm%s %dx%d' % (' gen' if form >= 1000000 else '', form // 1000 % 1000, form % 1000)
    if kind == 1:
        return 'k_conv3x3 Cin=%d slab=%d' % (form // 10, 16 * (form % 10))
    if kind == 2:
        return 'k_conv3x3s%s Cin=%d slab=%d MT=%d' % (' gen' if form >= 100000 else '', form // 100 % 1000, 16 * (form // 10 % 10), form % 10)
    if kind == 3:
        return 'k_conv_gs tile=%d slab=%d nbuf=%d' % (form // 1000 % 1000, form % 1000, form // 1000000)
    if kind == 4:
        return 'k_conv_stem s%d Cout=%d' % (form // 100, form % 100)
    raise AssertionError('unknown conv kernel %d (form %d)' % (kind, form))


# Forms the detector's dispatch can select (from csrc/pam_conv_plan.hpp and ConvEngine.conv), each of which the cases above must reach:
REQUIRED = {
    'k_conv_stem s1 Cout=32',                                                  # layer 0
    'k_conv_gs tile=64 slab=64 nbuf=3', 'k_conv_gs tile=128 slab=64 nbuf=3',   # leaky 1x1 / stride-2 / unfused 3x3 layers: the pixel tile
    'k_conv_gs tile=256 slab=64 nbuf=3',                                       # that still is one round of workgroups, else 256
    'k_conv3x3s gen Cin=128 slab=64 MT=4', 'k_conv3x3s gen Cin=128 slab=64 MT=5',   # every general-activation instantiation
    'k_conv3x3s gen Cin=256 slab=32 MT=4', 'k_conv3x3s gen Cin=256 slab=32 MT=5',
    'k_conv3x3s gen Cin=512 slab=32 MT=4', 'k_conv3x3s gen Cin=512 slab=32 MT=5',
    'k_conv3x3 Cin=64 slab=64',                                                # the 104-wide 64 -> 128 block (classic, leaky + shortcut)
    'k_conv3x3 Cin=128 slab=64', 'k_conv3x3 Cin=256 slab=32', 'k_conv3x3 Cin=512 slab=32',   # gen_streamed = False
    'k_pw1 act=2',                                                             # 64 -> 32 (padded 64) 1x1 at >= 64 k pixels
    'k_upsample_add',                                                          # the unfused wide 3x3 layers' shortcut
    'k_conv_igemm gen 64x64',                                                  # that 1x1 below 64 k pixels (Kpad 64: no k_conv_gs)
    'k_conv_igemm gen 128x64',                                                 # ... above them with pw64 off; 3x3 + shortcut at 208 unfused off
    'k_conv_igemm gen 64x128', 'k_conv_igemm 64x128',                          # 26 x 26 layers at 31 views: two rounds of k_conv_gs tiles
}

_RECORDS = {}          # case id -> {(plan step dst, family): [launch labels]}


class Checker(object):
    def __init__(self, test):
        self.test, self.bad = test, []

    def __call__(self, family, where, got, ref):
        assert tuple(got.shape) == tuple(ref.shape), (where, tuple(got.shape), tuple(ref.shape))
        m = metrics(got, ref)
        print('PARITY ' + json.dumps(dict(test=self.test, family=family, where=where, **{k: round(v, 6) for k, v in m.items()})))
        self.bad += ['%s %s: %s %.4g > %.4g' % (family, where, k, m[k], TOL[family][k]) for k in METRICS if not m[k] <= TOL[family][k]]

    def done(self):
        assert not self.bad, '\n'.join(self.bad[:40])


class Env(object):
    pass


@pytest.fixture(scope='module')
def env():
    """One executor per input size (packing is per network), TF32 off for the fp32 reference."""
    from pam import _lib, yolov3
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    e = Env()
    e.dev = torch.device('cuda:0')
    e.nets = {}

    def net(w, h):
        if (w, h) not in e.nets:
            model = DC.calibrated(width=w, height=h)
            hip = yolov3.HipDarknet(model, e.dev)
            hip.lib = Spy(_lib.load())
            convs = {i: c.to(e.dev) for i, c in DC.folded_convs(model).items()}
            e.nets[(w, h)] = (model, hip, convs)
        return e.nets[(w, h)]
    e.net = net
    try:
        yield e
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def padded_bf16(r, c_pad):
    """fp32 (N, C, H, W) -> bf16 channels-last with zero channels up to c_pad (the executor's layout of that layer)."""
    y = r.to(torch.bfloat16)
    if c_pad > r.shape[1]:
        y = torch.cat([y, torch.zeros((r.shape[0], c_pad - r.shape[1]) + tuple(r.shape[2:]), dtype=y.dtype, device=y.device)], 1)
    return y.contiguous(memory_format=torch.channels_last)


def input_x8(e, w, h, n, seed):
    x = DC.images((n, 3, h, w), seed).to(torch.bfloat16).to(e.dev)
    return padded_bf16(x.float(), 8)


def family_of(hip, step, x):
    _, dst, op, src, act, skip = step
    if dst == 0:
        return 'stem'
    if skip is not None:
        return 'unfused3x3+add' if hip.unfused(step, x) else 'conv3x3+shortcut'
    if act == 'linear':
        return 'head1x1'
    if op.kh == 1:
        return 'conv1x1'
    return 'conv3x3s2' if op.stride == 2 else 'conv3x3'


def walk(e, w, h, n, toggles, check, seed=None, on_step=None):
    """Run the plan step by step on the reference's bf16 inputs; check(family, where, got, ref) per conv output.  -> {(dst, family):
    launches}.  on_step(step, outs, y) sees every executor output (outs still holds that step's inputs)."""
    model, hip, convs = e.net(w, h)
    last_use = {}
    for k, step in enumerate(hip.plan):
        for s in ([step[3]] + ([step[5]] if step[5] is not None else []) if step[0] == 'conv' else list(step[2:])):
            last_use[s] = k
    outs = {-1: input_x8(e, w, h, n, 1000 + 31 * n + w if seed is None else seed)}
    rec = {}
    saved = {k: hip.__dict__.get(k) for k in toggles}
    for k, v in toggles.items():
        setattr(hip, k, v)
    try:
        for k, step in enumerate(hip.plan):
            kind, dst = step[0], step[1]
            hip.lib.calls = []
            with torch.no_grad():
                y = hip.run_step(step, outs)
            torch.cuda.synchronize()
            if on_step is not None:
                on_step(step, outs, y)
            if kind == 'conv':
                _, _, op, src, act, skip = step
                fam = family_of(hip, step, outs[src])
                i = dst - 1 if skip is not None else dst
                c = convs[i]
                with torch.no_grad():
                    r = F.conv2d(outs[src][:, :c.in_channels].float(), c.weight, c.bias, c.stride, c.padding)
                    r = F.leaky_relu(r, 0.1) if act == 'leaky' else r
                    if skip is not None:
                        r = r + outs[skip][:, :c.out_channels].float()
                real = c.out_channels
                check(fam, 'layer %d' % dst, y[:, :real], r)
                if y.shape[1] > real:
                    assert float(y[:, real:].float().abs().max()) == 0.0, ('padded channels of layer %d' % dst)
                outs[dst] = padded_bf16(r, y.shape[1])
                rec[(dst, fam)] = list(hip.lib.calls)
                del r
            elif kind == 'upcat':
                a, b = outs[step[2]], outs[step[3]]
                want = torch.cat([F.interpolate(a.float(), scale_factor=2, mode='nearest'), b.float()], 1)
                assert torch.equal(y.float(), want), 'upsample + route of layer %d' % dst
                outs[dst] = y
                rec[(dst, 'upcat')] = list(hip.lib.calls)
            elif kind == 'add':
                with torch.no_grad():
                    r = outs[step[2]].float() + outs[step[3]].float()
                check('add', 'layer %d' % dst, y, r)
                outs[dst] = padded_bf16(r, y.shape[1])
                rec[(dst, 'add')] = list(hip.lib.calls)
            else:                                          # alias, head: the same tensor
                outs[dst] = outs[step[2]]
            del y
            for s in [s for s in outs if last_use.get(s, -1) <= k]:      # free what no later step reads (n = 31 at 416 is GBs)
                del outs[s]
    finally:
        for k, v in saved.items():
            if v is None:
                hip.__dict__.pop(k, None)
            else:
                setattr(hip, k, v)
    return rec


def run_case(e, case_id, w, h, n, toggles):
    chk = Checker(case_id)
    rec = walk(e, w, h, n, toggles, chk)
    _RECORDS[case_id] = rec
    print('FORMS ' + json.dumps(dict(case=case_id, layers=['%d %s: %s' % (d, f, ', '.join(v)) for (d, f), v in sorted(rec.items())])))
    return chk


@pytest.mark.parametrize('w,h,n,toggles', CASES, ids=CASE_IDS)
def test_every_launch_vs_fp32(env, w, h, n, toggles):
    """Every step of the plan at this input size, view count and executor setting, against the fp32 op on the same bf16 input."""
    case_id = CASE_IDS[CASES.index((w, h, n, toggles))]
    run_case(env, case_id, w, h, n, toggles).done()


def test_case_list_reaches_every_detector_form(env):
    """The union of the launches of every case includes every form in REQUIRED (cases not yet run in this session run here)."""
    seen = set()
    for (w, h, n, toggles), cid in zip(CASES, CASE_IDS):
        if cid not in _RECORDS:
            run_case(env, cid, w, h, n, toggles)
        for v in _RECORDS[cid].values():
            seen.update(v)
    print('SEEN ' + json.dumps(sorted(seen)))
    assert not REQUIRED - seen, sorted(REQUIRED - seen)
    # each toggle moves its layers off the default form
    assert any('k_conv3x3 Cin=128' in l for v in _RECORDS['416x416-n2-no_gen_streamed'].values() for l in v)
    assert not any('k_pw1' in l for v in _RECORDS['416x416-n10-no_pw64'].values() for l in v)
    assert not any('k_upsample_add' in l for v in _RECORDS['416x416-n10-no_unfuse_wide'].values() for l in v)


def test_per_image_outputs_are_batch_invariant(env):
    """Each layer's output for image 0 of a 5-view batch, bitwise, against the same layer run on that image alone (n = 1), on the same
    bf16 input: the kernel form of a layer changes with the batch (k_conv_gs pixel tile, k_pw1 from 64 k pixels), and the detector's
    boxes for a view must not depend on how many views share the launch.  Reports every layer whose output is not invariant."""
    model, hip, convs = env.net(416, 416)
    diff = []

    def one(step, outs, y):
        if step[0] in ('alias', 'head'):
            return
        solo = {k: v[:1].contiguous(memory_format=torch.channels_last) for k, v in outs.items()}
        calls = list(hip.lib.calls)
        with torch.no_grad():
            y1 = hip.run_step(step, solo)
        torch.cuda.synchronize()
        calls1 = list(hip.lib.calls[len(calls):])
        hip.lib.calls = calls
        if not torch.equal(y1[0], y[0]):
            diff.append('layer %d (%s vs %s): max |d| %.3g' % (step[1], ', '.join(calls1), ', '.join(calls), float((y1[0].float() - y[0].float()).abs().max())))
    walk(env, 416, 416, 5, {}, lambda *a: None, seed=4242, on_step=one)
    print('BATCHINV ' + json.dumps(diff))
    assert not diff, diff


# -- the whole detector, loaded from files through the product constructor ------------------------------------------------------------
# Heads vs the fp32 network.  A bf16 executor cannot beat the same network run in fp32 with bf16 weights and a bf16 store after every
# layer (darknet_calibrated.storage_forward): each head must stay within HEAD_FLOOR_RATIO of that floor, computed for the same images.
HEAD_FLOOR_RATIO = 1.1


@pytest.fixture(scope='module')
def detector(env, tmp_path_factory):
    from pam import yolov3
    d = str(tmp_path_factory.mktemp('darknet'))
    cfg, weights = os.path.join(d, 'yolov3.cfg'), os.path.join(d, 'calibrated.weights')
    with open(cfg, 'w') as f:
        f.write(yolov3.default_cfg())
    DC.calibrated().save_darknet_weights(weights)
    det = yolov3.YOLOv3(cfg, weights, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64)
    assert det.weights == weights
    det.test_files = (cfg, weights)
    return det


@pytest.mark.parametrize('n', [5, 31])
def test_detector_heads_within_the_bf16_floor(env, detector, n):
    model = DC.calibrated()
    x8 = input_x8(env, 416, 416, n, 77 + n)
    with torch.no_grad():
        heads = detector.net.forward(x8)
        x = x8[:, :3].float()
        ref = DC.storage_forward(model, x, bf16_weights=False, bf16_store=False)
        floor = DC.storage_forward(model, x)
    torch.cuda.synchronize()
    bad = []
    for k, (hd, r, fl) in enumerate(zip(heads, ref, floor)):
        assert hd.shape[1] == 256 and float(hd[:, 255:].float().abs().max()) == 0.0
        err, ferr = rel(hd[:, :255].float() - r, r), rel(fl - r, r)
        print('HEAD ' + json.dumps(dict(n=n, head=k, rel=err, floor=ferr)))
        if not err <= HEAD_FLOOR_RATIO * ferr:
            bad.append('head %d: rel err %.4g > %.2f x the bf16 floor %.4g' % (k, err, HEAD_FLOOR_RATIO, ferr))
    assert not bad, bad


def test_detector_boxes_replay_and_oracle(env, detector):
    """detect_dev on five 416 x 416 views (pixels / 255 are the calibrated input range): the graph replay equals an eager detector
    bitwise, and the boxes equal oracle/yolo_ref.detect applied to the kernel's own heads; every view has boxes."""
    from pam import yolov3
    n = 5
    rng = np.random.default_rng(21)
    imgs = rng.integers(0, 256, (n, 416, 416, 3), dtype=np.uint8)
    frames = torch.from_numpy(imgs).to(env.dev)
    b1, c1 = [t.clone() for t in detector.detect_dev(frames)]
    b2, c2 = [t.clone() for t in detector.detect_dev(frames)]                  # replay
    eager = yolov3.YOLOv3(*detector.test_files, None, score_thresh=0.5, nms_thresh=0.45, use_cuda=True, max_det=64, use_graph=False)
    b3, c3 = [t.clone() for t in eager.detect_dev(frames)]
    torch.cuda.synchronize()
    assert torch.equal(b1, b2) and torch.equal(c1, c2)
    assert torch.equal(b1, b3) and torch.equal(c1, c3)
    x8 = torch.from_numpy(Y.resize_frames(imgs, 416, 416)).to(env.dev).permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        hq = [t.permute(0, 2, 3, 1).float().cpu().numpy() for t in detector.net.forward(x8)]
    boxes, count = b1.cpu().numpy(), c1.cpu().numpy()
    for i in range(n):
        exp, cand = Y.detect([t[i] for t in hq], detector.anchors, 416, 416, 80, 0, 0.5, 0.45, 416, 416, 64)
        assert count[n + i] == cand and count[i] == len(exp), (i, count[i], len(exp), count[n + i], cand)
        assert len(exp) >= 1, i
        assert np.allclose(boxes[i, :count[i]], exp, rtol=2e-5, atol=1e-3), np.abs(boxes[i, :count[i]] - exp).max()
