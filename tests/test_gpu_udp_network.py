"""GPU: box_transform='udp' through HRNetPose.predict -- PoseResNet-50 and ViTPose-B at 256 x 192 with their seeded weights, 1 and 3
crops on 131 x 97 frames, plain and under flip_test + dark.  predict() against the reference chain: the network's input against
crop_udp64, the network's own features, the decode against udp64 and official_udp on the map the decode ran on; the dump's raw boxes;
the OKS-NMS on and off; one forward's outputs in guarded memory; two replays with the same bits."""
import functools
import json

import numpy as np
import pytest
import torch

import affine_ref as A
import dark_ref as D
import guarded_mem as G
import pose_nms_ref as P
import udp_ref as U
from image_ref import bf16_bits_to_f64, crop_check, noise_frames

pytestmark = pytest.mark.gpu

J = 17
FRAME = (131, 97)
RES = (256, 192)
HM = (64, 48)
BOXES = {1: [[[30.0, 20.0, 24.0, 70.0]], []], 3: [[[30.0, 20.0, 24.0, 70.0], [50.5, 60.25, 40.0, 12.0]], [[-6.0, 40.0, 60.0, 44.0]]]}
NETS = {'poseresnet50': dict(c=50, model_name='PoseResNet'), 'vitpose_b': dict(c='B', model_name='ViTPose')}
MODES = {'plain': dict(), 'flip+dark': dict(flip_test=True, shift_heatmap=False, dark=True)}


def parity(test, where, **figures):
    print('PARITY ' + json.dumps(dict(test=test, family='udp', where=where, **{k: (round(v, 7) if isinstance(v, float) else v) for k, v in figures.items()})))


@functools.lru_cache(maxsize=None)
def net_of(name, mode):
    """One object per (network, mode): flip_test doubles every forward and is fixed before the first capture."""
    from pam import hrnet
    kw = dict(NETS[name])
    net = hrnet.HRNetPose(kw.pop('c'), 17, None, resolution=RES, max_dets=2, graph_bucket=4, max_crops=4, box_transform='udp', **kw, **MODES[mode])
    assert net.box_transform == 'udp' and net.box_scale == 1.25 and net.uses_effective_box
    return net


@pytest.fixture(scope='module')
def frames():
    fr = noise_frames(2, FRAME[0], FRAME[1], 19)
    return fr, [torch.from_numpy(f).cuda() for f in fr]


def pbl(dev_frames, boxes):
    return [[dict(image_id=0, category_id=1, score=0.9, bbox=list(b), data=dev_frames[v], feature=[]) for b in bs] for v, bs in enumerate(boxes)]


def tables(boxes, dev):
    vl = [v for v, bs in enumerate(boxes) for _ in bs]
    sl = [s for bs in boxes for s in range(len(bs))]
    bx = np.asarray([b for bs in boxes for b in bs], dtype=np.float32)
    t = lambda a, d: torch.tensor(a, dtype=d, device=dev)
    return t(vl, torch.int32), t(sl, torch.int32), torch.from_numpy(bx).to(dev), vl, sl, bx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lift_bias(net, dev_frames):
    """Seeded random networks' maps straddle zero, where the clamp at 0.001 flattens the logarithm; the head bias is set once, from a
    first forward, so that every map value is at least 0.5 (the decode is what is tested here, the network's features are its own)."""
    if getattr(net, '_udp_test_bias', False):
        return
    net.predict(pbl(dev_frames, BOXES[3]))
    f0 = net.features(net.input_buffer(4))
    lowest = torch.einsum('nchw,jc->njhw', f0.float(), net.head_w.float()).amin(dim=(0, 2, 3))
    net.head_b.copy_(0.5 - lowest)
    net._udp_test_bias = True


@pytest.mark.parametrize('crops', [1, 3])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('name', list(NETS))
def test_predict_under_udp_equals_the_reference_chain(frames, name, mode, crops):
    """predict() with 1 and 3 crops: the effective table is pam_box_cs_host's; the network's input is crop_udp64's crop within its
    tolerance (mirrors: the column reversal bit for bit); the dump's rows are head_decode's on the replay's own features bit for bit;
    and on the map that call wrote -- the kernel's own bits, read in float64 -- the keypoints equal udp64's and official_udp's within
    the decode bound (64 x 2^-53 |M| through udp64's derivation) plus the float32 rounding of the mapping.  Then the same call again:
    the same bits, no new capture."""
    fr, dev_frames = frames
    net = net_of(name, mode)
    flip, dark = bool(MODES[mode].get('flip_test')), bool(MODES[mode].get('dark'))
    lift_bias(net, dev_frames)
    dev = net.device
    boxes = BOXES[crops]
    view_of, slot_of, bx, vl, sl, raw = tables(boxes, dev)
    n = len(vl)
    dump = net.predict(pbl(dev_frames, boxes))
    got = dump.device_det.clone()
    want_eff = A.box_cs64(raw, RES[1], RES[0])
    from pam import _lib
    assert np.array_equal(bits(_lib.box_cs(raw, RES[1], RES[0], 1.25)), bits(want_eff))
    assert np.array_equal(bits(dump.device_eff.cpu().numpy()), bits(want_eff))
    assert [[it['bbox'] for it in v] for v in dump] == boxes            # the dump's bbox stays the caller's box
    # the crop
    x = net.input_buffer(4)
    rows = x.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy()          # (N, H, W, 8)
    val, tol = U.crop_udp64(fr, np.asarray(vl), raw, RES)
    worst, bad = crop_check(bf16_bits_to_f64(rows[:n, :, :, :3].view(np.uint16)).transpose(0, 3, 1, 2), val, tol)
    assert bad == 0, (worst, bad)
    assert not flip or np.array_equal(rows[n:2 * n], rows[:n, :, ::-1])
    # the decode, re-issued on the replay's features with a heat-map pointer
    f = net.features(x)
    nf, c, h, w = f.shape
    assert nf == (8 if flip else 4) and (h, w) == HM
    eff = dump.device_eff
    det = torch.zeros_like(got); kp = torch.zeros((n, J, 3), dtype=torch.float32, device=dev)
    heat = torch.zeros((n, J, h, w), dtype=torch.float32, device=dev).contiguous(memory_format=torch.channels_last)
    net.head_decode(f, view_of, slot_of, eff, det, kp, heat=heat, n=n)
    torch.cuda.synchronize()
    for v, s in zip(vl, sl):
        assert torch.equal(got[v, s], det[v, s]), (v, s)
    listed = np.asarray([it['keypoints'] for v in dump for it in v], dtype=np.float32).reshape(n, J, 3)
    assert np.array_equal(listed, kp.cpu().numpy())
    drows = torch.stack([det[v, s] for v, s in zip(vl, sl)]).cpu().numpy()
    M = heat.cpu().numpy().astype(np.float64)
    assert (M > 0.25).all()
    bd = 64.0 * 2.0 ** -53 * np.abs(M)
    idx = M.reshape(n, J, -1).argmax(2)
    k = 11 if dark else 0
    assert not dark or net.dark_blur_kernel(h) == 11
    res = U.udp64(M, bd, idx, k)
    py, px, sy, sx = U.cells_of(drows, want_eff, h, w)
    verdict = D.judge(py, px, idx, res, w, sy, sx)
    assert verdict['wrong'] == [], verdict['wrong'][:5]
    assert np.array_equal(bits(drows[:, :, 2]), bits(M.reshape(n, J, -1)[np.arange(n)[:, None], np.arange(J)[None, :], idx]))
    dec = res['decided']
    figures = dict(cases=int(idx.size), decided=int(dec.sum()), worst_over_allowance=verdict['worst'])
    if dark:
        off = U.official_udp(M, k)
        assert dec.sum() >= 0.5 * idx.size, (int(dec.sum()), int(idx.size))
        ey, ex = np.abs(py - off[..., 1]), np.abs(px - off[..., 0])
        assert (ey[dec] <= (res['bound'] + sy)[dec] + 1e-10).all() and (ex[dec] <= (res['bound'] + sx)[dec] + 1e-10).all()
        figures.update(max_vs_official=float(max(ey[dec].max(), ex[dec].max())),
                       max_offset=float(np.maximum(np.abs(py - idx // w), np.abs(px - idx % w))[dec].max()))
    else:                                                              # no step: the rows are the mapping of the cell, to the bit
        wy, wx = U.map64(idx // w, idx % w, want_eff, h, w)
        assert np.array_equal(drows[:, :, 0], wy) and np.array_equal(drows[:, :, 1], wx)
    parity('test_predict_under_udp_equals_the_reference_chain', '%s %s n%d' % (name, mode, crops), **figures)
    # the affine decode of the same features lands elsewhere: the option reaches the decode
    det2 = torch.zeros_like(det)
    net.box_transform = 'affine'
    try:
        net.head_decode(f, view_of, slot_of, eff, det2, None, n=n)
    finally:
        net.box_transform = 'udp'
    torch.cuda.synchronize()
    assert not torch.equal(det2, det)
    # replay twice: the same bits, nothing captured
    caps = net.captures
    again = net.predict(pbl(dev_frames, boxes))
    assert net.captures == caps
    for v, s in zip(vl, sl):                                           # (the slots no crop names are never written)
        assert torch.equal(again.device_det[v, s], got[v, s]), (v, s)
    assert [[it['keypoints'] for it in v] for v in again] == [[it['keypoints'] for it in v] for v in dump]


@pytest.mark.parametrize('name', list(NETS))
def test_pose_nms_reads_the_effective_areas_under_udp(frames, name):
    """pose_nms on and off on the same object: off, predict() is what it was; on, the filter's counts, survivors and scores are
    pose_nms_ref's on the decode's rows with the areas We * He of the effective table, and the dump keeps the caller's boxes."""
    fr, dev_frames = frames
    net = net_of(name, 'plain')
    lift_bias(net, dev_frames)
    boxes = BOXES[3]
    _, _, _, vl, sl, raw = tables(boxes, net.device)
    assert not net.pose_nms
    plain = net.predict(pbl(dev_frames, boxes))
    det = plain.device_det.cpu().numpy()
    S = det.shape[1]
    eff = A.box_cs64(raw, RES[1], RES[0])
    want = P.apply(det, [len(b) for b in boxes], S, P.areas_from_rows(len(boxes), S, vl, sl, eff), np.full((len(boxes), S), 0.9, dtype=np.float32))
    net.pose_nms = True
    try:
        dump = net.predict(pbl(dev_frames, boxes))
        assert dump.device_n_det.cpu().numpy().tolist() == want['n_det_out'].tolist()
        kept = dump._kept()
        for v in range(len(boxes)):
            for s in range(int(want['n_det_out'][v])):
                assert np.array_equal(dump.device_det.cpu().numpy()[v, s], want['det'][v, s]), (v, s)
        assert [[it['bbox'] for it in v] for v in dump] == [[boxes[v][i] for i in kept[v]] for v in range(len(boxes))]
        assert np.array_equal(bits(dump.device_eff.cpu().numpy()), bits(eff))
    finally:
        net.pose_nms = False
    off = net.predict(pbl(dev_frames, boxes))
    for v, s in zip(vl, sl):
        assert torch.equal(off.device_det[v, s], plain.device_det[v, s]), (v, s)


@pytest.mark.parametrize('mode', list(MODES))
def test_one_udp_forward_in_guarded_memory(frames, mode):
    """preprocess -> features -> head_decode of the PoseResNet with its input, effective table, tracker rows and keypoints carved out of
    guarded_mem's sentinel arena: no band changes, every input element is written, the table's spare rows keep the sentinel, and the
    rows are predict()'s bit for bit."""
    fr, dev_frames = frames
    net = net_of('poseresnet50', mode)
    lift_bias(net, dev_frames)
    dev = net.device
    boxes = BOXES[3]
    view_of, slot_of, bx, vl, sl, raw = tables(boxes, dev)
    n = len(vl)
    dump = net.predict(pbl(dev_frames, boxes))
    N = net.forward_crops(4)
    V, S = int(dump.device_det.shape[0]), int(dump.device_det.shape[1])
    arena = G.GuardArena(dev, 2 * N * 8 * RES[0] * RES[1] + 16 * (n + 2) + V * S * J * 3 * 8 + n * J * 3 * 4 + 16 * G.GUARD + 16 * G.ALIGN)
    x = arena.alloc(N, 8, RES[0], RES[1])
    arena.alloc(n + 2, 8, 1, 1)                                       # the effective table: 16 bytes a row
    arena.alloc(V * S, 4 * J * 3, 1, 1)                               # (V, S, 17, 3) float64
    arena.alloc(n, 2 * J * 3, 1, 1)                                   # (n, 17, 3) float32
    eff = arena.payload(arena.allocs[1]).view(torch.float32).reshape(n + 2, 4)
    det = arena.payload(arena.allocs[2]).view(torch.float64).reshape(V, S, J, 3)
    kp = arena.payload(arena.allocs[3]).view(torch.float32).reshape(n, J, 3)
    ptrs = torch.tensor([f.data_ptr() for f in dev_frames], dtype=torch.int64, device=dev)
    net.preprocess(ptrs, FRAME[0], FRAME[1], view_of, bx, x, eff=eff)
    f = net.features(x)
    net.head_decode(f, view_of, slot_of, eff[:n], det, kp, n=n)
    torch.cuda.synchronize()
    assert arena.violations() == [], arena.report()
    unwritten = arena.unwritten()
    assert unwritten[0] == 0 and unwritten[3] == 0
    sent = np.uint32(G.SENTINEL << 16 | G.SENTINEL)
    eb = eff.cpu().numpy().view(np.uint32)
    assert np.array_equal(eb[:n], bits(A.box_cs64(raw, RES[1], RES[0]))) and (eb[n:] == sent).all()
    for v, s in zip(vl, sl):
        assert torch.equal(det[v, s], dump.device_det[v, s]), (v, s)
    listed = np.asarray([it['keypoints'] for v in dump for it in v], dtype=np.float32).reshape(n, J, 3)
    assert np.array_equal(listed, kp.cpu().numpy())
