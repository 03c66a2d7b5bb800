"""GPU: the flip test (pam_preprocess_crops_flip, pam_head_decode_flip) through the C ABI against the float64 restatement of
tests/flip_ref.py, then through HRNetPose.predict, FramePipeline and the ivclabpose facade.  Every output sits between guard bands;
rows a call does not cover keep their sentinel; every case prints a PARITY line.  The inputs, their bounds and the share of undecided
maps are those tests/test_flip_ref.py checks on the CPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import flip_ref as FR
import image_ref as R
from test_gpu_image_shapes import Guarded, stream, up

pytestmark = pytest.mark.gpu

J = R.J
OFFS = np.array([-0.25, 0.0, 0.25])


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib.load()


def parity(test, where, **figures):
    print('PARITY ' + json.dumps(dict(test=test, family='flip', where=where, **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in figures.items()})))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- mirrored crops -----------------------------------------------------------------------------------------------------------------------
CROP_FRAME = (600, 800)
CROP_BOXES = [[10, 20, 300, 500], [700.5, 87.75, 160.5, 300.25], [33.3, 44.7, 170.9, 230.1]]     # the second overhangs the right edge


def run_crops(lib, dev, fn, frames, view_of, boxes, res, out_c, n_total, antialias):
    """One of the two crop entry points into a guarded (n_total, H, W, out_c) bf16 buffer -> its bits (int16 numpy)."""
    H, W = res
    fr = [up(frames[v], dev) for v in range(frames.shape[0])]
    ptrs = torch.tensor([f.data_ptr() for f in fr], dtype=torch.int64, device=dev)
    out = Guarded(n_total * H * W * out_c, torch.bfloat16, dev)
    v_dev, b_dev = up(view_of, dev), up(boxes, dev)
    rc = fn(stream(dev), len(boxes), n_total, ptrs.data_ptr(), frames.shape[1], frames.shape[2], v_dev.data_ptr(), b_dev.data_ptr(),
            H, W, out_c, out.ptr(), antialias)
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.view(torch.int16).reshape(n_total, H, W, out_c).cpu().numpy()


@pytest.mark.parametrize('antialias', [0, 1])
@pytest.mark.parametrize('out_c', [3, 8])
@pytest.mark.parametrize('res', [(256, 192), (384, 288)], ids=['256x192', '384x288'])
def test_mirrored_crops_are_the_plain_crops_reversed(lib, dev, res, out_c, antialias):
    """pam_preprocess_crops_flip, 3 boxes over 2 views, n_total = 2n + 2: rows [0, n) bit-equal to pam_preprocess_crops_ex, rows [n, 2n)
    bit-equal to their column reversal (channels 3-7 of the 8-channel form +0), the spare rows equal to row 2n - 1."""
    frames = R.noise_frames(2, CROP_FRAME[0], CROP_FRAME[1], 7)
    boxes = np.asarray(CROP_BOXES, dtype=np.float32)
    view_of = np.array([0, 1, 0], dtype=np.int32)
    n = len(boxes)
    plain = run_crops(lib, dev, lib.pam_preprocess_crops_ex, frames, view_of, boxes, res, out_c, n, antialias)
    got = run_crops(lib, dev, lib.pam_preprocess_crops_flip, frames, view_of, boxes, res, out_c, 2 * n + 2, antialias)
    assert np.array_equal(got[:n], plain)
    assert np.array_equal(got[n:2 * n], plain[:, :, ::-1])
    assert not np.array_equal(plain, plain[:, :, ::-1])
    assert out_c == 3 or not got[:, :, :, 3:].any()                  # +0: all bits clear
    assert all(np.array_equal(got[k], got[2 * n - 1]) for k in range(2 * n, 2 * n + 2))
    parity('test_mirrored_crops', '%dx%d c%d aa%d' % (res + (out_c, antialias)), rows=int(got.shape[0]), mismatches=0)


# ---- head kernel ----------------------------------------------------------------------------------------------------------------------------
class FlipHead(object):
    """Device copies of one case (feature rows [0, n) plain, [n, 2n) mirrored, one spare) and the calls on it, every output guarded."""

    def __init__(self, lib, dev, feat, wt, b, boxes):
        self.lib, self.dev = lib, dev
        self.nf, self.h, self.w, self.C = feat.shape
        self.n = boxes.shape[0]
        assert self.nf == 2 * self.n + 1
        self.P = self.h * self.w
        self.f = up(feat, dev, torch.bfloat16)
        assert np.array_equal(self.f.float().cpu().numpy(), feat)
        self.wt, self.b = up(wt, dev), up(b, dev)
        self.rows = self.n + 1                                        # one more (view, slot), keypoint and heat-map row than the call covers
        self.boxes = up(np.concatenate([boxes, boxes[-1:]]), dev)
        self.view_of = (torch.arange(self.rows, dtype=torch.int32, device=dev) % 3).contiguous()
        self.slot_of = (torch.arange(self.rows, dtype=torch.int32, device=dev) // 3).contiguous()
        self.slots = (self.rows + 2) // 3

    def heatmaps(self):
        """pam_head_heatmaps of every feature row -> (nf, P, 17) float32 numpy."""
        out = Guarded(self.nf * self.P * J, torch.float32, self.dev)
        assert self.lib.pam_head_heatmaps(stream(self.dev), self.nf * self.P, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J, out.ptr()) == 0
        torch.cuda.synchronize()
        assert out.intact()
        return out.t.reshape(self.nf, self.P, J).cpu().numpy()

    def decode(self, flags, heat=False, plain_entry=False):
        """-> det rows (n, 17, 3) float64, kp (n, 17, 3), heat (n, P, 17) or None, raw bytes of (det, kp, heat) for byte comparisons."""
        n = self.n
        need = int(self.lib.pam_head_decode_flip_scratch_bytes(n, self.h, self.w))
        assert need == int(self.lib.pam_head_decode_scratch_bytes(n, self.h, self.w))
        scratch = Guarded(need, torch.uint8, self.dev)
        det = Guarded(3 * self.slots * J * 3, torch.float64, self.dev)
        kp = Guarded(self.rows * J * 3, torch.float32, self.dev)
        hm = Guarded(self.rows * self.P * J, torch.float32, self.dev) if heat else None
        tail = (hm.ptr() if heat else None, self.view_of.data_ptr(), self.slot_of.data_ptr(), self.boxes.data_ptr(), self.slots, det.ptr(), kp.ptr(), scratch.ptr())
        if plain_entry:
            rc = self.lib.pam_head_decode(stream(self.dev), n, self.h, self.w, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J, *tail)
        else:
            rc = self.lib.pam_head_decode_flip(stream(self.dev), n, n, self.h, self.w, self.f.data_ptr(), self.C, self.wt.data_ptr(), self.b.data_ptr(), J, flags, *tail)
        assert rc == 0
        torch.cuda.synchronize()
        assert scratch.intact() and det.intact() and kp.intact() and (hm is None or hm.intact())
        d = det.t.reshape(3, self.slots, J, 3)
        rows = torch.stack([d[i % 3, i // 3] for i in range(3 * self.slots)])
        assert det.untouched(rows[n:]) and kp.untouched(kp.t.reshape(self.rows, J, 3)[n:])
        h3 = hm.t.reshape(self.rows, self.P, J) if heat else None
        assert h3 is None or hm.untouched(h3[n:])
        raw = (det.t.cpu().numpy().tobytes(), kp.t.cpu().numpy().tobytes(), hm.t.cpu().numpy().tobytes() if heat else b'')
        return rows[:n].cpu().numpy(), kp.t.reshape(self.rows, J, 3)[:n].cpu().numpy(), (h3[:n].cpu().numpy() if heat else None), raw


def merged32(hh, n, h, w, flags):
    """The merged map formed in float32 on the host from pam_head_heatmaps' output hh (2n + 1, P, 17): 0.5f * (P + F[pair][xs])."""
    if not flags & 1:
        return hh[:n]
    xs = FR.source_columns(w, bool(flags & 2))
    src = (np.arange(h)[:, None] * w + xs[None, :]).reshape(-1)
    with np.errstate(invalid='ignore'):
        return np.float32(0.5) * (hh[:n] + hh[n:2 * n][:, src][:, :, FR.PAIR])


def rows_to_cells(rows, boxes, h, w):
    """det rows (n, 17, 3) (y, x, score) -> flat cell (n, 17) and offsets oy, ox in {-1, 0, 1} quarter cells: the (cell, offset) whose
    box mapping (image_ref.decode64 on the fractional cell) gives exactly that (y, x).  A row that is no such image fails here."""
    n = rows.shape[0]
    yc = (np.arange(h)[:, None] + OFFS[None, :]).reshape(-1); xc = (np.arange(w)[:, None] + OFFS[None, :]).reshape(-1)
    ytab, _ = R.decode64(np.broadcast_to(yc, (n, yc.size)), np.zeros((n, 1)), boxes, h, w)
    _, xtab = R.decode64(np.zeros((n, 1)), np.broadcast_to(xc, (n, xc.size)), boxes, h, w)
    idx = np.empty((n, J), dtype=np.int64); oy = np.empty((n, J), dtype=np.int64); ox = np.empty((n, J), dtype=np.int64)
    for i in range(n):
        for j in range(J):
            ky = np.nonzero(ytab[i] == rows[i, j, 0])[0]; kx = np.nonzero(xtab[i] == rows[i, j, 1])[0]
            assert ky.size == 1 and kx.size == 1, ('row is not the image of a cell + quarter offset', i, j, rows[i, j].tolist())
            idx[i, j] = (ky[0] // 3) * w + kx[0] // 3
            oy[i, j], ox[i, j] = ky[0] % 3 - 1, kx[0] % 3 - 1
    return idx, oy, ox


def check_decode(name, where, rows, kp, heat, m32, M, bd, boxes, h, w, flags):
    """One call's rows against the float64 map M (n, 17, h, w) and its bound: arg-max through image_ref.argmax_check (wrong == [],
    undecided <= 1 %), score within the bound of M at the returned cell, every decided quarter-pixel sign exact (an undecided one may
    be anything; without flag 4 and outside the strict border every offset is 0), (y, x) the box-mapped image of cell + offset.
    m32 (n, P, 17), the same map formed in float32 from pam_head_heatmaps: the score, the written map, the arg-max and the signs
    are its own bits (the head chain is bit-identical in every kernel)."""
    n = rows.shape[0]
    flatM, flatB = M.reshape(n, J, -1), bd.reshape(n, J, -1)
    idx, oy, ox = rows_to_cells(rows, boxes[:n], h, w)
    res = R.argmax_check(flatM, flatB, idx)
    assert res['wrong'] == [], (name, where, res['wrong'][:5])
    assert res['undecided'] <= 0.01 * res['maps'], (name, where, res['undecided'])
    a, c = np.arange(n)[:, None], np.arange(J)[None, :]
    want, tol = flatM[a, c, idx], flatB[a, c, idx]
    fin = np.isfinite(want)
    with np.errstate(invalid='ignore'):
        score_ratio = float((np.abs(rows[:, :, 2] - want)[fin] / tol[fin]).max()) if fin.any() else 0.0
    assert score_ratio <= 1.0 and np.array_equal(rows[:, :, 2][~fin], want[~fin]), (name, where, score_ratio)
    inside, sx, sy, dx, dy = FR.quarter64(M, bd, idx)
    if not flags & 4:
        sx, sy, dx, dy = np.zeros_like(sx), np.zeros_like(sy), np.ones_like(dx), np.ones_like(dy)
    assert np.array_equal(ox[dx], sx[dx]) and np.array_equal(oy[dy], sy[dy]), (name, where, 'quarter-pixel sign')
    assert not ox[~inside].any() and not oy[~inside].any()
    assert np.array_equal(kp[:, :, 0].astype(np.float64), rows[:, :, 1]) and np.array_equal(kp[:, :, 1].astype(np.float64), rows[:, :, 0])
    assert np.array_equal(kp[:, :, 2].astype(np.float64), rows[:, :, 2])
    # the kernel's own bits
    m = m32.transpose(0, 2, 1)                                        # (n, 17, P)
    with np.errstate(invalid='ignore'):
        first = np.where(np.isneginf(m).all(2) | np.isnan(m.max(2)), 0, m.argmax(2))
    assert np.array_equal(idx, first), (name, where, 'arg-max of the float32 map')
    assert np.array_equal(bits(rows[:, :, 2]), bits(m[a, c, idx])), (name, where, 'score bits')
    if flags & 4:
        m4 = m.reshape(n, J, h, w); py, px = idx // w, idx % w
        cl = lambda v, hi: np.clip(v, 0, hi)
        with np.errstate(invalid='ignore'):
            ex = m4[a, c, py, cl(px + 1, w - 1)] - m4[a, c, py, cl(px - 1, w - 1)]
            ey = m4[a, c, cl(py + 1, h - 1), px] - m4[a, c, cl(py - 1, h - 1), px]
        sgn = lambda e: np.where(inside, np.where(e > 0, 1, np.where(e < 0, -1, 0)), 0)
        assert np.array_equal(ox, sgn(ex)) and np.array_equal(oy, sgn(ey)), (name, where, 'signs of the float32 map')
    heat_ratio = 0.0
    if heat is not None:
        assert np.array_equal(bits(heat), bits(m32)), (name, where, 'written map bits')
        g = heat.transpose(0, 2, 1).astype(np.float64)
        ok = np.isfinite(flatM)
        with np.errstate(invalid='ignore'):
            heat_ratio = float((np.abs(g - flatM)[ok] / flatB[ok]).max())
        assert heat_ratio <= 1.0 and np.array_equal(g[~ok], flatM[~ok]), (name, where, heat_ratio)
    parity(name, where, flags=flags, maps=res['maps'], undecided=res['undecided'], undecided_signs=int((~dx).sum() + (~dy).sum()),
           score_ratio=score_ratio, heat_ratio=heat_ratio, offsets=int((ox != 0).sum() + (oy != 0).sum()))
    return idx, oy, ox


def reference(feat, wt, b, n, flags):
    hmP, bdP, hmF, bdF = FR.maps64(feat, wt, b, n)
    return FR.merge64(hmP, bdP, hmF, bdF, bool(flags & 2)) if flags & 1 else (hmP, bdP)


FLAG_SETS = (1, 3, 5, 7, 4)
RANDOM_CASES = [(c, hw, n) for c in FR.FLIP_CHANNELS for hw in FR.FLIP_MAPS for n in FR.FLIP_CROPS]


@pytest.mark.parametrize('C_,hw,n', RANDOM_CASES, ids=['C%d-%dx%d-n%d' % (c, hw[0], hw[1], n) for c, hw, n in RANDOM_CASES])
def test_flip_head_vs_fp64(lib, dev, C_, hw, n):
    """pam_head_decode_flip with flags 1, 3, 5, 7 and 4 on seeded random features (a batch of 2n + 1 rows), with and without a heat-map
    pointer; flags 0 against pam_head_decode byte for byte (det, kp and heat-maps)."""
    h, w = hw
    name = 'C%d %dx%d n%d' % (C_, h, w, n)
    feat, wt, b, boxes = FR.flip_inputs(C_, h, w, n)
    hd = FlipHead(lib, dev, feat, wt, b, boxes)
    hh = hd.heatmaps()
    ref = {}
    for flags in FLAG_SETS:
        key = flags & 3
        if key not in ref:
            ref[key] = reference(feat, wt, b, n, flags)
        M, bd = ref[key]
        m32 = merged32(hh, n, h, w, flags)
        rows, kp, _, raw = hd.decode(flags)
        check_decode('test_flip_head_vs_fp64', name, rows, kp, None, m32, M, bd, boxes, h, w, flags)
        rows2, kp2, heat, raw2 = hd.decode(flags, heat=True)
        assert raw2[:2] == raw[:2], (name, flags, 'the heat-map pointer changed the keypoints')
        check_decode('test_flip_head_vs_fp64', name + ' +heat', rows2, kp2, heat, m32, M, bd, boxes, h, w, flags)
    for heat in (False, True):
        assert hd.decode(0, heat=heat)[3] == hd.decode(0, heat=heat, plain_entry=True)[3], (name, 'flags 0', heat)


@pytest.mark.parametrize('hw', FR.PLANT_MAPS, ids=['%dx%d' % hw for hw in FR.PLANT_MAPS])
def test_flip_head_planted_cases(lib, dev, hw):
    """The planted crops of flip_ref.planted_inputs (one crop per case): a peak only in the mirrored crop shows in the swapped joint at
    the mirrored (shifted) column, the shift's edge columns, an exact plain-fed / mirror-fed tie across a tile seam (lower index wins),
    peaks at the border rows and columns (offset strictly inside only), equal neighbours (no offset), a neighbour pair ordered by the
    mirrored crop alone, joint 7 with a -inf bias (cell 0, score -inf, no offset)."""
    h, w = hw
    for flags in (5, 7, 4):
        feat, wt, b, boxes, cases = FR.planted_inputs(h, w, bool(flags & 2), merged=bool(flags & 1))
        n = len(cases)
        for weights in ('main', 'tie') if flags & 1 else ('main',):
            wt_, b_ = FR.tie_weights(wt, b) if weights == 'tie' else (wt, b)
            hd = FlipHead(lib, dev, feat, wt_, b_, boxes)
            M, bd = reference(feat, wt_, b_, n, flags)
            rows, kp, heat, _ = hd.decode(flags, heat=True)
            name = 'planted %dx%d %s' % (h, w, weights)
            idx, oy, ox = check_decode('test_flip_head_planted_cases', name, rows, kp, heat, merged32(hd.heatmaps(), n, h, w, flags), M, bd, boxes, h, w, flags)
            assert (idx[:, 7] == 0).all() and np.isneginf(rows[:, 7, 2]).all() and not ox[:, 7].any() and not oy[:, 7].any()
            for i, cname, e in cases:
                if (cname == 'tie') != (weights == 'tie'):
                    continue
                j, where = e['joint'], (name, cname, flags)
                if flags & 1:
                    if e.get('among'):
                        assert idx[i, j] in e['among'], where
                    if 'tie' in e:
                        assert idx[i, j] == e['cell'] and bits(heat[i, e['cell'], j]) == bits(heat[i, e['tie'], j]), where
                if 'inside' in e:
                    assert idx[i, j] == e['cell'], where
                    assert e['inside'] or (ox[i, j] == 0 and oy[i, j] == 0), where
                    assert not e['inside'] or (ox[i, j] != 0 and oy[i, j] != 0), where          # random neighbours: never equal
                if 'dx' in e:
                    want = e['dx'] if flags & 1 else 0
                    assert idx[i, j] == e['cell'] and ox[i, j] == want, where


# ---- network level --------------------------------------------------------------------------------------------------------------------------
NET_FRAME = (288, 360)
NET_BOXES = [[[20.0, 30.0, 100.0, 200.0], [150.5, 40.25, 90.0, 180.0]], [[200.0, 60.0, 120.0, 210.0]]]
MORE_BOXES = [[[20.0, 30.0, 100.0, 200.0], [150.5, 40.25, 90.0, 180.0], [10.0, 5.0, 60.0, 120.0]], [[200.0, 60.0, 120.0, 210.0], [5.5, 7.25, 200.0, 260.0]]]


def _pbl(frames, boxes):
    return [[dict(image_id=0, category_id=1, score=0.9, bbox=b, data=frames[v], feature=[]) for b in bs] for v, bs in enumerate(boxes)]


def _net_case(kw):
    from pam import hrnet
    net = hrnet.HRNetPose(*kw.pop('args'), resolution=(256, 192), max_dets=4, **kw)
    frames = [f for f in R.noise_frames(2, NET_FRAME[0], NET_FRAME[1], 11)]
    return net, frames


@pytest.mark.parametrize('case', ['r50-flip-post', 'w32-flip'])
def test_predict_under_the_flip_test(case):
    """predict() of 3 boxes over 2 views under the default graph_bucket (a forward of 8 crops: 3 plain, 3 mirrored, 2 spare): the
    feature batch of that forward, read back, merged and decoded in float64 with the network's head weights, must carry the dump's
    keypoints through the arg-max and sign checks -- the row layout through bucket padding and replay.  A second predict() of 5 boxes
    (another bucket) in between does not disturb the first dump."""
    kw = dict(args=(50, 17, None), model_name='PoseResNet', flip_test=True, post_process=True) if case == 'r50-flip-post' else \
        dict(args=(32, 17, None), flip_test=True)
    net, frames = _net_case(kw)
    flags = net.decode_flags()
    assert flags == (7 if case == 'r50-flip-post' else 3)
    dump = net.predict(_pbl(frames, NET_BOXES))
    dump2 = net.predict(_pbl(frames, MORE_BOXES))
    assert (8, 'features', 0) in net._graphs and (16, 'features', 0) in net._graphs
    n = 3
    x = net.input_buffer(4)                                            # the 8-row replay's own input: what preprocess filled for `dump`
    assert x.shape[0] == 8
    xb = x.view(torch.int16) if x.is_contiguous() else x.permute(0, 2, 3, 1).contiguous().view(torch.int16)
    assert torch.equal(xb[n:2 * n], xb[:n].flip(2)) and torch.equal(xb[2 * n], xb[2 * n - 1]) and torch.equal(xb[7], xb[2 * n - 1])
    f = net.features(x)
    feat = f.permute(0, 2, 3, 1).float().cpu().numpy()                 # (8, h, w, C)
    h, w = feat.shape[1:3]
    wt, b = net.head_w.cpu().numpy(), net.head_b.cpu().numpy()
    M, bd = reference(feat, wt, b, n, flags)
    boxes = np.asarray([bx for v in NET_BOXES for bx in v], dtype=np.float32)
    got = dump.device_det.cpu().numpy()
    rows = np.stack([got[0, 0], got[0, 1], got[1, 0]])
    listed = np.asarray([it['keypoints'] for v in dump for it in v]).reshape(n, J, 3)
    kp = listed.astype(np.float32)
    assert np.array_equal(listed[:, :, [1, 0, 2]], rows)
    lib = net.lib
    hh = np.empty((2 * n + 1,) + (h * w, J), dtype=np.float32)
    hm = torch.empty((8 * h * w * J,), dtype=torch.float32, device=f.device)
    assert lib.pam_head_heatmaps(stream(f.device), 8 * h * w, f.data_ptr(), f.shape[1], net.head_w.data_ptr(), net.head_b.data_ptr(), J, hm.data_ptr()) == 0
    hh[:] = hm.reshape(8, h * w, J)[:2 * n + 1].cpu().numpy()
    check_decode('test_predict_under_the_flip_test', case, rows, kp, None, merged32(hh, n, h, w, flags), M, bd, boxes, h, w, flags)
    assert len(dump2[0]) == 3 and len(dump2[1]) == 2


def test_predict_without_the_options_is_the_plain_decode():
    """flip_test=False: predict() is the parent's -- the dump equals pam_head_decode composed by hand on the read-back features, the
    forward has as many rows as the bucket, and the crops are those of pam_preprocess_crops_ex."""
    net, frames = _net_case(dict(args=(50, 17, None), model_name='PoseResNet'))
    assert net.decode_flags() == 0 and net.forward_crops(4) == 4
    dump = net.predict(_pbl(frames, NET_BOXES))
    assert (4, 'features', 0) in net._graphs and (8, 'features', 0) not in net._graphs
    n, dev = 3, net.device
    f = net.features(net.input_buffer(4))
    h, w = f.shape[2:]
    boxes = torch.tensor([bx for v in NET_BOXES for bx in v], dtype=torch.float32, device=dev)
    view_of = torch.tensor([0, 0, 1], dtype=torch.int32, device=dev); slot_of = torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    det = torch.zeros_like(dump.device_det); kp = torch.zeros((n, J, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty((int(net.lib.pam_head_decode_scratch_bytes(n, h, w)),), dtype=torch.uint8, device=dev)
    assert net.lib.pam_head_decode(stream(dev), n, h, w, f.data_ptr(), f.shape[1], net.head_w.data_ptr(), net.head_b.data_ptr(), J, None,
                                   view_of.data_ptr(), slot_of.data_ptr(), boxes.data_ptr(), det.shape[1], det.data_ptr(), kp.data_ptr(),
                                   scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    got = dump.device_det
    for v, s in ((0, 0), (0, 1), (1, 0)):
        assert torch.equal(got[v, s], det[v, s])
    listed = np.asarray([it['keypoints'] for v in dump for it in v], dtype=np.float32).reshape(n, J, 3)
    assert np.array_equal(listed, kp.cpu().numpy())


# ---- pipeline and facade ----------------------------------------------------------------------------------------------------------------
def test_prewarmed_flip_pipeline_never_captures_and_feeds_the_tracker_its_own_keypoints():
    """FramePipeline(prewarm=True, flip_test=True) with PoseResNet-50 over 6 Shelf-like frames: the prewarm captures the doubled forwards
    (8, 16, 24 crops for buckets of 4, 8, 12 boxes), no step captures, and every frame's tracker record equals the one a pipeline
    without a network gives when it is fed the decoded keypoints."""
    from pam import synth
    from pam.pipeline import FramePipeline
    from test_gpu_pipeline import _rig
    seq, cams, cfg, conf, meta = _rig('S2')
    Cv, md = meta['C'], 2
    pipe = FramePipeline(cams, cfg, conf, (meta['h'], meta['w']), max_dets=md, prewarm=True, autotune=False, width=50, model_name='PoseResNet',
                         resolution=(256, 192), flip_test=True, post_process=True)
    net = pipe.net
    assert net.flip_test and net.post_process and net.shift_heatmap and net.decode_flags() == 7
    assert pipe.warmed['buckets'] == [4, 8, 12] and sorted(k[0] for k in net._graphs) == [8, 16, 24]
    fed = FramePipeline(cams, cfg, conf, (meta['h'], meta['w']), max_dets=md, hrnet=False)
    dev = pipe.device
    frames = [up(f, dev) for f in R.noise_frames(Cv, meta['h'], meta['w'], 13)]
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=dev)
    c0, seen = net.captures, set()
    for t in range(6):
        vl, sl, bx = [], [], []
        for v in range(Cv):
            for s, kp in enumerate(seq['frames'][t][v][:((t + v) % (md + 1))]):
                x0, y0, x1, y1 = kp[:, 0].min(), kp[:, 1].min(), kp[:, 0].max(), kp[:, 1].max()
                vl.append(v); sl.append(s); bx.append([x0, y0, max(x1 - x0, 8.0), max(y1 - y0, 8.0)])
        cnt = torch.tensor([vl.count(v) for v in range(Cv)], dtype=torch.int32, device=dev)
        seen.add(len(vl))
        if vl:
            pipe.pose_step(ptrs, torch.tensor(vl, dtype=torch.int32, device=dev), torch.tensor(sl, dtype=torch.int32, device=dev),
                           torch.tensor(bx, dtype=torch.float32, device=dev).reshape(-1, 4))
        assert net.captures == c0, t
        rows = pipe.det_local[:, :md].clone()
        pipe.track_step(t, cnt)
        ra = pipe.results(strict=False)
        fed.track_step(t, cnt, rows)
        rb = fed.results(strict=False)
        assert ra['n_tracks'] == rb['n_tracks'], t
        for ta, tb in zip(ra['tracks'], rb['tracks']):
            assert ta['track_id'] == tb['track_id'] and ta['emitted'] == tb['emitted'], t
            if ta['emitted']:
                assert np.array_equal(ta['pose3d'], tb['pose3d']), t
        if vl:                                                          # quarter-cell offsets reached the records
            assert bool((rows != 0).any())
    assert len(seen) >= 3, seen


def test_facade_reads_the_three_keys_from_the_fliptest_config():
    """configs/Shelf/model_configs_fliptest.yaml: the facade's network has the three options on; the stock Shelf config leaves them off."""
    import pam
    from pam import synth
    from pam.dataset import GetConfig
    from pam.ivclabpose import ivclabpose
    cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
    path = os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_fliptest.yaml')
    p = dict(GetConfig(path).POSE_MODELS.HRPOSE)
    assert p['FLIP_TEST'] is True and p['SHIFT_HEATMAP'] is True and p['POST_PROCESS'] is True
    p['CHECKPOINT_FILE'] = ''
    net = ivclabpose({'NAME': ''}, p, dict(cfg, NAME='Iterative'), conf).pose_model
    assert net.flip_test and net.shift_heatmap and net.post_process and net.decode_flags() == 7 and net.forward_crops(20) == 40
    stock = dict(GetConfig(os.path.join(os.path.dirname(path), 'model_configs.yaml')).POSE_MODELS.HRPOSE)
    assert not {'FLIP_TEST', 'SHIFT_HEATMAP', 'POST_PROCESS'} & set(stock)
