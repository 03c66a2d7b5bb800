"""CPU: the float64 restatement of the UDP protocol (tests/udp_ref.py) against an independent statement of mmpose's steps, the share of
cases the derived bound leaves undecided on the GPU tests' own inputs (asserted here, so that tests/test_gpu_udp.py cannot hide
behind it), the rejection of deliberately wrong variants by the checks the GPU tests apply, the geometry properties that separate
'udp' from 'affine', and what needs no device: the option, its refusals, the call head_decode issues, the new symbols and the config."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import affine_ref as A
import dark_ref as D
import image_ref as R
import udp_ref as U
from image_ref import crop_check

J = R.J
RANDOM_CASES = [(c, hw, k, n) for c in U.UDP_CHANNELS for hw, k in U.UDP_MAPS for n in U.UDP_CROPS]
IDS = ['C%d-%dx%d-k%d-n%d' % (c, hw[0], hw[1], k, n) for c, hw, k, n in RANDOM_CASES]


def positions(idx, res, w):
    return idx // w + res['oy'], idx % w + res['ox']


def planted64(hw, k, flags):
    """(M, tiny bound, idx, cases) of the planted crops in float64: the bound is the float64 roundings' own (64 x 2^-53 |M|), so that a
    deviation of 1e-7 cell shows."""
    feat, wt, b, _, cases = U.planted_inputs(hw[0], hw[1], flags)
    n = len(cases)
    M, _ = U.reference(feat, wt, b, n, flags)
    M = np.where(np.isfinite(M), M, -1.0e30)
    return M, 64.0 * 2.0 ** -53 * np.abs(M), M.reshape(n, J, -1).argmax(2), cases


@pytest.mark.parametrize('hw,k', [p for p in U.PLANTS if p[0] != (2, 2)], ids=lambda v: str(v).replace(' ', ''))
def test_udp64_equals_the_official_steps_on_planted_blobs(hw, k):
    """Winners in every corner, on every edge and at the centre (and on the 7 x 5 map with k = 11, where the reflection bounces more
    than once: R = 5 >= both sizes - 1), plain and merged: udp64's position of the planted joint equals official_udp's (scipy's
    mirror mode, a whole-map edge pad, np.linalg.inv) to 1e-12 cell; every border winner moved."""
    h, w = hw
    for flags in U.UDP_FLAGS:
        M, bd, idx, cases = planted64(hw, k, flags)
        res = U.udp64(M, bd, idx, k)
        off = U.official_udp(M[:, 5:6], k)[:, 0]
        py, px = positions(idx, res, w)
        seen = set()
        for i, (y, x) in cases:
            assert idx[i, 5] == y * w + x
            err = max(abs(off[i, 0] - px[i, 5]), abs(off[i, 1] - py[i, 5]))
            assert err <= 1e-12, (flags, (y, x), err)
            on_border = y in (0, h - 1) or x in (0, w - 1)
            assert not on_border or max(abs(res['oy'][i, 5]), abs(res['ox'][i, 5])) > 0.4, (flags, (y, x))
            seen.add((y in (0, h - 1), x in (0, w - 1)))
        assert seen == {(True, True), (True, False), (False, True), (False, False)}
    assert (k - 1) // 2 < min(h, w) - 1 or hw == (7, 5)


def test_the_reflection_holds_for_any_distance():
    for n in (2, 3, 5, 7):
        want = np.pad(np.arange(n), (n - 1, n - 1), mode='reflect')
        got = U.reflect101(np.arange(-(n - 1), 2 * n - 1), n)
        assert np.array_equal(got, want)
        far = U.reflect101(np.arange(-40, 40), n)
        assert far.min() == 0 and far.max() == n - 1 and np.array_equal(far[40 - 2 * (n - 1):40], far[40:40 + 2 * (n - 1)])


@pytest.mark.parametrize('C_,hw,k,n', RANDOM_CASES, ids=IDS)
def test_at_most_one_percent_undecided_on_the_gpu_inputs(C_, hw, k, n):
    """On the random-blob inputs of the GPU test (udp_ref.SEED; chosen on the CPU: seeds 1 and 2 leave nothing undecided, seed 3 one
    case of C = 256, 7 x 5, 3 crops, merged with the shift), plain, merged and merged with the shift: at most 1 % of the cases are
    undecided, arg-max included; every derived bound of a decided case is at most dark_ref.CAP; udp64 equals official_udp to 1e-10."""
    h, w = hw
    for flags in U.UDP_FLAGS:
        feat, wt, b, _, _ = U.udp_inputs(C_, h, w, n, k, bool(flags & 2))
        M, bd = U.reference(feat, wt, b, n, flags)
        idx = M.reshape(n, J, -1).argmax(2)
        res = U.udp64(M, bd, idx, k)
        undecided = ~(res['decided'] & D.argmax_decided(M, bd))
        off = U.official_udp(M, k)
        py, px = positions(idx, res, w)
        err = max(float(np.abs(off[..., 0] - px).max()), float(np.abs(off[..., 1] - py).max()))
        bb = res['bound'][res['decided']]
        print('UDP64', C_, hw, k, n, flags, 'cases', int(idx.size), 'undecided', int(undecided.sum()), 'official', err,
              'bound', float(bb.min(initial=np.inf)), float(bb.max(initial=0.0)), 'B range', float(M.min()), float(M.max()))
        assert res['inside'].all()
        assert undecided.sum() <= 0.01 * idx.size, (flags, int(undecided.sum()), int(idx.size))
        assert (bb <= U.CAP).all() and err <= 1e-10
        assert D.judge(py, px, idx, res, w)['wrong'] == []
        zero = U.udp64(M, bd, idx, 0)
        assert not zero['inside'].any() and not zero['ox'].any() and not zero['oy'].any() and zero['decided'].all()


VARIANTS = ('zero_pad', 'stencil2', 'inside_rule', 'no_eps', 'clamp_dark')


@pytest.mark.parametrize('hw,k', [((64, 48), 11), ((33, 17), 17)], ids=['64x48-k11', '33x17-k17'])
def test_wrong_decoders_move_a_planted_case_by_more_than_its_bound(hw, k):
    """dark_ref.judge -- the check test_gpu_udp.py applies -- on the planted crops fails each wrong decoder on the planted joint: zero
    padding (DARK's frame), DARK's +-2 stencil, DARK's inside rule (a border winner left where it is), the Hessian without e (1e-7
    cell: the planted bound here is the float64 roundings' own), and DARK's clamp at 1e-10 (on the same maps times 200: every sample round the peak above 50)."""
    h, w = hw
    M, bd, idx, cases = planted64(hw, k, 0)
    for v in VARIANTS:
        Mv, bv = (200.0 * M, 200.0 * bd) if v == 'clamp_dark' else (M, bd)
        good = U.udp64(Mv, bv, idx, k)
        assert D.judge(*positions(idx, good, w), idx, good, w)['wrong'] == []
        assert np.isfinite(good['bound'][:, 5]).all()
        wrong = D.judge(*positions(idx, U.udp64(Mv, bv, idx, k, v), w), idx, good, w)['wrong']
        hit = sorted({a for a, c, _, _, _ in wrong if c == 5})
        print('VARIANT', hw, k, v, 'planted crops rejected', hit, 'of', len(cases))
        assert hit, v
        if v in ('zero_pad', 'inside_rule'):                   # every border and corner winner shows these two
            assert len(hit) >= len(cases) - 1, (v, hit)


def test_the_affine_mapping_and_the_affine_crop_pitch_are_rejected():
    """The / hm_w mapping moves a planted keypoint by px We (1 / (w - 1) - 1 / w) pixels, far beyond the decode bound and the float32
    rounding of the mapping; the / out_w crop pitch moves the samples of an inside box beyond crop_udp64's tolerance."""
    h, w, k = 64, 48, 11
    M, bd, idx, cases = planted64((h, w), k, 0)
    res = U.udp64(M, bd, idx, k)
    eff = A.box_cs64(R.head_inputs(D.PLANT_C, h, w, 2 * len(cases), U.SEED)[3][:len(cases)], 192, 256)
    py, px = positions(idx, res, w)
    y, x = U.map64(py, px, eff, h, w)
    yb, xb = U.map64(py, px, eff, h, w, 'hm_w')
    rows = np.stack([y, x, np.zeros_like(x)], axis=2)
    cy, cx, sy, sx = U.cells_of(rows, eff, h, w)
    assert (np.abs(cy - py) <= sy).all() and (np.abs(cx - px) <= sx).all()         # the inverse the GPU test judges with is map64's
    rows_bad = np.stack([yb, xb, np.zeros_like(x)], axis=2)
    by, bx, _, _ = U.cells_of(rows_bad, eff, h, w)
    moved = [i for i, (cy_, cx_) in cases if cx_ > 0 and abs(bx[i, 5] - px[i, 5]) > res['bound'][i, 5] + sx[i, 5]]
    assert len(moved) == sum(1 for _, (_, cx_) in cases if cx_ > 0)
    seen = 0
    for kk, (hw, res_, names, boxes) in enumerate(U.case_list()):
        val, tol = U.case_reference(kk, False)
        bad, _ = U.crop_udp64(U.case_frames(hw), U.case_view_of(len(boxes)), boxes, res_, pitch='out_w')
        assert crop_check(val, val, tol) == (0.0, 0)
        i = names.index('inside, taller')
        worst, n_bad = crop_check(bad[i:i + 1], val[i:i + 1], tol[i:i + 1])
        assert n_bad > 0 and worst > 4.0, (hw, res_, worst, n_bad)
        seen += 1
    assert seen == len(U.FRAME_SIZES) * len(U.OUTPUTS)


def test_geometry_udp_is_unbiased_where_affine_is_not():
    """Three properties the align-corners grids have and the affine ones lack: cell c and cell hm_w - 1 - c map symmetrically about the
    box centre; crop pixel u and its mirror out_w - 1 - u do; crop pixel u and heat-map cell u (hm_w - 1) / (out_w - 1) name the same
    frame position.  Dyadic numbers, so the float32 coordinates of the crop are exact and the properties hold to the last bit."""
    xe, We, W, w = 16.0, 382.0, 192, 48                         # pitches 2 (crop) and 382 / 47 (map)
    eff = np.asarray([[xe, 8.0, We, 510.0]], dtype=np.float32)
    centre = xe + We / 2
    c = np.arange(w, dtype=np.float64)[None, :]
    _, x_udp = U.map64(c * 0, c, eff, 64, w)
    _, x_aff = U.map64(c * 0, c, eff, 64, w, 'hm_w')
    assert np.abs(x_udp + x_udp[:, ::-1] - 2 * centre).max() <= 2 * R.ulp32(centre)
    assert np.abs(x_aff + x_aff[:, ::-1] - 2 * centre).min() > We / w - 1e-3
    su, _, _ = U._coords(xe, We, W)
    sa, _, _ = U._coords(xe, We, W, 'out_w')
    assert np.array_equal(su + su[::-1], np.full(W, 2 * centre))
    assert np.abs(sa + sa[::-1] - 2 * centre).min() > We / W - 1e-3
    u = np.arange(W, dtype=np.float64)
    _, x_cell = U.map64(u[None] * 0, (u * (w - 1) / (W - 1))[None], eff, 64, w)
    assert np.abs(x_cell[0] - su).max() <= R.ulp32(xe + We)
    _, x_cell_aff = U.map64(u[None] * 0, (u * w / W)[None], eff, 64, w, 'hm_w')      # the affine pair agrees with itself ...
    assert np.abs(x_cell_aff[0] - sa).max() <= R.ulp32(xe + We)
    assert np.abs(x_cell_aff[0] - su)[1:].min() > 0.01 and abs(x_cell_aff[0, -1] - su[-1]) > We / W - 1e-3      # ... and not with the UDP grid


# ---- host logic that needs no device --------------------------------------------------------------------------------------------------------
def test_udp_is_a_box_transform_and_refuses_the_quarter_step_and_the_soft_argmax():
    """check_box_transform('udp', 1.25) is accepted; post_process or soft_beta with 'udp' raises ValueError in the constructor before
    anything touches a device and at the attribute; dark, flip_test and shift_heatmap are taken; head_decode issues pam_head_decode_udp
    with decode_flags() & 3 and the blur size of dark_blur_kernel, or 0 without dark."""
    from pam import _lib, hrnet
    assert _lib.check_box_transform('udp', 1.25) == ('udp', 1.25) and 'udp' in _lib.BOX_TRANSFORMS
    for kw in (dict(post_process=True), dict(soft_beta=4.0), dict(flip_test=True, post_process=True), dict(dark=True, soft_beta=2.0)):
        with pytest.raises(ValueError):
            hrnet.HRNetPose(48, 17, None, box_transform='udp', **kw)
    for name in ('ViTPose', 'PoseResNet'):
        with pytest.raises(ValueError, match='udp'):
            hrnet.HRNetPose('B' if name == 'ViTPose' else 50, 17, None, model_name=name, resolution=(256, 192), box_transform='udp', post_process=True)
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    assert net.box_transform == 'stretch' and not net.uses_effective_box
    net.post_process = True                                      # (fine without 'udp')
    net.post_process = False
    net.box_transform = 'udp'
    assert net.uses_effective_box
    for name, value in (('post_process', True), ('soft_beta', 2.0)):
        with pytest.raises(ValueError, match='udp'):
            setattr(net, name, value)
    assert net.post_process is False and net.soft_beta is None

    class Lib(object):                                           # records the call head_decode issues
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def fn(*a):
                self.calls.append((name, a))
                return 16 if name.endswith('scratch_bytes') else 0
            return fn

    class T(object):                                             # as much of a tensor as head_decode touches
        shape = (8, 48, 64, 48); dtype = None

        def __init__(self, shape=None):
            self.shape = shape or self.shape

        def is_contiguous(self, memory_format=None):
            return True

        def data_ptr(self):
            return 4096

        def numel(self):
            return 1 << 20
    import torch
    import unittest.mock as mock
    T.dtype = torch.bfloat16
    net.lib, net.device, net._hd_scratch = Lib(), torch.device('cpu'), T()
    net.head_w, net.head_b = T((17, 48)), T((17,))
    with mock.patch.object(torch.cuda, 'current_stream', lambda d=None: mock.Mock(cuda_stream=0)):
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        name, a = net.lib.calls[-1]
        assert name == 'pam_head_decode_udp' and a[1] == 8 and a[10] == 0 and a[11] == 0, (name, a[:12])
        net.flip_test, net.dark = True, True
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        name, a = net.lib.calls[-1]
        assert name == 'pam_head_decode_udp' and a[1] == 4 and a[2] == 4 and a[10] == 3 and a[11] == 11, (name, a[:12])
        net.shift_heatmap = False
        net.head_decode(T((8, 48, 96, 72)), T(), T(), T(), T((5, 4, 17, 3)))
        name, a = net.lib.calls[-1]
        assert name == 'pam_head_decode_udp' and a[10] == 1 and a[11] == 17
        net.blur_kernel = 13
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        assert net.lib.calls[-1][1][11] == 13
        net.dark = False
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        assert net.lib.calls[-1][0] == 'pam_head_decode_udp' and net.lib.calls[-1][1][10:12] == (1, 0)
        net.box_transform = 'affine'
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        assert net.lib.calls[-1][0] == 'pam_head_decode_flip'


def test_the_three_symbols_are_declared_bound_and_refuse_bad_arguments_without_a_device():
    """pam_preprocess_crops_udp, pam_head_decode_udp and pam_head_decode_udp_scratch_bytes: declared in include/pam.h, bound in _lib,
    exported by the library; every documented PAM_E_ARG comes back before any launch; n == 0 is PAM_OK; the scratch query equals
    pam_head_decode's and refuses a map below 2 x 2."""
    from pam import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pam.h')).read()
    names = ('pam_preprocess_crops_udp', 'pam_head_decode_udp', 'pam_head_decode_udp_scratch_bytes')
    for name in names:
        assert re.search(r'\b%s\(' % name, header) and name in _lib._SIGS and name in _lib.EXPORTS
    assert _lib._SIGS['pam_head_decode_udp'] == _lib._SIGS['pam_head_decode_dark']
    assert _lib._SIGS['pam_preprocess_crops_udp'] == _lib._SIGS['pam_preprocess_crops_affine']
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pam_head_decode_udp
    fn.restype, fn.argtypes = _lib._SIGS['pam_head_decode_udp']
    p = C.c_void_p(4096)                                       # never dereferenced: every call below is refused before a launch

    def call(n=2, row0=2, h=64, w=48, Cc=48, Jn=17, flags=1, k=11):
        return fn(None, n, row0, h, w, p, Cc, p, p, Jn, flags, k, None, p, p, p, 4, p, None, p)
    for kw in (dict(k=10), dict(k=16), dict(k=7), dict(k=19), dict(k=1), dict(k=-11), dict(flags=4), dict(flags=5), dict(flags=7), dict(flags=2),
               dict(flags=8), dict(row0=1), dict(Jn=16), dict(Cc=44), dict(n=-1), dict(w=1), dict(h=1), dict(h=1, w=1), dict(w=0), dict(k=0, w=1)):
        assert call(**kw) == -1, kw
    for k in (0, 9, 11, 13, 15, 17):
        assert call(n=0, row0=0, k=k) == 0 and call(n=0, row0=0, flags=3, k=k) == 0 and call(n=0, row0=0, flags=0, k=k) == 0
    assert call(n=0, row0=0, h=2, w=2) == 0
    q = lib.pam_head_decode_udp_scratch_bytes
    q.restype, q.argtypes = _lib._SIGS['pam_head_decode_udp_scratch_bytes']
    base = lib.pam_head_decode_scratch_bytes
    base.restype, base.argtypes = _lib._SIGS['pam_head_decode_scratch_bytes']
    assert q(5, 64, 48) == base(5, 64, 48) > 0 and q(3, 2, 2) == base(3, 2, 2) and q(3, 1, 48) == -1 and q(3, 64, 1) == -1 and q(-1, 64, 48) == -1
    crop = lib.pam_preprocess_crops_udp
    crop.restype, crop.argtypes = _lib._SIGS['pam_preprocess_crops_udp']
    good = [None, 2, 2, 0, p, 100, 120, p, p, 1.25, 16, 12, 8, p, 0, p]
    bad = {1: -1, 4: None, 7: None, 8: None, 9: [0.0, -1.25, float('nan')], 10: [1, 0, -3], 11: [1, 0, -3], 12: [4, 0, 16], 13: None, 15: None}
    for at, values in bad.items():
        for val in (values if isinstance(values, list) else [values]):
            a = list(good); a[at] = val
            assert crop(*a) == -1, (at, val)
    a = list(good); a[2] = 1
    assert crop(*a) == -1                                      # n_total < n
    a = list(good); a[3] = 1; a[2] = 3
    assert crop(*a) == -1                                      # flip: n_total < 2 n
    a = list(good); a[1] = 0; a[2] = 0
    assert crop(*a) == 0                                       # nothing to do
    a[10] = a[11] = 2
    assert crop(*a) == 0                                       # 2 x 2 is the smallest output


def test_shipped_config_sets_the_protocol():
    import pam
    from pam.dataset import GetConfig
    from pam.ivclabpose import POSE_OPTIONS, box_transform_options
    root = os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf')
    p = GetConfig(os.path.join(root, 'model_configs_vitpose_b_udp.yaml')).POSE_MODELS.HRPOSE
    d = dict(p)
    assert box_transform_options(p) == ('udp', 1.25)
    assert d['FLIP_TEST'] is True and d['SHIFT_HEATMAP'] is False and d['DARK'] is True and d['BLUR_KERNEL'] == 11 and 'POST_PROCESS' not in d
    assert d['MODEL_NAME'] == 'ViTPose' and d['C'] == 'B'
    stock = dict(GetConfig(os.path.join(root, 'model_configs_vitpose_b.yaml')).POSE_MODELS.HRPOSE)
    added = {'FLIP_TEST', 'SHIFT_HEATMAP', 'DARK', 'BLUR_KERNEL', 'BOX_TRANSFORM', 'BOX_SCALE'}
    assert {k: v for k, v in d.items() if k not in added} == stock and not added & set(stock)
    # the facade's loop over POSE_OPTIONS on an object with the option set: the keys land, nothing is refused
    from pam import hrnet
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    net.box_transform = 'udp'
    for key, attr, conv, when_absent in POSE_OPTIONS:
        value = d.get(key)
        if value is not None or when_absent:
            setattr(net, attr, conv(value))
    assert net.flip_test and net.dark and not net.shift_heatmap and not net.post_process and net.decode_flags() == 1 and net.dark_blur_kernel(64) == 11
    for bad in (dict(BOX_TRANSFORM='UDP'), dict(BOX_TRANSFORM='udp', BOX_SCALE=0)):
        with pytest.raises(ValueError):
            box_transform_options(bad)
