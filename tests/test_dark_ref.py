"""CPU: the float64 restatement of the DARK decode (tests/dark_ref.py) against an independent statement of the published steps, the
share of cases the derived bound leaves undecided on the GPU tests' own inputs (asserted here, so that tests/test_gpu_dark.py cannot
hide behind it), the rejection of deliberately wrong variants by the check the GPU test applies (dark_ref.judge) on the same data, the
planted cases' expectations, and what needs no device: the option refusals of HRNetPose, the blur size default, the flag word and the
two new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dark_ref as D
import image_ref as R

J = R.J
RANDOM_CASES = [(c, hw, k, n) for c in D.DARK_CHANNELS for hw, k in D.DARK_MAPS for n in D.DARK_CROPS]
IDS = ['C%d-%dx%d-k%d-n%d' % (c, hw[0], hw[1], k, n) for c, hw, k, n in RANDOM_CASES]
_CACHE = {}


def case64(C_, hw, n, flags):
    """(M, bound, idx) of one random-blob case and flag word, computed once and left unchanged."""
    key = (C_, hw, n, flags)
    if key not in _CACHE:
        if (C_, hw, n) not in _CACHE:
            _CACHE[(C_, hw, n)] = D.dark_inputs(C_, hw[0], hw[1], n)
        feat, wt, b, _, _ = _CACHE[(C_, hw, n)]
        M, bd = D.reference(feat, wt, b, n, flags)
        _CACHE[key] = (M, bd, M.reshape(n, J, -1).argmax(2))
    return _CACHE[key]


def positions(idx, res, w):
    return idx // w + res['oy'], idx % w + res['ox']


@pytest.mark.parametrize('C_,hw,k,n', RANDOM_CASES, ids=IDS)
def test_dark64_equals_the_official_steps_and_leaves_at_most_one_percent_undecided(C_, hw, k, n):
    """On the random-blob inputs of the GPU test, plain, merged and merged with the shift: dark64's position equals official_dark's
    (full-map blur through scipy, the max(M) / max(B) rescaling, a matrix inverse) to 1e-10 cell on every inside case; at most 1 % of
    the inside cases are undecided (dark_ref.SEED: none), arg-max included; every derived bound of a decided case is at most 2e-3."""
    h, w = hw
    for flags in D.DARK_FLAGS:
        M, bd, idx = case64(C_, hw, n, flags)
        res = D.dark64(M, bd, idx, k)
        ins = res['inside']
        off = D.official_dark(M, k)
        py, px = positions(idx, res, w)
        err = max(float(np.abs(off[..., 0] - px).max()), float(np.abs(off[..., 1] - py).max()))
        assert err <= 1e-10, (flags, err)
        undecided = ins & ~(res['decided'] & D.argmax_decided(M, bd))
        bb = res['bound'][ins & res['decided']]
        print('DARK64', C_, hw, k, n, flags, 'inside', int(ins.sum()), 'undecided', int(undecided.sum()), 'official', err,
              'bound', float(bb.min(initial=np.inf)), float(bb.max(initial=0.0)))
        assert undecided.sum() <= 0.01 * ins.sum(), (flags, int(undecided.sum()), int(ins.sum()))
        assert (bb <= D.CAP).all()
        assert D.judge(py, px, idx, res, w)['wrong'] == []
        assert not res['ox'][~ins].any() and not res['oy'][~ins].any()
    assert C_ != 32 or n != 3 or hw == (7, 5) or ins.sum() > 17              # the blobs lie anywhere: most are inside, some are not


VARIANTS = ('no_blur', 'argmax_after_blur', 'loose_border', 'reflect', 'taps17', 'no_log', 'dxy_sign')


@pytest.mark.parametrize('C_,hw,k', [(48, (96, 72), 17), (256, (64, 48), 11), (32, (33, 17), 11)])
def test_wrong_decoders_are_rejected_by_the_gpu_check_on_the_gpu_inputs(C_, hw, k):
    """dark_ref.judge -- the check test_gpu_dark.py applies -- on the GPU test's random-blob inputs (3 crops) fails each wrong decoder:
    the blur left out, the arg-max taken after the blur, the quarter rule's border test (px < w - 1: the planted border cases show it
    where the random ones do not), reflect padding instead of zeros (shows only near an edge), k = 17's taps at k = 11 (at k = 17
    itself: 11's taps, the same mistake the other way), the Taylor step without the logarithm, dxy with the sign flipped; and, merged,
    the window without the joint swap and the unshifted column under the shift."""
    h, w = hw
    M, bd, idx = case64(C_, hw, 3, 0)
    good = D.dark64(M, bd, idx, k)
    assert D.judge(*positions(idx, good, w), idx, good, w)['wrong'] == []
    for v in VARIANTS:
        if v == 'argmax_after_blur':
            idx2 = D.blur64(M, D.taps(k)).reshape(3, J, -1).argmax(2)
            py, px = positions(idx2, D.dark64(M, bd, idx2, k), w)
            moved = int((idx2 != idx).sum())
        elif v == 'taps17' and k == 17:
            py, px = positions(idx, D.dark64(M, bd, idx, 11), w); moved = None
        else:
            py, px = positions(idx, D.dark64(M, bd, idx, k, v), w); moved = None
        wrong = D.judge(py, px, idx, good, w)['wrong']
        print('VARIANT', C_, hw, k, v, len(wrong), 'of', int(good['inside'].sum()), moved)
        if v == 'argmax_after_blur':                             # every winner the blur moves is a failure (the others decode alike)
            cells = {(a, c) for a, c, _, _, _ in wrong}
            assert moved > 0 and all((a, c) in cells for a, c in zip(*np.nonzero(idx2 != idx))), (v, moved, len(wrong))
            continue
        if v == 'loose_border':
            continue                                             # differs only for winners at px = w - 2 / py = h - 2: the planted cases below
        if v == 'reflect':
            near = D.inside_of(idx, h, w) & ((idx % w < (k - 1) // 2 + 2) | (idx % w >= w - (k - 1) // 2 - 2) |
                                            (idx // w < (k - 1) // 2 + 2) | (idx // w >= h - (k - 1) // 2 - 2))
            assert near.sum() > 0 and len(wrong) >= 0.5 * near.sum(), (v, len(wrong), int(near.sum()))
            continue
        assert len(wrong) > 0.5 * good['inside'].sum(), (v, len(wrong))
    for flags, variant, wrong_flags in ((1, 'no_swap', 1), (3, 'no_swap', 3), (3, 'ok', 1)):
        Mg, bg, ig = case64(C_, hw, 3, flags)
        feat, wt, b, _, _ = _CACHE[(C_, hw, 3)]
        Mw, bw = D.reference(feat, wt, b, 3, wrong_flags, variant)
        iw = Mw.reshape(3, J, -1).argmax(2)
        ref = D.dark64(Mg, bg, ig, k)
        wrong = D.judge(*positions(iw, D.dark64(Mw, bw, iw, k), w), ig, ref, w)['wrong']
        print('VARIANT', C_, hw, k, 'merge', flags, variant, wrong_flags, len(wrong), 'of', int(ref['inside'].sum()))
        assert len(wrong) > 0.5 * ref['inside'].sum(), (flags, variant, len(wrong))


PLANTS = [((96, 72), 17), ((64, 48), 11), ((33, 17), 11), ((33, 17), 17), ((7, 5), 11)]


@pytest.mark.parametrize('hw,k', PLANTS, ids=['%dx%d-k%d' % (hw[0], hw[1], k) for hw, k in PLANTS])
def test_planted_cases_pin_what_they_say(hw, k):
    """The planted inputs of the GPU test in float64, for flags 0, 1 and 3: every expectation a case carries holds for the restatement
    (the winner's cell, which side of the inside rule it is on, a non-zero decided offset inside, the spike's exact zero, the mirrored
    crop's blob in joint 6 at a column that reads it); joint 7 is a map of -inf; the quarter rule's border test moves a winner at
    px = w - 2 / py = h - 2 that the rule leaves alone, and judge rejects it; the two-sided overhang and the tile seam are really there."""
    h, w = hw
    R_ = (k - 1) // 2
    for flags in D.DARK_FLAGS:
        feat, wt, b, boxes, cases = D.planted_inputs(h, w, k, flags)
        n = len(cases)
        M, bd = D.reference(feat, wt, b, n, flags)
        idx = M.reshape(n, J, -1).argmax(2)
        res = D.dark64(M, bd, idx, k)
        am = D.argmax_decided(M, bd)
        assert np.isneginf(M[:, 7]).all() and (idx[:, 7] == 0).all() and not res['inside'][:, 7].any()
        loose = D.dark64(M, bd, idx, k, 'loose_border')
        rejected = D.judge(*positions(idx, loose, w), idx, res, w)['wrong']
        moved = 0
        for i, name, e in cases:
            j, where = e['joint'], (name, flags)
            assert am[i, j], where
            if 'among' in e:
                assert idx[i, j] in e['among'], where
                continue
            assert idx[i, j] == e['cell'], where
            assert bool(res['inside'][i, j]) == e['inside'], where
            if e.get('zero'):
                assert res['decided'][i, j] and res['ox'][i, j] == 0 and res['oy'][i, j] == 0 and res['bound'][i, j] == 0, where
                assert M[i, j].max() > 0 and np.sort(M[i, j].ravel())[-2] < -20, where
            elif name == 'plateau':                              # pins the tie rule alone: on the square's corner the Hessian is close
                print('PLANTED', hw, k, flags, name, 'decided', bool(res['decided'][i, j]), 'bound', float(res['bound'][i, j]))   # to singular
            elif e['inside']:
                assert res['decided'][i, j] and res['bound'][i, j] <= D.CAP, where
                assert abs(res['ox'][i, j]) + abs(res['oy'][i, j]) > 10 * res['bound'][i, j], where
            else:
                assert res['ox'][i, j] == 0 and res['oy'][i, j] == 0, where
                if loose['inside'][i, j]:
                    moved += 1
                    assert any(a == i and c == j for a, c, _, _, _ in rejected), where
            if 'centre' in e and e['inside']:
                cy, cx = e['centre']
                py, px = idx[i, j] // w + res['oy'][i, j], idx[i, j] % w + res['ox'][i, j]
                print('PLANTED', hw, k, flags, name, 'centre', (cy, cx), 'decoded', (float(py), float(px)))
                assert flags != 0 or (abs(py - cy) < 0.25 and abs(px - cx) < 0.25), where       # (the background moves it a little)
                assert 2 * R_ + 5 <= w or (px - R_ - 2 < 0 and px + R_ + 2 > w - 1)
                y0, y1 = idx[i, j] // w - R_ - 2, idx[i, j] // w + R_ + 2
                assert h * w <= R.HEAD_TILE or (max(y0, 0) * w) // R.HEAD_TILE < (min(y1, h - 1) * w + w - 1) // R.HEAD_TILE
            if 'tile' in e:
                assert idx[i, j] // R.HEAD_TILE == e['tile'], where
        assert moved >= 2 or min(h, w) < 7, (flags, moved)
    assert (2 * R_ + 5 > w) == ((hw, k) in (((33, 17), 17), ((7, 5), 11)))


def test_the_scale_free_form_and_the_official_rescaling():
    """The stated deviation: on the random-blob maps (max(M) > 0, every blurred sample far above 1e-10) leaving max(M) / max(B) out
    changes nothing beyond rounding (the first test: 1e-10); on the lone spike of a negative map the official scale is negative and
    un-clamps the map, so official_dark moves the keypoint while the scale-free definition leaves it where it is."""
    h, w, k = 33, 17, 11
    feat, wt, b, boxes, cases = D.planted_inputs(h, w, k, 0)
    n = len(cases)
    M, bd = D.reference(feat, wt, b, n, 0)
    i = [c for c, name, _ in cases if name == 'spike'][0]
    idx = M.reshape(n, J, -1).argmax(2)
    res = D.dark64(M, bd, idx, k)
    with np.errstate(invalid='ignore', divide='ignore'):
        off = D.official_dark(np.where(np.isfinite(M), M, -1e30)[i:i + 1, 9:10], k)[0, 0]
    assert res['ox'][i, 9] == 0 and res['oy'][i, 9] == 0
    assert abs(off[0] - idx[i, 9] % w) + abs(off[1] - idx[i, 9] // w) > 1e-3


def test_taps_are_opencvs():
    """sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8: 2.0 at 11, 2.9 at 17 (OpenCV's rule; not 3.0); the taps sum to 1, are symmetric, and sizes below 9 or even are refused."""
    assert abs(D.sigma_of(11) - 2.0) < 1e-15 and abs(D.sigma_of(17) - 2.9) < 1e-15
    for k in (9, 11, 13, 15, 17):
        g = D.taps(k)
        assert g.size == k and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == (k - 1) // 2
    assert abs(D.taps(11)[5] / D.taps(11)[4] - np.exp(1.0 / 8.0)) < 1e-14
    for k in (7, 10, 19):
        with pytest.raises(AssertionError):
            D.taps(k)


# ---- host logic that needs no device --------------------------------------------------------------------------------------------------------
def test_dark_option_refusals_default_blur_size_and_flag_word_need_no_device():
    """dark with post_process or soft_beta raises ValueError, in the constructor before anything touches a device and at the attribute
    whichever is set last; blur_kernel None means 17 for a (96, 72) map and 11 for a (64, 48) one, and takes only odd sizes 9 .. 17;
    head_decode passes decode_flags() & 3."""
    from pam import hrnet
    for kw in (dict(post_process=True), dict(soft_beta=4.0), dict(flip_test=True, post_process=True)):
        with pytest.raises(ValueError, match='dark'):
            hrnet.HRNetPose(48, 17, None, dark=True, **kw)
    for bad in (7, 10, 19, 11.5):
        with pytest.raises(ValueError, match='blur_kernel'):
            hrnet.HRNetPose(48, 17, None, dark=True, blur_kernel=bad)
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    assert net.dark is False and net.blur_kernel is None
    assert net.dark_blur_kernel(96) == 17 and net.dark_blur_kernel(64) == 11 and net.dark_blur_kernel(128) == 17 and net.dark_blur_kernel(95) == 11
    net.blur_kernel = 13
    assert net.dark_blur_kernel(96) == 13 and net.dark_blur_kernel(64) == 13
    with pytest.raises(ValueError):
        net.blur_kernel = 8
    net.blur_kernel = None
    net.dark = True
    for name, value in (('post_process', True), ('soft_beta', 2.0)):
        with pytest.raises(ValueError):
            setattr(net, name, value)
    assert net.decode_flags() & 3 == 0
    net.flip_test = True
    assert net.decode_flags() & 3 == 3 and net.forward_crops(5) == 10
    net.shift_heatmap = False
    assert net.decode_flags() & 3 == 1
    net.dark = False
    net.post_process = True
    with pytest.raises(ValueError):
        net.dark = True
    assert net.dark is False and net.decode_flags() == 5

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
    T.dtype = torch.bfloat16
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    net.lib, net.device, net._hd_scratch = Lib(), torch.device('cpu'), T()
    net.head_w, net.head_b = T((17, 48)), T((17,))
    net.flip_test, net.dark = True, True
    import unittest.mock as mock
    with mock.patch.object(torch.cuda, 'current_stream', lambda d=None: mock.Mock(cuda_stream=0)):
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        name, a = net.lib.calls[-1]
        assert name == 'pam_head_decode_dark' and a[1] == 4 and a[2] == 4 and a[10] == 3 and a[11] == 11, (name, a[:12])
        net.shift_heatmap = False
        net.head_decode(T((8, 48, 96, 72)), T(), T(), T(), T((5, 4, 17, 3)))
        name, a = net.lib.calls[-1]
        assert name == 'pam_head_decode_dark' and a[10] == 1 and a[11] == 17
        net.dark = False
        net.head_decode(T(), T(), T(), T(), T((5, 4, 17, 3)))
        assert net.lib.calls[-1][0] == 'pam_head_decode_flip' and net.lib.calls[-1][1][10] == 1


def test_the_two_symbols_are_declared_bound_and_refuse_bad_arguments_without_a_device():
    """pam_head_decode_dark and pam_head_decode_dark_scratch_bytes: declared in include/pam.h, bound in _lib, exported by the library;
    an even k, k = 7, k = 19, the QUARTER flag, SHIFT without MERGE and MERGE with flip_row0 < n give PAM_E_ARG before any launch;
    n == 0 is PAM_OK; the scratch query equals pam_head_decode's."""
    from pam import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pam.h')).read()
    for name in ('pam_head_decode_dark', 'pam_head_decode_dark_scratch_bytes'):
        assert re.search(r'\b%s\(' % name, header) and name in _lib._SIGS and name in _lib.EXPORTS
    assert len(_lib._SIGS['pam_head_decode_dark'][1]) == len(_lib._SIGS['pam_head_decode_flip'][1]) + 1
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pam_head_decode_dark
    fn.restype, fn.argtypes = _lib._SIGS['pam_head_decode_dark']
    p = C.c_void_p(4096)                                       # never dereferenced: every call below is refused before a launch

    def call(n=2, row0=2, Cc=48, Jn=17, flags=1, k=11):
        return fn(None, n, row0, 64, 48, p, Cc, p, p, Jn, flags, k, None, p, p, p, 4, p, None, p)
    for kw in (dict(k=10), dict(k=16), dict(k=7), dict(k=19), dict(k=0), dict(k=-11), dict(flags=4), dict(flags=5), dict(flags=7), dict(flags=2),
               dict(flags=8), dict(row0=1), dict(Jn=16), dict(Cc=44), dict(n=-1)):
        assert call(**kw) == -1, kw
    for k in (9, 11, 13, 15, 17):
        assert call(n=0, row0=0, k=k) == 0 and call(n=0, row0=0, flags=3, k=k) == 0 and call(n=0, row0=0, flags=0, k=k) == 0
    q = lib.pam_head_decode_dark_scratch_bytes
    q.restype, q.argtypes = _lib._SIGS['pam_head_decode_dark_scratch_bytes']
    assert q(3, 33, 17) == 3 * 3 * 17 * 8 and q(-1, 1, 1) == -1
