"""CPU: the float64 restatement of the flip test (tests/flip_ref.py) against an independent torch statement of the official steps, the
rejection of deliberately wrong variants on the GPU tests' own inputs, the share of maps the float32 bound leaves undecided on those
inputs (asserted here, so that tests/test_gpu_flip.py cannot hide behind it), and the refusals that need no device: option
combinations of HRNetPose and flag combinations of pam_head_decode_flip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import flip_ref as FR
import image_ref as R

J = R.J
RANDOM_CASES = [(c, hw, n) for c in FR.FLIP_CHANNELS for hw in FR.FLIP_MAPS for n in FR.FLIP_CROPS]
_CACHE = {}


def case64(C_, hw, n):
    """(hmP, bdP, hmF, bdF, boxes) of one random case, computed once."""
    key = (C_, hw, n)
    if key not in _CACHE:
        feat, wt, b, boxes = FR.flip_inputs(C_, hw[0], hw[1], n)
        _CACHE[key] = FR.maps64(feat, wt, b, n) + (boxes,)
    return _CACHE[key]


def flat(a):
    return a.reshape(a.shape[0], J, -1)


def test_merge64_and_quarter64_equal_the_official_steps_on_random_maps():
    """flip(3), channel swap, [..., 1:] = clone[..., :-1], average, floor(coord + 0.5) and the 1 < px < W - 1 test in torch float64
    against merge64 / quarter64: exact agreement, shift on and off, odd and even widths."""
    rng = np.random.default_rng(0)
    for h, w in ((7, 5), (12, 8), (33, 17)):
        P, F = rng.standard_normal((3, J, h, w)), rng.standard_normal((3, J, h, w))
        zero = np.zeros_like(P)
        for shift in (False, True):
            M, _ = FR.merge64(P, zero, F, zero, shift)
            T = FR.official_merge(torch.from_numpy(P), torch.from_numpy(F), shift)
            assert np.array_equal(M, T.numpy()), (h, w, shift)
            idx = flat(M).argmax(2)
            inside, sx, sy, dx, dy = FR.quarter64(M, np.zeros_like(M), idx)
            assert dx.all() and dy.all()                       # zero bounds: every sign of a random map is decided
            want = FR.official_offsets(T)
            assert np.array_equal(want[:, :, 0], idx % w + 0.25 * sx) and np.array_equal(want[:, :, 1], idx // w + 0.25 * sy)
            assert inside.any() and not inside.all()


def test_source_columns():
    assert FR.source_columns(5, False).tolist() == [4, 3, 2, 1, 0]
    assert FR.source_columns(5, True).tolist() == [4, 4, 3, 2, 1]              # column 0 keeps its own value; column 0 of the mirror is dropped
    assert FR.PAIR[FR.PAIR].tolist() == list(range(J)) and FR.PAIR[0] == 0 and FR.PAIR[5] == 6
    assert [[j, int(FR.PAIR[j])] for j in range(1, J, 2)] == FR.FLIP_PAIRS


@pytest.mark.parametrize('C_,hw,n', RANDOM_CASES, ids=['C%d-%dx%d-n%d' % (c, hw[0], hw[1], n) for c, hw, n in RANDOM_CASES])
def test_undecided_share_of_the_gpu_cases(C_, hw, n):
    """On the inputs of test_gpu_flip.py's random cases the float32 bound leaves at most 1 % of the maps undecided (flip_ref.SEED: none), merged
    with and without the shift and unmerged (flags 4); the count of undecided quarter-pixel signs is printed."""
    hmP, bdP, hmF, bdF, _ = case64(C_, hw, n)
    for name, (M, bd) in (('merge', FR.merge64(hmP, bdP, hmF, bdF, False)), ('merge+shift', FR.merge64(hmP, bdP, hmF, bdF, True)),
                          ('plain', (hmP, bdP))):
        idx = flat(M).argmax(2)
        res = R.argmax_check(flat(M), flat(bd), idx)
        _, _, _, dx, dy = FR.quarter64(M, bd, idx)
        print('UNDECIDED', C_, hw, n, name, res['undecided'], 'of', res['maps'], 'signs', int((~dx).sum() + (~dy).sum()))
        assert res['wrong'] == [] and res['undecided'] <= 0.01 * res['maps'], (name, res['undecided'])


@pytest.mark.parametrize('C_,hw', [(48, (33, 17)), (256, (64, 48)), (32, (7, 5))])
def test_wrong_merges_are_rejected_on_the_gpu_inputs(C_, hw):
    """The arg-max of a wrong merge -- no joint swap, no shift where one is asked, the shift the other way, a circular shift at x = 0 --
    fails argmax_check against merge64's map and bound on the random inputs of the GPU test.  (The issue words the last variant as
    'xs = w - 1 - x at x = 0', which IS the rule: column 0 keeps its own value w - 1.  The variant tested is the one that differs at
    x = 0, the wrap-around of the x >= 1 rule.)"""
    hmP, bdP, hmF, bdF, _ = case64(C_, hw, 3)
    M, bd = FR.merge64(hmP, bdP, hmF, bdF, True)
    good = R.argmax_check(flat(M), flat(bd), flat(M).argmax(2))
    assert good['wrong'] == []
    for variant, shift in (('no_swap', True), ('ok', False), ('other_direction', True), ('x0_wrap', True)):
        W, _ = FR.merge64(hmP, bdP, hmF, bdF, shift, variant)
        res = R.argmax_check(flat(M), flat(bd), flat(W).argmax(2))
        if variant == 'x0_wrap':                               # differs in column 0 alone: the maps that peak there must fail
            col0 = [(a, j) for a in range(3) for j in range(J) if flat(W)[a, j].argmax() % hw[1] == 0 or flat(M)[a, j].argmax() % hw[1] == 0]
            diff = [(a, j) for a, j in col0 if flat(W)[a, j].argmax() != flat(M)[a, j].argmax()]
            assert {(a, j) for a, j, _, _ in res['wrong']} == set(diff)
        else:
            assert len(res['wrong']) > 0.5 * res['maps'], (variant, len(res['wrong']))
    # and without the shift, the swap alone
    M0, bd0 = FR.merge64(hmP, bdP, hmF, bdF, False)
    W0, _ = FR.merge64(hmP, bdP, hmF, bdF, False, 'no_swap')
    assert len(R.argmax_check(flat(M0), flat(bd0), flat(W0).argmax(2))['wrong']) > 0.5 * 3 * (J - 1)


@pytest.mark.parametrize('hw', FR.PLANT_MAPS)
def test_planted_cases_pin_what_they_say(hw):
    """The planted inputs of the GPU test in float64: every expectation a case carries holds for the correct restatement (the peak of
    the mirrored crop appears in joint 6 at the column(s) that read it, the seam tie is exact and the lower index wins, the border
    peaks are inside exactly where 1 < px < w - 1 and 1 < py < h - 1, equal neighbours give no offset, the mirrored crop alone orders a
    neighbour pair), a circular shift at x = 0 and the <= border test are rejected on them, and joint 7 is a map of -inf."""
    h, w = hw
    for shift in (False, True):
        feat, wt, b, boxes, cases = FR.planted_inputs(h, w, shift)
        n = len(cases)
        for weights in ('main', 'tie'):
            wt_, b_ = FR.tie_weights(wt, b) if weights == 'tie' else (wt, b)
            hmP, bdP, hmF, bdF = FR.maps64(feat, wt_, b_, n)
            M, bd = FR.merge64(hmP, bdP, hmF, bdF, shift)
            idx = flat(M).argmax(2)
            res = R.argmax_check(flat(M), flat(bd), idx)
            assert res['wrong'] == [] and res['undecided'] <= 0.01 * res['maps']
            inside, sx, sy, dx, dy = FR.quarter64(M, bd, idx)
            assert np.isneginf(M[:, 7]).all() and (idx[:, 7] == 0).all() and not inside[:, 7].any()
            for i, name, e in cases:
                j = e['joint']
                if (name == 'tie') != (weights == 'tie'):
                    continue
                if 'among' in e:
                    assert (idx[i, j] in e['among']) == bool(e['among']), (name, shift)
                    if e['among']:
                        assert abs(M[i, j].max() - 0.5 * hmF[i, 5].max()) < 4.0 and hmF[i, 5].max() > 30.0       # half height
                if 'cell' in e:
                    assert idx[i, j] == e['cell'], (name, shift)
                if 'tie' in e:
                    assert flat(M)[i, j, e['tie']] == flat(M)[i, j, e['cell']] and e['tie'] // R.HEAD_TILE == e['cell'] // R.HEAD_TILE + 1
                if 'inside' in e:
                    assert bool(inside[i, j]) == e['inside'], (name, shift)
                if 'dx' in e:
                    assert sx[i, j] == e['dx'] and inside[i, j] and (dx[i, j] or e['dx'] == 0), (name, shift)
        # the <= border test moves the peaks at px = 1 / w - 2 ... that the strict test leaves alone: a decided non-zero sign there
        loose = FR.quarter64(M, bd, idx, strict=False)
        moved = [(i, name) for i, name, e in cases if 'inside' in e and not e['inside'] and loose[0][i, 5]
                 and ((loose[1][i, 5] != 0 and loose[3][i, 5]) or (loose[2][i, 5] != 0 and loose[4][i, 5]))]
        assert len(moved) >= 2, moved
        if shift:                                              # the peak in the mirrored crop's column 0 shows under a circular shift only
            W, _ = FR.merge64(hmP, bdP, hmF, bdF, True, 'x0_wrap')
            bad = R.argmax_check(flat(M), flat(bd), flat(W).argmax(2))['wrong']
            assert any(a == 1 and j == 6 for a, j, _, _ in bad), bad


def test_refused_option_combinations_need_no_device():
    """soft_beta with flip_test or post_process raises ValueError: in the constructor before anything touches a device, and at the
    attribute whichever is set last."""
    from pam import hrnet
    for kw in (dict(flip_test=True), dict(post_process=True), dict(flip_test=True, post_process=True)):
        with pytest.raises(ValueError, match='soft_beta'):
            hrnet.HRNetPose(48, 17, None, soft_beta=4.0, **kw)
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    assert (net.flip_test, net.shift_heatmap, net.post_process, net.soft_beta, net.decode_flags()) == (False, True, False, None, 0)
    net.soft_beta = 4.0
    for name in ('flip_test', 'post_process'):
        with pytest.raises(ValueError):
            setattr(net, name, True)
    net.soft_beta = None
    net.flip_test = True
    assert net.decode_flags() == 3 and net.forward_crops(5) == 10
    net.post_process = True
    with pytest.raises(ValueError):
        net.soft_beta = 2.0
    net.shift_heatmap = False
    assert net.decode_flags() == 5
    net.flip_test = False
    assert net.decode_flags() == 4 and net.forward_crops(5) == 5


def test_flag_and_argument_refusals_of_the_abi_need_no_device():
    """pam_head_decode_flip / pam_preprocess_crops_flip check their arguments before any launch: shift without merge, unknown bits, the
    mirrored rows in front of row n, a joint count other than 17, channels not a multiple of 8, fewer than 2n rows -> PAM_E_ARG (-1);
    the scratch query equals pam_head_decode's."""
    from pam import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pam_head_decode_flip
    fn.restype, fn.argtypes = _lib._SIGS['pam_head_decode_flip']
    p = C.c_void_p(4096)                                       # never dereferenced: every call below is refused before a launch

    def call(n=2, row0=2, Cc=48, Jn=17, flags=1):
        return fn(None, n, row0, 64, 48, p, Cc, p, p, Jn, flags, None, p, p, p, 4, p, None, p)
    for kw in (dict(flags=2), dict(flags=6), dict(flags=8), dict(flags=15), dict(flags=-1), dict(row0=1), dict(row0=1, flags=7), dict(Jn=16),
               dict(Cc=44), dict(n=-1)):
        assert call(**kw) == -1, kw
    assert call(n=0, row0=0) == 0 and call(n=0, row0=0, flags=7) == 0         # nothing to do: no launch either
    q = lib.pam_head_decode_flip_scratch_bytes
    q.restype, q.argtypes = _lib._SIGS['pam_head_decode_flip_scratch_bytes']
    ref = lib.pam_head_decode_scratch_bytes
    ref.restype, ref.argtypes = _lib._SIGS['pam_head_decode_scratch_bytes']
    assert q(3, 33, 17) == ref(3, 33, 17) == 3 * 3 * 17 * 8 and q(-1, 1, 1) == -1
    pre = lib.pam_preprocess_crops_flip
    pre.restype, pre.argtypes = _lib._SIGS['pam_preprocess_crops_flip']
    assert pre(None, 3, 5, p, 10, 10, p, p, 8, 8, 3, p, 0) == -1                # n_total < 2n
    assert pre(None, 3, 6, p, 10, 10, p, p, 8, 8, 4, p, 0) == -1                # out_c
    assert pre(None, 0, 0, p, 10, 10, p, p, 8, 8, 3, p, 0) == 0
