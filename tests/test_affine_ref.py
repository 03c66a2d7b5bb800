"""CPU: the pose checkpoints' centre/scale box transform -- pam_box_cs_host against the float64 restatement of tests/affine_ref.py bit
for bit, the transform's properties, known answers of the crop restatement warp64, and the proof that warp64's derived tolerance
rejects each wrong restatement one could plant in the kernel, on the inputs the GPU test uses -- plus the shipped config's keys."""
import os

import numpy as np
import pytest

import affine_ref as A
from image_ref import MEAN, STD, crop_check
from pam import _lib

RES = ((16, 12), (64, 48), (256, 192), (384, 288))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def edge_boxes():
    out = []
    for hw in A.FRAME_SIZES:
        for res in RES:
            out += [b for _, b in A.case_boxes(hw, res)]
    out += [[0, 0, 12, 16], [3, 4, 3e38, 1], [3, 4, 1, 3e38], [1e30, -1e30, 5, 5], [7, 7, -4, 9], [7, 7, 9, -4], [7, 7, -4, -9],
            [5, 5, 1e-44, 1e-44], [5, 5, float('inf'), 3], [float('nan'), 2, 3, 4], [2, float('nan'), 3, 4]]
    return np.asarray(out, dtype=np.float32)


@pytest.mark.parametrize('res', RES)
@pytest.mark.parametrize('scale', (1.25, 1.0, 1.1))
def test_host_entry_equals_the_restatement_bit_for_bit(res, scale):
    H, W = res
    rng = np.random.default_rng([5, H, W])
    rnd = np.concatenate([rng.random((5000, 4)) * [2000, 1200, 600, 900] - [100, 100, 0, 0],
                          rng.random((3000, 4)) * [100, 100, 40, 40] - [20, 20, 0, 0],
                          rng.integers(0, 64, (2000, 4)).astype(np.float64) * [1, 1, 3, 4]]).astype(np.float32)   # many exact ties of the aspect
    assert len(rnd) == 10000
    for boxes in (edge_boxes(), rnd):
        got = _lib.box_cs(boxes, W, H, scale)
        want = A.box_cs64(boxes, W, H, scale)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), np.nonzero((bits(got) != bits(want)).any(1))[0][:5]


def test_host_entry_argument_errors():
    lib = _lib.load()
    b = np.zeros((2, 4), dtype=np.float32); e = np.zeros((2, 4), dtype=np.float32)
    p = lambda a: a.ctypes.data
    assert lib.pam_box_cs_host(2, p(b), 12, 16, 1.25, p(e)) == 0
    assert lib.pam_box_cs_host(0, None, 12, 16, 1.25, None) == 0
    for args in ((-1, p(b), 12, 16, 1.25, p(e)), (2, None, 12, 16, 1.25, p(e)), (2, p(b), 12, 16, 1.25, None), (2, p(b), 0, 16, 1.25, p(e)),
                 (2, p(b), 12, 0, 1.25, p(e)), (2, p(b), 12, 16, 0.0, p(e)), (2, p(b), 12, 16, -1.0, p(e)), (2, p(b), 12, 16, float('nan'), p(e))):
        assert lib.pam_box_cs_host(*args) == -1, args
    with pytest.raises(ValueError):
        _lib.check_box_transform('letterbox')
    with pytest.raises(ValueError):
        _lib.check_box_transform('affine', 0.0)
    assert _lib.check_box_transform(None, None) == ('stretch', 1.25) and _lib.check_box_transform('affine', 1.1) == ('affine', 1.1)


@pytest.mark.parametrize('res', RES)
def test_transform_properties(res):
    H, W = res
    rng = np.random.default_rng([6, H, W])
    b = (rng.random((2000, 4)) * [1500, 900, 500, 700] + [0, 0, 1, 1]).astype(np.float32)
    for scale in (1.25, 1.0):
        e = A.box_cs64(b, W, H, scale).astype(np.float64)
        bd = b.astype(np.float64)
        cx, cy = bd[:, 0] + bd[:, 2] * 0.5, bd[:, 1] + bd[:, 3] * 0.5
        # the centre is preserved: xe + We / 2 is cx up to the float32 roundings of xe and We
        ulp = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(e[:, 0] + e[:, 2] * 0.5 - cx) <= ulp(e[:, 0]) * 0.5 + ulp(e[:, 2]) * 0.25 + 1e-12)
        assert np.all(np.abs(e[:, 1] + e[:, 3] * 0.5 - cy) <= ulp(e[:, 1]) * 0.5 + ulp(e[:, 3]) * 0.25 + 1e-12)
        # We / He = out_w / out_h within 1 float32 ulp, taken as the format's relative spacing 2^-23: We and He are each one rounding
        # (relative 2^-24) away from numbers in exactly that ratio.  (The absolute spacing AT 0.75 is 2^-24, two thirds of that: a bound
        # no pair of correctly rounded extents can promise, 0.75 lying in the upper half of its binade.)
        assert np.all(np.abs(e[:, 2] / e[:, 3] / (W / H) - 1.0) <= 2.0 ** -23)
        # the aspect-fixed box: the raw box with the short side grown, never shrunk; area = scale^2 x its area
        fw_, fh_ = np.maximum(bd[:, 2], bd[:, 3] * W / H), np.maximum(bd[:, 3], bd[:, 2] * H / W)
        assert np.allclose(e[:, 2] * e[:, 3], scale * scale * fw_ * fh_, rtol=4 * 2.0 ** -24, atol=0)
        # the effective box contains the raw one (scale >= 1), up to the roundings of its own corners
        slack = ulp(e[:, 0]) + ulp(e[:, 2]) + ulp(e[:, 1]) + ulp(e[:, 3])
        assert np.all(e[:, 0] <= bd[:, 0] + slack) and np.all(e[:, 1] <= bd[:, 1] + slack)
        assert np.all(e[:, 0] + e[:, 2] >= bd[:, 0] + bd[:, 2] - slack) and np.all(e[:, 1] + e[:, 3] >= bd[:, 1] + bd[:, 3] - slack)
    # degenerate boxes: (x, y, 0, 0)
    d = A.box_cs64([[3, 4, 0, 0], [3, 4, float('nan'), 5], [3, 4, -2, -3]], W, H)
    assert np.array_equal(d[0], [3, 4, 0, 0]) and np.array_equal(d[1], [3, 4, 0, 0])
    assert d[2, 2] == 0 and d[2, 3] == 0            # both extents negative: We < 0
    # exactly at the aspect: both extents kept, scaled
    t = A.box_cs64([[10, 8, 12, 16]], W, H, 1.25)[0]
    assert np.array_equal(t, np.float32([10 + 6 - 7.5, 8 + 8 - 10, 15, 20]))


def normalised(frame_rgb):
    return (np.asarray(frame_rgb, dtype=np.float64) / 255.0 - MEAN) / STD


def test_identity_known_answer_and_the_zero_border():
    """A box at the aspect with scale 1, We = out_w and integer xe, ye inside the frame reads the frame's own pixels: warp64 returns
    exactly their normalised values; moved one pixel past an edge the column (row) outside is exactly the normalised value of 0."""
    hw = A.FRAME_SIZES[0]
    fr = A.case_frames(hw)
    H, W = 16, 12
    val, tol = A.warp64(fr, [0, 1], [[5, 7, W, H], [hw[1] - W, hw[0] - H, W, H]], (H, W), scale=1.0)
    for i, (v, x, y) in enumerate(((0, 5, 7), (1, hw[1] - W, hw[0] - H))):
        want = normalised(fr[v, y:y + H, x:x + W, ::-1]).transpose(2, 0, 1)
        assert np.array_equal(val[i], want)
    zero = normalised(np.zeros(3))
    for antialias in (False, True):
        val, _ = A.warp64(fr, [0, 0, 1, 1], [[-1, 7, W, H], [5, -1, W, H], [hw[1] - W + 1, 3, W, H], [4, hw[0] - H + 1, W, H]], (H, W), scale=1.0,
                          antialias=antialias)
        assert np.array_equal(val[0][:, :, 0], np.broadcast_to(zero[:, None], (3, H)))
        assert np.array_equal(val[0][:, :, 1:], normalised(fr[0, 7:7 + H, 0:W - 1, ::-1]).transpose(2, 0, 1))
        assert np.array_equal(val[1][:, 0, :], np.broadcast_to(zero[:, None], (3, W)))
        assert np.array_equal(val[2][:, :, W - 1], np.broadcast_to(zero[:, None], (3, H)))
        assert np.array_equal(val[3][:, H - 1, :], np.broadcast_to(zero[:, None], (3, W)))
    # boxes that must be all zero
    k = [i for i, c in enumerate(A.case_list()) if c[1] == (16, 12)][0]
    names = A.case_list()[k][2]
    val, _ = A.case_reference(k, False)
    for nm in A.OUTSIDE:
        assert np.array_equal(val[names.index(nm)], np.broadcast_to(zero[:, None, None], (3, 16, 12))), nm


def test_antialias_equals_plain_where_nothing_is_down_scaled():
    for k, (hw, res, names, boxes) in enumerate(A.case_list()):
        if res != (64, 48):
            continue
        p, a = A.case_reference(k, False)[0], A.case_reference(k, True)[0]
        eff = A.box_cs64(boxes, res[1], res[0])
        up = eff[:, 2] <= res[1]
        assert up.any() and not up.all()
        assert np.array_equal(p[up], a[up])
        down = names.index('down-scaled 3 x')
        assert not up[down] and np.abs(p[down] - a[down]).max() > 0.1


WRONG = {'half-pixel convention': dict(half=0.5), 'replicated border': dict(replicate=True), 'missing 1.25': dict(scale=1.0),
         'no aspect fix': dict(aspect_fix=False)}
# the boxes each mistake must show on: (the border forms) the ones that hang over an edge
SHOWS_ON = {'half-pixel convention': ('wider', 'taller', 'up-scaled 9 x 7', 'over the left edge'),
            'replicated border': ('over the left edge', 'over the top edge', 'over the right edge', 'over the bottom edge'),
            'missing 1.25': ('wider', 'taller', 'at the aspect', 'up-scaled 9 x 7'),
            'no aspect fix': ('wider', 'taller', 'w = 0', 'h = 0')}


@pytest.mark.parametrize('wrong', sorted(WRONG))
def test_the_tolerance_rejects_wrong_restatements(wrong):
    for k, (hw, res, names, boxes) in enumerate(A.case_list()):
        if res not in A.SMALL_OUTPUTS:
            continue
        val, tol = A.case_reference(k, False)
        bad, _ = A.warp64(A.case_frames(hw), A.case_view_of(len(boxes)), boxes, res, **WRONG[wrong])
        assert crop_check(val, val, tol) == (0.0, 0)
        for nm in SHOWS_ON[wrong]:
            i = names.index(nm)
            worst, n_bad = crop_check(bad[i:i + 1], val[i:i + 1], tol[i:i + 1])
            assert n_bad > 0 and worst > 4.0, (wrong, hw, res, nm, worst, n_bad)


def test_the_tolerance_rejects_a_normaliser_without_the_outside_taps():
    seen = 0
    for k, (hw, res, names, boxes) in enumerate(A.case_list()):
        if 'down-scaled 3 x' not in names:
            continue
        i = names.index('down-scaled 3 x')
        val, tol = A.case_reference(k, True)
        bad, _ = A.warp64(A.case_frames(hw), A.case_view_of(len(boxes))[i:i + 1], boxes[i:i + 1], res, antialias=True, count_outside=False)
        eff = A.box_cs64(boxes[i:i + 1], res[1], res[0])[0]
        if not (eff[0] < 0 or eff[0] + eff[2] > hw[1] or eff[1] < 0 or eff[1] + eff[3] > hw[0]):
            continue                                     # (the box must leave the frame for the two normalisers to differ)
        worst, n_bad = crop_check(bad, val[i:i + 1], tol[i:i + 1])
        assert n_bad > 0 and worst > 4.0, (hw, res, worst, n_bad)
        seen += 1
    assert seen >= 4


def test_tolerance_is_tight_where_the_frame_is_smooth():
    """Nothing in the tolerance is a blanket figure: in the frames' smooth left half it stays near half a bf16 ulp of the value."""
    k = [i for i, c in enumerate(A.case_list()) if c[1] == (64, 48) and c[0] == A.FRAME_SIZES[1]][0]
    names = A.case_list()[k][2]
    val, tol = A.case_reference(k, False)
    i = names.index('at the aspect')                     # x 7.5 .. 22.5 of a 97-wide frame: the smooth half
    assert np.median(tol[i] / np.maximum(np.abs(val[i]), 2.0 ** -7)) < 2.0 ** -7


def test_shipped_config_sets_the_keys_and_a_bad_transform_is_refused():
    import pam
    from pam.dataset import GetConfig
    from pam.ivclabpose import box_transform_options
    root = os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf')
    p = GetConfig(os.path.join(root, 'model_configs_affine.yaml')).POSE_MODELS.HRPOSE
    assert dict(p)['BOX_TRANSFORM'] == 'affine' and dict(p)['FLIP_TEST'] is True
    assert box_transform_options(p) == ('affine', 1.25)
    flip = dict(GetConfig(os.path.join(root, 'model_configs_fliptest.yaml')).POSE_MODELS.HRPOSE)
    assert {k: v for k, v in dict(p).items() if k not in ('BOX_TRANSFORM', 'BOX_SCALE')} == flip
    stock = GetConfig(os.path.join(root, 'model_configs.yaml')).POSE_MODELS.HRPOSE
    assert not {'BOX_TRANSFORM', 'BOX_SCALE'} & set(dict(stock)) and box_transform_options(stock) == ('stretch', 1.25)
    assert box_transform_options(dict(BOX_TRANSFORM='stretch', BOX_SCALE=1.4)) == ('stretch', 1.4)
    for bad in (dict(BOX_TRANSFORM='letterbox'), dict(BOX_TRANSFORM='Affine'), dict(BOX_TRANSFORM=True), dict(BOX_TRANSFORM='affine', BOX_SCALE=0)):
        with pytest.raises(ValueError):
            box_transform_options(bad)
