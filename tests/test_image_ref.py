"""CPU: the float64 restatements of tests/image_ref.py agree with the older references (selfcheck.reference_preprocess,
selfcheck.reference_decode, torch's antialiased interpolation, F.conv2d in float64), and every tolerance they hand to the GPU tests
(tests/test_gpu_image_shapes.py) rejects a deliberately wrong restatement on the very inputs those tests use: pixel centres without the
-0.5, channels not swapped, bf16 by truncation, a 1/32-pixel shift, a one-sided cut of the antialias window, a last-index tie rule, a
head that skips its final 8 channels.  The share of heat-maps whose arg-max the float32 bound leaves open is asserted here too."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_ref as R

RESOLUTIONS = [(256, 192), (384, 288)]
CROP_IDS = [c[0] for c in R.CROP_CASES]


def test_bf16_helpers_match_torch():
    x = np.random.default_rng(0).standard_normal(100000) * np.exp(np.random.default_rng(1).uniform(-20, 3, 100000))
    x = np.concatenate([x, [1.00390625, 1.01171875, -1.00390625, 0.0, 2.0 ** -7]])          # exact ties: to even
    want = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).double().numpy()
    assert np.array_equal(R.bf16_rne(x), want)
    assert np.all(np.abs(R.bf16_rne(x) - x.astype(np.float32)) <= 0.5 * R.bf16_ulp(x))
    assert np.all(R.bf16_ulp(np.array([1.0, 1.99, 2.0, 0.75])) == np.array([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]))
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(1919.5) == 2.0 ** -13


@pytest.mark.parametrize('case', R.CROP_CASES[:2], ids=CROP_IDS[:2])
@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_preprocess64_agrees_with_the_float32_restatement(case, res):
    from pam import selfcheck
    frames, view_of, boxes = R.crop_case_inputs(case)
    val, tol = R.preprocess64(frames, view_of, boxes, res)
    ref = selfcheck.reference_preprocess(torch.from_numpy(frames), torch.from_numpy(view_of), torch.from_numpy(boxes), res).double().numpy()
    # the float32 restatement is one more float32 evaluation of the formula: it has to lie inside the tolerance without its bf16 term
    worst, bad = R.crop_check(ref, val, tol - 0.5 * R.bf16_ulp(np.abs(val)))
    assert bad == 0, worst
    assert R.crop_check(R.bf16_rne(ref), val, tol)[1] == 0


@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_antialias64_agrees_with_torch_on_integer_boxes(res):
    frames, view_of, boxes = R.crop_case_inputs(R.AA_CASES[0])
    val, tol = R.preprocess64(frames, view_of, boxes, res, antialias=True)
    mean = torch.tensor(R.MEAN).view(1, 3, 1, 1); std = torch.tensor(R.STD).view(1, 3, 1, 1)
    for i in range(4):                                     # the integer, in-frame boxes of the list
        bx, by, bw, bh = [int(v) for v in boxes[i]]
        crop = torch.from_numpy(frames[view_of[i], by:by + bh, bx:bx + bw].copy()).permute(2, 0, 1)[[2, 1, 0]].double().unsqueeze(0)
        ref = ((F.interpolate(crop, size=res, mode='bilinear', antialias=True, align_corners=False) / 255.0 - mean) / std).numpy()
        worst, bad = R.crop_check(ref[0], val[i], tol[i] - 0.5 * R.bf16_ulp(np.abs(val[i])))
        assert bad == 0, (i, worst)


def test_antialias_equals_bilinear_where_nothing_is_downscaled():
    frames, view_of, boxes = R.crop_case_inputs(R.AA_CASES[0])
    i = 2                                                  # 150 x 200 box, both outputs larger
    a, _ = R.preprocess64(frames, view_of[i:i + 1], boxes[i:i + 1], (256, 192), antialias=True)
    b, _ = R.preprocess64(frames, view_of[i:i + 1], boxes[i:i + 1], (256, 192))
    assert np.abs(a - b)[:, :, 4:-4, 4:-4].max() < 1e-5     # float32 coordinates in both; the border differs (box clip vs frame clip)


def test_head64_is_conv2d_in_float64():
    feat, wt, b, _ = R.head_inputs(48, 33, 17, 2)
    hm, bound = R.head64(feat, wt, b)
    x = torch.from_numpy(feat).double().permute(0, 3, 1, 2)
    ref = F.conv2d(x, torch.from_numpy(wt).double().reshape(17, 48, 1, 1), torch.from_numpy(b).double()).reshape(2, 17, -1).numpy()
    assert np.abs(hm - ref).max() < 1e-12
    ref32 = F.conv2d(x.float(), torch.from_numpy(wt).reshape(17, 48, 1, 1), torch.from_numpy(b)).reshape(2, 17, -1).double().numpy()
    assert np.all(np.abs(ref32 - hm) <= bound)              # any float32 evaluation order lies within the chain bound


@pytest.mark.parametrize('hw', R.DECODE_MAPS, ids=['%dx%d' % m for m in R.DECODE_MAPS])
def test_decode64_agrees_with_reference_decode(hw):
    from pam import selfcheck
    h, w = hw
    hm, boxes, cases = R.decode_inputs(h, w)
    hm = hm[:, [j for j in range(17) if j not in (7,)]]    # reference_decode's equality mask has no first index on a map of -inf
    ref = selfcheck.reference_decode(torch.from_numpy(hm).reshape(hm.shape[0], -1, h, w), torch.from_numpy(boxes)).numpy()
    idx = np.argmax(hm.astype(np.float64), axis=2)
    y, x = R.decode64(idx // w, idx % w, boxes, h, w)
    assert np.array_equal(ref[:, :, 0], y) and np.array_equal(ref[:, :, 1], x)
    assert np.array_equal(ref[:, :, 2], hm.max(2).astype(np.float64))
    for crop, name, px in cases:
        assert idx[crop, 5] == px[0], name  # the planted tie decodes to its first pixel


# ---- the checks have teeth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CROP_CASES, ids=CROP_IDS)
@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_crop_tolerance_rejects_wrong_restatements(case, res):
    frames, view_of, boxes = R.crop_case_inputs(case)
    val, tol = R.preprocess64(frames, view_of, boxes, res)
    assert R.crop_check(R.bf16_rne(val), val, tol)[1] == 0                      # the right answer passes
    wrong = dict(no_half=dict(half=0.0), not_swapped=dict(swap=False), shifted=dict(shift=1.0 / 32))
    if case[1][1] == 1:
        wrong.pop('shifted')                                                   # a frame one pixel wide has no x to shift along
    for name, kw in wrong.items():
        bad = R.preprocess64(frames, view_of, boxes, res, **kw)[0]
        assert R.crop_check(R.bf16_rne(bad), val, tol)[1] > 0, name
    assert R.crop_check(R.bf16_trunc(val), val, tol)[1] > 0


@pytest.mark.parametrize('res', RESOLUTIONS, ids=['256x192', '384x288'])
def test_antialias_tolerance_rejects_wrong_restatements(res):
    for case in R.AA_CASES + [R.aa_limit_case(res), R.aa_limit_case(res, 13.0)]:
        frames, view_of, boxes = R.crop_case_inputs(case)
        val, tol = R.preprocess64(frames, view_of, boxes, res, antialias=True)
        assert R.crop_check(R.bf16_rne(val), val, tol)[1] == 0
        for name, kw in dict(not_swapped=dict(swap=False), shifted=dict(shift=1.0 / 32)).items():
            bad = R.preprocess64(frames, view_of, boxes, res, antialias=True, **kw)[0]
            assert R.crop_check(R.bf16_rne(bad), val, tol)[1] > 0, (case[0], name)
        assert R.crop_check(R.bf16_trunc(val), val, tol)[1] > 0
        one_sided = R.preprocess64(frames, view_of, boxes, res, antialias=True, centred=False)[0]
        beyond = 'x13' in case[0]
        # up to the limit the window is never cut: both forms are the same; beyond it the one-sided cut is out of tolerance
        assert (R.crop_check(R.bf16_rne(one_sided), val, tol)[1] > 0) == beyond, case[0]


@pytest.mark.parametrize('C', R.HEAD_CHANNELS)
@pytest.mark.parametrize('hw', R.HEAD_MAPS, ids=['%dx%d' % m for m in R.HEAD_MAPS])
def test_argmax_check_rejects_a_last_index_rule_and_a_short_head(C, hw):
    h, w = hw
    feat, wt, b, boxes, cases = R.seam_inputs(C, h, w)
    hm, bound = R.head64(feat, wt, b)
    first = np.argmax(hm, axis=2)
    res = R.argmax_check(hm, bound, first)
    assert res['wrong'] == [] and res['undecided'] <= 0.01 * res['maps'], res['undecided']
    for crop, name, px in cases:
        assert first[crop, 5] == px[0] and all(hm[crop, 5, p] == hm[crop, 5, px[0]] for p in px), name     # the plant IS the maximum
        assert np.sort(hm[crop, 5])[-len(px) - 1] < hm[crop, 5, px[0]] - 1.0, name
    assert np.all(first[:, 3] == 0) and np.all(first[:, 7] == 0) and np.all(first[:, 9] == 0)
    last = R.last_index_argmax(hm)
    bad = R.argmax_check(hm, bound, last)['wrong']
    ties = [c for c, _, px in cases if len(px) > 1]
    assert {(a, j) for a, j, _, _ in bad} >= {(c, 5) for c in ties} | {(c, 3) for c in range(len(cases))}
    # a head that skips its final 8 channels: out of the FMA bound, and arg-maxima that argmax_check refuses
    feat, wt, b, boxes = R.head_case_inputs(C, h, w, 5)
    hm, bound = R.head64(feat, wt, b)
    short, _ = R.head64(feat, wt, b, channels=C - 8)
    assert np.any(np.abs(short - hm) > bound)
    if h * w > 100:
        assert R.argmax_check(hm, bound, np.argmax(short, axis=2))['wrong'] != []


@pytest.mark.parametrize('C', R.HEAD_CHANNELS)
@pytest.mark.parametrize('hw', R.HEAD_MAPS, ids=['%dx%d' % m for m in R.HEAD_MAPS])
def test_share_of_undecided_maps_is_at_most_one_percent(C, hw):
    h, w = hw
    for n in R.HEAD_CROPS:
        feat, wt, b, _ = R.head_case_inputs(C, h, w, n)
        hm, bound = R.head64(feat, wt, b)
        res = R.argmax_check(hm, bound, np.argmax(hm, axis=2))
        assert res['wrong'] == [] and res['undecided'] <= 0.01 * res['maps'], (n, res['undecided'], res['maps'])


def test_soft64_limits():
    feat, wt, b, _ = R.head_inputs(32, 7, 5, 2)
    hm, _ = R.head64(feat, wt, b)
    ey, ex, m = R.soft64(hm, 1.0e8, 7, 5)
    idx = np.argmax(hm, axis=2)
    assert np.allclose(ey, idx // 5, atol=1e-6) and np.allclose(ex, idx % 5, atol=1e-6) and np.array_equal(m, hm.max(2))
    ey, ex, _ = R.soft64(np.zeros((1, 17, 35)), 4.0, 7, 5)
    assert np.allclose(ey, 3.0) and np.allclose(ex, 2.0)


@pytest.mark.parametrize('C', R.HEAD_CHANNELS)
def test_soft_slack_covers_any_perturbation_within_the_bound(C):
    """soft64 of maps moved by +-bound (random signs, and the two signs that push the mean hardest) stays within soft_slack; without the
    slack the 1e-3-cell figure alone can be exceeded at beta 25, which is why the GPU tests' check_soft carries the term."""
    h, w = 64, 48
    feat, wt, b, _ = R.head_case_inputs(C, h, w, 5)
    hm, bound = R.head64(feat, wt, b)
    rng = np.random.default_rng(C)
    idx = np.arange(h * w)
    over = 0.0
    for beta in R.SOFT_BETAS:
        ey, ex, _ = R.soft64(hm, beta, h, w)
        sy, sx = R.soft_slack(hm, bound, beta, h, w)
        pushes = [np.sign(rng.standard_normal(hm.shape)), np.sign((idx // w) - ey[..., None]), np.sign((idx % w) - ex[..., None])]
        for e in pushes:
            py, px, _ = R.soft64(hm + e * bound, beta, h, w)
            assert np.all(np.abs(py - ey) <= sy + 1e-9) and np.all(np.abs(px - ex) <= sx + 1e-9), beta     # 1e-9: float64 round-off of soft64 itself
            over = max(over, float(np.abs(py - ey).max()), float(np.abs(px - ex).max()))
    assert over > 1e-3, over                               # a perturbation within the bound CAN move soft64 by more than 1e-3 of a cell
