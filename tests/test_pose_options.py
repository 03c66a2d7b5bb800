"""The optional keys of a POSE_MODELS.HRPOSE block (ivclabpose.POSE_OPTIONS): which attributes of the pose network a block sets, with
what values and in which order -- the order decides which refusal a bad YAML meets, because HRNetPose's property setters refuse
combinations as they are set.  No GPU: the network is a stand-in that keeps HRNetPose's own option properties and builds nothing.
The expectations are literals written from the constructor's text as it stood before the keys became one table."""
import types

import pytest

from pam import hrnet, ivclabpose as I

BASE = dict(NAME='HRPose', C=32, NUM_JOINTS=17, CHECKPOINT_FILE=None, MODEL_NAME='HRNet', RESOLUTION=[256, 192])
OPTIONS = ('soft_beta', 'shift_heatmap', 'post_process', 'blur_kernel', 'dark', 'flip_test', 'pose_nms', 'oks_thre', 'in_vis_thre')


class StandIn(hrnet.HRNetPose):
    def __init__(self, *a, **kw):
        object.__setattr__(self, 'order', [])
        object.__setattr__(self, 'ctor', kw)

    def __setattr__(self, name, value):
        if name in OPTIONS:
            self.order.append(name)
        super().__setattr__(name, value)


def build(monkeypatch, block, bag=False):
    monkeypatch.setattr(hrnet, 'HRNetPose', StandIn)
    block = dict(BASE, **block)
    model = I.ivclabpose({'NAME': ''}, types.SimpleNamespace(**block) if bag else block, None)
    return model.pose_model


@pytest.mark.parametrize('bag', [False, True])
def test_absent_keys_switch_the_four_flags_off_and_touch_nothing_else(monkeypatch, bag):
    net = build(monkeypatch, {}, bag)
    assert net.order == ['post_process', 'dark', 'flip_test', 'pose_nms']
    assert (net.soft_beta, net.shift_heatmap, net.post_process, net.blur_kernel, net.dark, net.flip_test) == (None, True, False, None, False, False)
    assert (net.pose_nms, net.oks_thre, net.in_vis_thre) == (False, 0.9, 0.2)
    assert (net.ctor['box_transform'], net.ctor['box_scale']) == ('stretch', 1.25)


@pytest.mark.parametrize('bag', [False, True])
def test_every_key_is_set_once_converted_in_the_constructors_order(monkeypatch, bag):
    net = build(monkeypatch, dict(SHIFT_HEATMAP=0, POST_PROCESS=0, BLUR_KERNEL=11.0, DARK=1, FLIP_TEST=1, OKS_NMS=1, OKS_THRE='0.8',
                                  IN_VIS_THRE=0, BOX_TRANSFORM='affine', BOX_SCALE=1.5), bag)
    assert net.order == ['shift_heatmap', 'post_process', 'blur_kernel', 'dark', 'flip_test', 'pose_nms', 'oks_thre', 'in_vis_thre']
    assert (net.shift_heatmap, net.post_process, net.blur_kernel, net.dark, net.flip_test) == (False, False, 11, True, True)
    assert type(net.blur_kernel) is int and (net.pose_nms, net.oks_thre, net.in_vis_thre) == (True, 0.8, 0.0)
    assert (net.ctor['box_transform'], net.ctor['box_scale']) == ('affine', 1.5)
    soft = build(monkeypatch, dict(SOFT_ARGMAX_BETA='2.5'), bag)
    assert soft.order[0] == 'soft_beta' and soft.soft_beta == 2.5 and soft.order[1:] == ['post_process', 'dark', 'flip_test', 'pose_nms']
    assert build(monkeypatch, dict(SOFT_ARGMAX_BETA=0), bag).soft_beta is None          # 0 leaves the hard arg-max


@pytest.mark.parametrize('block, text', [
    (dict(SOFT_ARGMAX_BETA=2, POST_PROCESS=True), 'soft_beta cannot be combined'),                 # met at post_process
    (dict(DARK=True, POST_PROCESS=True), 'dark cannot be combined'),                               # post_process goes in first, dark is refused
    (dict(SOFT_ARGMAX_BETA=2, DARK=True, FLIP_TEST=True), 'dark cannot be combined'),              # dark is set before flip_test
    (dict(SOFT_ARGMAX_BETA=2, FLIP_TEST=True), 'soft_beta cannot be combined'),
    (dict(BLUR_KERNEL=10, DARK=True), 'blur_kernel must be'),                                      # blur_kernel is set before dark
])
def test_a_bad_block_meets_the_refusal_the_order_gives_it(monkeypatch, block, text):
    with pytest.raises(ValueError, match=text):
        build(monkeypatch, block)


def test_opt_reads_dicts_attribute_bags_and_missing_blocks():
    assert I._opt(None, 'K') is None and I._opt(None, 'K', 3) == 3
    assert I._opt({'K': 0}, 'K', 3) == 0 and I._opt({}, 'K', 3) == 3
    assert I._opt(types.SimpleNamespace(K=0), 'K', 3) == 0 and I._opt(types.SimpleNamespace(), 'K') is None
    m = I.ivclabpose({'NAME': '', 'DETECT_EVERY': 5, 'TRACK_BOX_GROW': 1.5}, None, None)
    assert m.detect_every == 5 and m.track_box_rule == dict(grow=1.5, pad_px=8.0, min_size_px=8.0, max_gap=3)
    m = I.ivclabpose(types.SimpleNamespace(NAME='', TRACK_BOX_PAD=2), None, None)
    assert m.detect_every == 1 and m.track_box_rule == dict(grow=1.25, pad_px=2.0, min_size_px=8.0, max_gap=3)
    assert I.one_euro_from_matcher({'ONE_EURO': {'BETA': 0.4}}) == {'beta': 0.4} and I.one_euro_from_matcher(types.SimpleNamespace()) is None
