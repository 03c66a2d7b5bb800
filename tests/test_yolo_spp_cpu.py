"""CPU: the YOLOv3-SPP network definition (yolov3.spp_cfg), its Darknet .weights file, the executor's plan for the SPP block and the
near-miss patterns it must go on refusing, the CPU restatement of the SPP kernel's contract (spp_ref.py) against darknet_maxpool + cat,
and the calibrated test network of darknet_spp_calibrated.py.  No GPU."""
import hashlib
import os
from collections import Counter

import numpy as np
import pytest
import torch

import darknet_spp_calibrated as SC
import spp_ref as R
from pam import yolov3

SPP_FLOATS = 63052381
SPP_BYTES = 20 + 4 * SPP_FLOATS            # 252 209 544: the size of the public yolov3-spp.weights


def test_spp_cfg_layer_table():
    net, layers = yolov3.parse_cfg(yolov3.spp_cfg())
    assert len(layers) == 114
    assert Counter(b['type'] for b in layers) == {'convolutional': 76, 'shortcut': 23, 'route': 7, 'maxpool': 3, 'yolo': 3, 'upsample': 2}
    assert [i for i, b in enumerate(layers) if b['type'] == 'yolo'] == [89, 101, 113]
    assert [(i, b['size'], b['stride']) for i, b in enumerate(layers) if b['type'] == 'maxpool'] == [(78, 5, 1), (80, 9, 1), (82, 13, 1)]
    assert [layers[i]['layers'] for i in (79, 81, 83)] == [[-2], [-4], [-1, -3, -5, -6]]
    b = layers[84]
    assert (b['type'], b['filters'], b['size'], b['stride'], b['batch_normalize'], b['activation']) == ('convolutional', 512, 1, 1, 1, 'leaky')
    # the absolute skips keep their values, the relative route behind each head too
    assert [b['layers'] for b in layers if b['type'] == 'route'][3:] == [[-4], [-1, 61], [-4], [-1, 36]]
    # without the seven SPP layers it is yolov3.cfg, layer for layer
    _, plain = yolov3.parse_cfg(yolov3.default_cfg())
    assert layers[:78] + layers[85:] == plain
    m = yolov3.Darknet(yolov3.spp_cfg())
    assert m.chans[77:85] == [512, 512, 512, 512, 512, 512, 2048, 512]
    assert 'yolov3-spp' in yolov3.ARCHS and yolov3.ARCHS['yolov3-spp'] is yolov3.spp_cfg


def test_default_and_tiny_cfg_text_is_unchanged():
    """sha256 of the generated text, taken from the commit before spp_cfg shared default_cfg's generator."""
    want = {('default_cfg', ()): '3b7d2d453c8c39665c7b90e0a0b6ed6d8d02a6c53a824a8bafe3ceaaeb202611',
            ('default_cfg', (608, 320, 3)): '16b77fc1321a0dba8e744fc0d0f130b7f68916a4e7347d7251736af770fc9500',
            ('tiny_cfg', ()): '2926b9d30dc8256d5df90a4e13c6c1de77b5b9bf8e8cae9a67304031c6f34b7f',
            ('tiny_cfg', (608, 320, 3)): '330fc47969ccfc2e67d5f113196dd0754344d377c2dd8ca4898ceb5897a306fe'}
    for (name, a), digest in want.items():
        assert hashlib.sha256(getattr(yolov3, name)(*a).encode()).hexdigest() == digest, (name, a)


def test_spp_weights_file_size_and_round_trip(tmp_path):
    m = yolov3.Darknet(yolov3.spp_cfg()).init_random(3)
    assert sum(p.numel() for mm in m.conv_modules() for p in mm.parameters()) + 2 * sum(mm.bn.num_features for mm in m.conv_modules() if hasattr(mm, 'bn')) == SPP_FLOATS
    path = str(tmp_path / 'spp.weights')
    m.save_darknet_weights(path)
    assert os.path.getsize(path) == SPP_BYTES == 252209544
    m2 = yolov3.Darknet(yolov3.spp_cfg(320, 320))                  # the weights do not depend on the input size
    m2.load_darknet_weights(path)                                  # raises when floats are left over
    sd, sd2 = m.state_dict(), m2.state_dict()
    for k in sd:
        if not k.endswith('num_batches_tracked'):
            assert torch.equal(sd[k], sd2[k]), k
    with pytest.raises(ValueError):
        yolov3.Darknet().load_darknet_weights(path)                # the SPP file into Darknet-53: 1 050 624 floats left over


@pytest.mark.parametrize('width,height', [(416, 416), (416, 256)])
def test_spp_head_shapes(width, height):
    m = yolov3.Darknet(yolov3.spp_cfg(width, height)).init_random(0).eval()
    with torch.no_grad():
        heads = m(torch.rand((1, 3, height, width), generator=torch.Generator().manual_seed(1)))
    assert [tuple(h.shape) for h in heads] == [(1, 255, height // s, width // s) for s in (32, 16, 8)]
    assert all(bool(torch.isfinite(h).all()) for h in heads)


def test_spp_plan_is_one_step():
    """The executor's plan for the standard SPP cfg (host logic: packs on the CPU): layers 78 .. 83 are ONE step that writes layer 83 from
    layer 77, no max-pool step, and the rest is Darknet-53's plan with the layer numbers shifted by 7 behind the block."""
    m = yolov3.Darknet(yolov3.spp_cfg()).init_random(0).eval()
    hip = yolov3.HipDarknet(m, torch.device('cpu'))
    kinds = Counter(s[0] for s in hip.plan)
    assert kinds['spp'] == 1 and kinds['pool'] == 0 and kinds['head'] == 3 and kinds['upcat'] == 2 and kinds['conv'] == 76 and kinds['add'] == 0
    assert [s for s in hip.plan if s[0] == 'spp'] == [('spp', 83, 77, (5, 9, 13))]
    assert hip.real[83] == hip.padded[83] == 2048
    assert hip.real[77:85] == hip.padded[77:85] == [512, 512, 512, 512, 512, 512, 2048, 512]
    assert len(hip.real) == len(hip.padded) == 114
    op84 = [s for s in hip.plan if s[0] == 'conv' and s[1] == 84][0][2]
    assert (op84.cin, op84.cout, op84.kh) == (2048, 512, 1) and [s for s in hip.plan if s[0] == 'conv' and s[1] == 84][0][3] == 83
    plain = yolov3.HipDarknet(yolov3.Darknet(yolov3.default_cfg()).init_random(0).eval(), torch.device('cpu'))
    shift = lambda v: v + 7 if v >= 78 else v

    def shape_of(s):
        if s[0] == 'conv':
            return (s[0], s[1], (s[2].cin, s[2].cout, s[2].kh, s[2].stride), s[3], s[4], s[5])
        return s
    want = []
    for s in plain.plan:
        if s[0] == 'conv':
            want.append(('conv', shift(s[1]), (s[2].cin, s[2].cout, s[2].kh, s[2].stride), shift(s[3]), s[4], None if s[5] is None else shift(s[5])))
        else:
            want.append((s[0],) + tuple(shift(v) for v in s[1:]))
    got = [shape_of(s) for s in hip.plan if not (s[0] == 'spp' or (s[0] == 'conv' and s[1] == 84))]
    # layer 78 of the plain plan reads 77; here the layer behind the block (85) reads 84
    want = [(w[:3] + (84,) + w[4:]) if (w[0] == 'conv' and w[1] == 85) else w for w in want]
    assert got == want


HEAD = ('[net]\nwidth=64\nheight=64\nchannels=3\n[convolutional]\nbatch_normalize=1\nfilters=64\nsize=3\nstride=1\npad=1\nactivation=leaky\n'
        '[convolutional]\nbatch_normalize=1\nfilters=64\nsize=3\nstride=2\npad=1\nactivation=leaky\n')
TAIL = '[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n[yolo]\nmask=0,1,2\nanchors=1,1,2,2,3,3\nclasses=1\n'


def _block(sizes=(5, 9, 13), strides=(1, 1, 1), closing='-1,-3,-5,-6', backs=('-2', '-4')):
    return ('[maxpool]\nstride=%d\nsize=%d\n[route]\nlayers=%s\n[maxpool]\nstride=%d\nsize=%d\n[route]\nlayers=%s\n[maxpool]\nstride=%d\nsize=%d\n'
            '[route]\nlayers=%s\n' % (strides[0], sizes[0], backs[0], strides[1], sizes[1], backs[1], strides[2], sizes[2], closing))


def _plan(cfg):
    return yolov3.HipDarknet(yolov3.Darknet(cfg).init_random(0).eval(), torch.device('cpu'))


def test_spp_pattern_elsewhere_and_with_other_sizes():
    """The pattern, not the layer numbers: behind layer 1 of a small cfg (a 32 x 32 map, the kernel's limit), with absolute route indices,
    with sizes 3 / 7 / 11."""
    hip = _plan(HEAD + _block() + TAIL)
    assert [s for s in hip.plan if s[0] in ('spp', 'pool')] == [('spp', 7, 1, (5, 9, 13))] and hip.real[2:8] == [64] * 5 + [256]
    hip = _plan(HEAD + _block((3, 7, 11), closing='6,4,2,1', backs=('1', '1')) + TAIL)
    assert [s for s in hip.plan if s[0] in ('spp', 'pool')] == [('spp', 7, 1, (3, 7, 11))]


@pytest.mark.parametrize('block,tail,match', [
    (_block(closing='-6,-5,-3,-1'), TAIL, 'maxpool'),                        # the closing route in another order
    (_block(closing='-5,-3,-1,-6'), TAIL, 'maxpool'),
    (_block(closing='-1,-3,-5'), TAIL, 'maxpool'),                           # ... without the source
    (_block((5, 8, 13)), TAIL, 'maxpool'),                                   # an even pool size
    (_block((4, 9, 13)), TAIL, 'maxpool'),
    (_block((5, 9, 15)), TAIL, 'maxpool'),                                   # above 13
    (_block((9, 5, 13)), TAIL, 'maxpool'),                                   # not ascending
    (_block(strides=(2, 1, 1)), TAIL, 'maxpool'),                            # a stride-2 pool
    (_block(strides=(1, 1, 2)), TAIL, 'maxpool'),
    (_block(backs=('-2', '-3')), TAIL, 'maxpool'),                           # the third pool pools the first pool, not the source
    (_block(), '[route]\nlayers=-2\n' + TAIL, 'maxpool'),                    # an inner layer (pool 13) that a later route reads
    (_block(), '[route]\nlayers=-1,-6\n' + TAIL, 'maxpool'),                 # ... (pool 5) in a route over several layers
    (_block((3, 7, 11), closing='-6,-5,-3,-1'), TAIL, 'maxpool'),            # size 3 alone is a pool the executor runs; the 7 behind it is not
], ids=['order', 'order2', 'no-source', 'even', 'even-first', 'above-13', 'descending', 'stride2', 'stride2-last', 'chained', 'inner-read',
        'inner-read-multi', 'order-3-7-11'])
def test_near_miss_patterns_are_still_refused(block, tail, match):
    cfg = HEAD + block + tail
    m = yolov3.Darknet(cfg).init_random(0).eval()                            # the fp32 module runs them
    if 'stride=2\nsize' not in block:                                         # (a stride-2 pool leaves nothing its route could join)
        with torch.no_grad():
            assert len(m(torch.rand(1, 3, 64, 64))) == 1
    with pytest.raises(NotImplementedError, match=match):
        yolov3.HipDarknet(m, torch.device('cpu'))


def test_multi_layer_route_elsewhere_is_still_refused():
    cfg = HEAD + '[route]\nlayers=-1,-2\n' + TAIL
    with pytest.raises(NotImplementedError, match='route over several layers'):
        _plan(cfg)


def test_spp_block_refuses_padded_sources_and_maps_above_the_limit():
    from pam import _lib
    assert _lib.SPP_MAX_HW == 32
    padded = HEAD.replace('filters=64\nsize=3\nstride=2', 'filters=40\nsize=3\nstride=2')      # 40 channels run padded to 64
    with pytest.raises(NotImplementedError, match='channel-padded'):
        _plan(padded + _block() + TAIL)
    with pytest.raises(NotImplementedError, match='maps up to 32'):
        _plan(HEAD.replace('width=64', 'width=66') + _block() + TAIL)                           # a 32 x 33 map
    assert yolov3._layer_sizes(yolov3.Darknet(yolov3.spp_cfg(416, 256)))[77] == (8, 13)


# ---- the kernel's contract on the CPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_loop_restatement_equals_darknet_maxpool_and_tells_the_mistakes_apart(case):
    """At every shape of the GPU test: the explicit-loop contract == darknet_maxpool + cat == the kernel's clamped cascade, exactly (a maximum
    selects; -inf and ties included), and the three mistakes give something else."""
    n, c, h, w, sizes = case
    xb = R.planted_input(min(n, 2), min(c, 48), h, w, 100 * h + w)           # the CPU model has no slabs: 48 channels hold every plant
    x = xb.double().numpy()
    want = R.torch_spp(xb.float(), sizes).double().numpy()
    loop = R.loop_spp(x, sizes)
    assert loop.shape == want.shape == (x.shape[0], 4 * x.shape[1], h, w)
    assert np.array_equal(loop, want)
    assert np.array_equal(R.cascade_spp(x, sizes), loop)
    if sizes == (5, 9, 13):                                                  # taps skipped, not clamped: border columns lost.  (With 3 / 7 / 11
        assert not np.array_equal(R.cascade_spp(x, sizes, clamp=False), loop)    # the tap that stays inside still covers the border: no difference.)
    if (h, w) != (1, 1):                                                     # on one pixel every window is that pixel
        assert not np.array_equal(R.loop_spp(x, sizes, start='full'), loop)  # windows from -pad, not -pad / 2
        assert not np.array_equal(R.loop_spp(x, sizes, order='x a b c'), loop)   # the concat order reversed
    # the corner maxima reach exactly the pixels whose window holds the corner
    a = sizes[0] // 2
    assert (loop[:, 2 * x.shape[1], :a + 1, :a + 1] == R.BIG).all()          # channel 0 of the smallest pool


def test_taps_cover_the_window_with_neighbours_that_touch():
    for r1 in range(1, 5):
        for r2 in range(r1 + 1, 6):
            for r3 in range(r2 + 1, 7):
                for rs, rt in ((r1, r2), (r2, r3)):
                    o = R.taps(rs, rt)
                    assert o[0] == -(rt - rs) and o[-1] == rt - rs and len(o) <= 5 and all(0 < b - a <= 2 * rs + 1 for a, b in zip(o, o[1:])), (rs, rt, o)
    assert R.taps(2, 4) == [-2, 2] and R.taps(4, 6) == [-2, 2] and R.taps(1, 3) == [-2, 0, 2]


def test_zero_sign_rule():
    a = torch.tensor([0.0, -0.0, 1.0, -0.0, 0.0], dtype=torch.bfloat16)
    b = torch.tensor([-0.0, -0.0, 1.0, 1.0, 2.0 ** -126], dtype=torch.bfloat16)
    assert R.same_up_to_zero_sign(a, b).tolist() == [True, True, True, False, False]


# ---- the calibrated test network ----------------------------------------------------------------------------------------------------------
def test_calibrated_spp_is_deterministic_and_gives_5_to_63_boxes():
    m = SC.calibrated()
    again = SC._build(SC.SEED)
    for (k, a), b in zip(m.state_dict().items(), again.state_dict().values()):
        assert torch.equal(a, b), k
    assert len(SC.folded_convs(m)) == 76
    per = SC.check_box_counts()
    print('spp calibrated boxes (kept, candidates):', per)
