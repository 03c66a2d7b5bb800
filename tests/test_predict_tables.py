"""CPU: the one upload of HRNetPose.predict(), as HRNetPose._call_tables packs it on the host.  With n persons in V views the int32 array is
[view_of n | slot_of n | boxes 4n as float32 bits | per-view counts V | one pad word when V is odd | frame pointers V as int64 | with
pose_nms a (V, S) float32 box-score table, 1.0 where a person has no score], S = max(max_dets, max(counts)).  Every expected value below
is written out by hand from that layout."""
import numpy as np

from pam.dump import DumpResults
from pam.hrnet import HRNetPose

P0, P2 = 0x7F0012345600, 0x7F00ABCDEF00       # frame addresses above 2^32: both halves of the int64 words carry bits
B00, B01, B20 = [10.0, 20.0, 30.5, 40.25], [1.5, 2.5, 3.5, 4.5], [100.0, 200.0, 50.0, 60.0]


def _net(pose_nms=False):
    net = HRNetPose.__new__(HRNetPose)
    net.max_dets = 1
    net.pose_nms = pose_nms
    return net


def _three_views():
    """Counts [2, 0, 1]; one person with a score, one with 'score': None, one without the key."""
    return [[dict(bbox=B00, score=0.75), dict(bbox=B01, score=None)], [], [dict(bbox=B20)]]


def _ptr_of(table):
    asked = []

    def frame_ptr_of(v):
        asked.append(v)
        return table[v]
    return frame_ptr_of, asked


def test_three_views_odd_count_pads_to_an_even_pointer_offset():
    frame_ptr_of, asked = _ptr_of({0: P0, 2: P2})              # (a view without persons has no frame: asking for it would raise)
    meta, (views, slots, boxes, cnt, S, o_ptr) = _net()._call_tables(_three_views(), frame_ptr_of)
    assert meta.dtype == np.int32 and meta.size == 28          # 3 + 3 + 12 + 3 + 1 pad + 6
    assert meta[0:3].tolist() == [0, 0, 2] == views            # view_of
    assert meta[3:6].tolist() == [0, 1, 0] == slots            # slot_of
    assert meta[6:18].view(np.float32).tolist() == B00 + B01 + B20 and boxes == [B00, B01, B20]
    assert meta[18:21].tolist() == [2, 0, 1] == cnt            # counts, then one pad word at [21]
    assert o_ptr == 22 and o_ptr % 2 == 0
    assert meta[22:28].view(np.int64).tolist() == [P0, 0, P2]
    assert S == 2                                              # a view's count above max_dets = 1 widens the buffer
    assert sorted(asked) == [0, 2]


def test_pose_nms_appends_the_box_score_table():
    meta, (views, slots, boxes, cnt, S, o_ptr) = _net(pose_nms=True)._call_tables(_three_views(), _ptr_of({0: P0, 2: P2})[0])
    assert meta.size == 34 and o_ptr == 22 and S == 2          # the 28 words above + V * S = 6 scores
    assert meta[22:28].view(np.int64).tolist() == [P0, 0, P2]
    assert meta[28:34].view(np.float32).reshape(3, 2).tolist() == [[0.75, 1.0], [1.0, 1.0], [1.0, 1.0]]
    # the same call with a score on the third view's person: [[s00, s01], [1, 1], [s20, 1]]
    pbl = _three_views()
    pbl[0][1]['score'], pbl[2][0]['score'] = 0.5, 0.25
    meta, _ = _net(pose_nms=True)._call_tables(pbl, _ptr_of({0: P0, 2: P2})[0])
    assert meta[28:34].view(np.float32).reshape(3, 2).tolist() == [[0.75, 0.5], [1.0, 1.0], [0.25, 1.0]]


def test_two_views_even_count_has_no_pad_word():
    pbl = [[dict(bbox=B00)], [dict(bbox=B01), dict(bbox=B20), dict(bbox=B00)]]
    meta, (views, slots, boxes, cnt, S, o_ptr) = _net()._call_tables(pbl, _ptr_of({0: P0, 1: P2})[0])
    n, V = 4, 2
    assert o_ptr == 6 * n + V == 26 and meta.size == 26 + 2 * V
    assert meta[0:4].tolist() == [0, 1, 1, 1] and meta[4:8].tolist() == [0, 0, 1, 2]
    assert meta[8:24].view(np.float32).tolist() == B00 + B01 + B20 + B00
    assert meta[24:26].tolist() == [1, 3] and S == 3
    assert meta[26:30].view(np.int64).tolist() == [P0, P2]


def test_an_empty_call_returns_before_anything_touches_a_device():
    net = _net()
    net._arenas, net.max_crops = {}, 32                        # (what predict() reads before it looks at the persons); no `device`
    out = net.predict([[], [], []], batch_size=4)
    assert type(out) is DumpResults and len(out) == 3 and list(out) == [[], [], []]
    assert out.device_det is None and not hasattr(net, 'device')
