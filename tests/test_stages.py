"""CPU: the host-side homes of the optional stages (pam.stages, _lib.Handle.track_boxes, visualization.view3d_setup) on plain host
buffers: the One-Euro rows' refusal and their two attachments, the merge of the track-box rule, and the 3D view's defaults against the
values testmodel.view3d_setup gave before it moved (recorded on that commit, as literals)."""
import types

import numpy as np
import pytest
import torch

from pam import _lib, stages


def one_euro_rows(ids, fresh, samples, max_tracks=4):
    """A stages.OneEuro without a handle whose 'pinned' twins hold these rows, in Handle.one_euro_buffers' layout."""
    n = len(ids)
    pose = np.zeros((1, max_tracks, 17, 3)); pose[0, :n] = np.arange(n * 51, dtype=np.float64).reshape(n, 17, 3)
    meta = np.zeros((1, 2 + 3 * max_tracks), dtype=np.int32)
    meta[0, :2] = n, sum(fresh)
    meta[0, 2:2 + 3 * n] = np.array([ids, fresh, samples]).T.reshape(-1)
    oe = stages.OneEuro.__new__(stages.OneEuro)
    oe.host = (pose, meta)
    return oe, pose[0, :n]


def record(ids):
    return dict(n_tracks=len(ids), tracks=[dict(track_id=i) for i in ids])


def test_one_euro_rows_attach_in_the_records_order():
    oe, pose = one_euro_rows([7, 3, 9], [1, 0, 1], [5, 2, 1])
    assert oe.fetched is False
    rec = record([7, 3, 9])
    f = oe.rows(rec)
    assert f['n_tracks'] == 3 and f['n_fresh'] == 2 and f['ids'].tolist() == [7, 3, 9] and np.array_equal(f['pose'], pose)
    oe.add_to(rec)                                       # FramePipeline.results()
    assert np.array_equal(rec['pose3d_filtered'], pose) and sorted(rec['filter_meta']) == ['fresh', 'ids', 'n_fresh', 'samples']
    assert rec['filter_meta']['fresh'].tolist() == [True, False, True] and rec['filter_meta']['samples'].tolist() == [5, 2, 1]
    assert rec['filter_meta']['n_fresh'] == 2 and rec['filter_meta']['ids'].tolist() == [7, 3, 9]
    # IterativeTracker._filter_attach: the same rows into the record's tracks
    from pam.tracker import IterativeTracker
    trk = IterativeTracker.__new__(IterativeTracker)
    trk.one_euro, trk._oe, trk.last = True, oe, dict(record([7, 3, 9]), status=0)
    trk._filter_attach()
    assert trk.last['one_euro']['ids'].tolist() == [7, 3, 9]
    for k, r in enumerate(trk.last['tracks']):
        assert np.array_equal(r['pose3d_filtered'], pose[k]) and (r['filter_fresh'], r['filter_samples']) == ([True, False, True][k], [5, 2, 1][k])
    trk.last = dict(record([]), status=_lib.ST_INPUT_VOID)   # a void frame's record lists no tracks: nothing is compared or attached
    trk._filter_attach()
    assert 'one_euro' not in trk.last


@pytest.mark.parametrize('ids', [[7, 3], [7, 9, 3], [7, 3, 9, 1], []])
def test_one_euro_rows_that_do_not_follow_the_record_are_refused(ids):
    oe, _ = one_euro_rows([7, 3, 9], [1, 1, 1], [1, 1, 1])
    rec = record(ids)
    for call in (oe.rows, oe.add_to):
        with pytest.raises(_lib.PamError, match='the One-Euro rows do not follow the record'):
            call(rec)
    assert 'pose3d_filtered' not in rec and 'filter_meta' not in rec


def test_pose_nms_kept_reads_the_filters_words():
    words = np.array([2, 0, 1] + [1, 2, -1, -1] + [-1] * 4 + [3, -1, -1, -1], dtype=np.int32)     # [n_det | keep_from], 3 views x 4 slots
    assert stages.PoseNmsOut.kept(words, 3, 4) == [[1, 2], [], [3]]


def test_track_boxes_merges_the_rule_with_the_defaults():
    seen = []
    h = _lib.Handle.__new__(_lib.Handle)
    h.C, h._h = 2, None
    h.lib = types.SimpleNamespace(pam_track_boxes=lambda *a: (seen.append(a[6:10]), 0)[1])
    boxes, count = torch.zeros((2, 4, 5)), torch.zeros(4, dtype=torch.int32)
    ids, info = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    h.track_boxes(0, 5, 360, 288, boxes, count, ids, info)
    h.track_boxes(0, 5, 360, 288, boxes, count, ids, info, pad_px=2, max_gap=1)
    h.track_boxes(0, 5, 360, 288, boxes, count, ids, info, **dict(_lib.TRACK_BOX_RULE, grow=1.5))
    assert seen == [(1.25, 8.0, 8.0, 3), (1.25, 2.0, 8.0, 1), (1.5, 8.0, 8.0, 3)]
    assert all(type(x) is t for row in seen for x, t in zip(row, (float, float, float, int)))
    assert _lib.TRACK_BOX_RULE == dict(grow=1.25, pad_px=8.0, min_size_px=8.0, max_gap=3)         # (the merge leaves the table alone)
    with pytest.raises(TypeError, match='margin'):
        h.track_boxes(0, 5, 360, 288, boxes, count, ids, info, margin=1.0)
    assert len(seen) == 3


VIEW3D_RIG = [(3, 0, 2.5), (-2, 3, 2.5), (-1, -3, 2)]
VIEW3D_DEFAULT = [[-703.5462646484375, 499.1363525390625, -135.2378387451172, 3848.197509765625],
                  [103.06881713867188, 72.16956329345703, -837.7183837890625, 3745.153076171875],
                  [-0.7424038648605347, -0.5198367834091187, -0.4226182699203491, 12.025617599487305]]
VIEW3D_BLOCK = {'SIZE': [320, 240], 'AZIMUTH': 20, 'ELEVATION': 40, 'UP': [0, 1, 0], 'MARGIN': 0.1}
VIEW3D_OF_BLOCK = [[-211.4042205810547, -102.84601593017578, -222.46604919433594, 2251.60009765625],
                   [83.56278991699219, -292.6643371582031, -30.41436767578125, 1370.351318359375],
                   [-0.7198463082313538, -0.6427876353263855, 0.2620026171207428, 10.216864585876465]]


def test_view3d_setup_gives_the_defaults_and_the_matrix_of_before(monkeypatch):
    from pam import testmodel, visualization as V
    monkeypatch.setattr(V, 'view3d_background', lambda cams, P, size, up=(0, 0, 1), device=None: ('background', size, tuple(up), str(device)))
    cams = [types.SimpleNamespace(position=np.array(p, dtype=np.float64)) for p in VIEW3D_RIG]
    model = types.SimpleNamespace(device='cpu', cameras=cams)
    for block, size, up, want in (({}, (640, 480), (0.0, 0.0, 1.0), VIEW3D_DEFAULT), (None, (640, 480), (0.0, 0.0, 1.0), VIEW3D_DEFAULT),
                                  (VIEW3D_BLOCK, (320, 240), (0.0, 1.0, 0.0), VIEW3D_OF_BLOCK),
                                  ({k.lower(): v for k, v in VIEW3D_BLOCK.items()}, (320, 240), (0.0, 1.0, 0.0), VIEW3D_OF_BLOCK)):
        v3 = V.view3d_setup(cams, block, torch.device('cpu'))
        assert v3['size'] == size and v3['background'] == ('background', size, up, 'cpu')
        assert v3['P'].dtype == np.float32 and v3['P'].shape == (3, 4) and v3['P'].tolist() == want
        assert v3['P_dev'].dtype == torch.float32 and tuple(v3['P_dev'].shape) == (1, 3, 4) and v3['P_dev'].reshape(3, 4).tolist() == want
        old = testmodel.view3d_setup(model, block)                                          # the facade's form of the same set-up
        assert sorted(old) == ['P', 'background'] and old['background'] == v3['background'] and torch.equal(old['P'], v3['P_dev'])
    with pytest.raises(ValueError, match=r"DATASET.VIEW3D: unknown key\(s\) \['zoom'\]"):
        testmodel.view3d_setup(model, {'ZOOM': 2})
    with pytest.raises(ValueError, match='unknown key'):
        V.view3d_setup(cams, dict(size=(64, 48), zoom=2), torch.device('cpu'))
