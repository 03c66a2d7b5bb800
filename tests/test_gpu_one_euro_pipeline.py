"""GPU: the One-Euro filter through the Python layers, without a network.  On the golden trace S2 FramePipeline(one_euro=True) -- view
sharding and crop sharding, the tracker on the caller's stream and on its own -- gives the bits IterativeTracker(one_euro=True) gives,
on its host-list path (the facade) and on its device path (tracking_dev); the facade's pts3d_filtered follows the 9-tuple's ids; and
with the option off every entry point makes the calls into the library it made before the option existed."""
import numpy as np
import pytest
import torch

import golden_io as G
from pam import synth
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

MD, NF = 8, 60
SETUP = ('pam_create', 'pam_out_layout', 'pam_set_cameras', 'pam_set_lens', 'pam_set_input_guard', 'pam_set_one_euro', 'pam_last_error')


def _facade(one_euro):
    from pam.ivclabpose import ivclabpose
    tr, c = G.load('trace_S2.npz'), G.cameras('S2')
    cfg = dict(synth.MATCHER_CFG[str(tr['meta.dataset'])]); conf = cfg.pop('CONF_THRESHOLD')
    m = dict(cfg, NAME='Iterative')
    if one_euro is not None:
        m['ONE_EURO'] = one_euro
    model = ivclabpose({'NAME': ''}, None, m, conf, max_dets=MD, max_tracks=16)
    model.GetCameraParameters({'P': c['P'], 'K': c['K'], 'RT': c['RT']}, 0, 0, F=c['F'])
    return model, cfg, conf


@pytest.fixture(scope='module')
def s2():
    frames = G.trace_frames(G.load('trace_S2.npz'))[:NF]
    assert all(any(len(v) for v in views) for views in frames)
    return frames, synth.pack_frames(frames, MD)


def test_pipeline_and_tracker_paths_give_the_same_filtered_poses(s2):
    from pam.distributed import CropGather
    from pam.pipeline import FramePipeline
    from pam.tracker import IterativeTracker
    frames, (nd_all, dd_all) = s2
    model, cfg, conf = _facade({})
    cams, C = model.cameras, len(model.cameras)
    mk = lambda **kw: FramePipeline(cams, cfg, conf, (1080, 1920), max_dets=MD, max_tracks=16, hrnet=False, one_euro=True, **kw)
    views, over, crops = mk(), mk(overlap_tracker=True), mk(shard='crops')
    trk = IterativeTracker(model.tracker.args, max_dets=MD, max_tracks=16, one_euro=True)
    dev = views.device
    moved = 0
    for t in range(NF):
        pbl, dr = synth.to_dump_results(frames[t])
        tup = model.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')
        want = model.tracker.tracks
        nd = torch.tensor(nd_all[t], dtype=torch.int32, device=dev); dd = torch.tensor(dd_all[t], dtype=torch.float64, device=dev)
        trk.tracking_dev(t, cams, nd, dd)
        recs = []
        for p in (views, over):
            p.write_local(dd); p.track_step(t, nd)
            recs.append(p.results())
        vl = [v for v in range(C) for _ in range(nd_all[t][v])]
        sl = [s for v in range(C) for s in range(nd_all[t][v])]
        crops.write_send(dd)
        crops.track_step_crops(t, nd, torch.tensor(CropGather.select_index(vl, sl, C, MD, 1)[0], dtype=torch.int64, device=dev))
        recs.append(crops.results())
        for name, rec in zip(('views', 'overlap', 'crops'), recs):
            assert [x['track_id'] for x in rec['tracks']] == [x.track_id for x in want], (name, t)
            assert rec['pose3d_filtered'].shape == (len(want), 17, 3)
            for k, x in enumerate(want):
                assert rec['tracks'][k]['pose3d'].tobytes() == x.pose3d.tobytes(), (name, t, k)
                assert rec['pose3d_filtered'][k].tobytes() == x.pose3d_filtered.tobytes(), (name, t, k)
            f = rec['filter_meta']
            assert f['ids'].tolist() == [x.track_id for x in want] and f['fresh'].tolist() == [x.filter_fresh for x in want]
            assert f['samples'].tolist() == [x.filter_samples for x in want] and f['n_fresh'] == sum(x.filter_fresh for x in want)
        assert [x.track_id for x in trk.tracks] == [x.track_id for x in want]
        for x, y in zip(trk.tracks, want):
            assert x.pose3d_filtered.tobytes() == y.pose3d_filtered.tobytes() and (x.filter_fresh, x.filter_samples) == (y.filter_fresh, y.filter_samples)
        # the facade: pts3d_filtered is aligned with the 9-tuple's ids and pts3d
        by_id = {x.track_id: x for x in want}
        assert len(model.pts3d_filtered) == len(tup[5]) == len(tup[3])
        for i, pid in enumerate(tup[5]):
            assert by_id[int(pid)].emitted and np.array_equal(model.pts3d_filtered[i], by_id[int(pid)].pose3d_filtered.T)
            assert np.array_equal(np.asarray(tup[3][i]), by_id[int(pid)].pose3d.T)
        moved += sum(1 for x in want if not np.array_equal(x.pose3d_filtered, x.pose3d))
    assert moved > 100 and sum(x.emitted for x in want) >= 3
    # reset(): the pipeline's filters start over with its tracks
    views.reset()
    views.write_local(dd); views.track_step(NF, nd)
    rec = views.results()
    assert rec['n_tracks'] > 0 and rec['filter_meta']['samples'].tolist() == [1] * rec['n_tracks']
    assert all(rec['pose3d_filtered'][k].tobytes() == x['pose3d'].tobytes() for k, x in enumerate(rec['tracks']))


def test_option_off_makes_the_calls_of_before(s2):
    from pam.distributed import CropGather
    from pam.pipeline import FramePipeline
    from pam.tracker import IterativeTracker
    frames, (nd_all, dd_all) = s2
    on, cfg, conf = _facade({'BETA': 0.4})
    off, _, _ = _facade(None)
    cams, C = on.cameras, len(on.cameras)
    assert off.tracker.one_euro is None and off.tracker._oe is None and off.tracker.handle.one_euro_cfg is None
    mk = lambda **kw: FramePipeline(cams, cfg, conf, (1080, 1920), max_dets=MD, max_tracks=16, hrnet=False, **kw)
    p_off, p_on, c_off, c_on = mk(), mk(one_euro=True), mk(shard='crops'), mk(shard='crops', one_euro=True)
    assert p_off.one_euro is None and p_off._oe is None                           # off: nothing allocated
    t_off = IterativeTracker(off.tracker.args, max_dets=MD, max_tracks=16)
    t_on = IterativeTracker(off.tracker.args, max_dets=MD, max_tracks=16, one_euro=dict(freq=30))
    dev = p_off.device
    for t in range(3):
        pbl, dr = synth.to_dump_results(frames[t])
        nd = torch.tensor(nd_all[t], dtype=torch.int32, device=dev); dd = torch.tensor(dd_all[t], dtype=torch.float64, device=dev)
        sel = torch.tensor(CropGather.select_index([v for v in range(C) for _ in range(nd_all[t][v])],
                                                   [s for v in range(C) for s in range(nd_all[t][v])], C, MD, 1)[0], dtype=torch.int64, device=dev)
        got = {}
        for name, fn in (('facade off', lambda: off.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')),
                         ('facade on', lambda: on.PersonTrack_Project3DPose(t, pbl, dr, 'SVD')),
                         ('dev off', lambda: t_off.tracking_dev(t, cams, nd, dd)), ('dev on', lambda: t_on.tracking_dev(t, cams, nd, dd)),
                         ('views off', lambda: (p_off.write_local(dd), p_off.track_step(t, nd), p_off.results())),
                         ('views on', lambda: (p_on.write_local(dd), p_on.track_step(t, nd), p_on.results())),
                         ('crops off', lambda: (c_off.write_send(dd), c_off.track_step_crops(t, nd, sel), c_off.results())),
                         ('crops on', lambda: (c_on.write_send(dd), c_on.track_step_crops(t, nd, sel), c_on.results()))):
            with recorded_calls() as calls:
                fn()
            got[name] = [c for c in calls if c not in SETUP]                                 # (a tracker opens its handle on its first frame)
        # the parent's lists, spelled out
        assert got['facade off'] == ['pam_frame'] and got['facade on'] == ['pam_frame', 'pam_one_euro', 'pam_sync']
        assert got['dev off'] == ['pam_frame_dev', 'pam_fetch', 'pam_sync']
        assert got['dev on'] == ['pam_frame_dev', 'pam_one_euro', 'pam_fetch', 'pam_sync']
        assert got['views off'] == ['pam_frame_dev_views', 'pam_fetch'] and got['views on'] == ['pam_frame_dev_views', 'pam_one_euro', 'pam_fetch']
        assert got['crops off'] == ['pam_frame_dev', 'pam_fetch'] and got['crops on'] == ['pam_frame_dev', 'pam_one_euro', 'pam_fetch']
    assert 'pose3d_filtered' not in p_off.results() and 'filter_meta' not in c_off.results()
    assert t_on.handle.one_euro_cfg.freq == 30.0 and t_on.tracks[0].pose3d_filtered is not None and t_off.tracks[0].pose3d_filtered is None
    with pytest.raises(ValueError):
        mk(one_euro=dict(freq=0))
    with pytest.raises(ValueError):
        IterativeTracker(off.tracker.args, max_dets=MD, max_tracks=16, one_euro=dict(cutoff=1.0))
