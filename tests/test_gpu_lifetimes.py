"""GPU: a dropped FramePipeline or IterativeTracker is freed by reference count alone -- no object of the host side reaches itself, so
its handle (pam_destroy), its streams and its share of a network's captured graphs go where the owner drops it, not where the cycle
collector next runs (handles freed in the middle of a later test's frame, and with them captures, preceded the one
segmentation fault inside hipGraphLaunch this suite has seen).  Each object runs one frame first, so that whatever a step stores has
been stored; the collector is off while the last reference goes.  Tracker only on the golden trace S1, max_dets 8; the network case:
HRNet-W32 at 256 x 192 with random weights, 2 views, 3 boxes -- the pipeline dies, the network stays."""
import gc
import weakref

import numpy as np
import pytest
import torch

import golden_io as G
from pam import _lib, synth
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu

MD, HW = 8, (288, 360)


@pytest.fixture(scope='module')
def s1():
    from pam.ivclabpose import ivclabpose
    tr, c = G.load('trace_S1.npz'), G.cameras('S1')
    cfg = dict(synth.MATCHER_CFG[str(tr['meta.dataset'])]); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, None, dict(cfg, NAME='Iterative'), conf, max_dets=MD, max_tracks=16)
    model.GetCameraParameters({'P': c['P'], 'K': c['K'], 'RT': c['RT']}, 0, 0, F=c['F'])
    frames = G.trace_frames(tr)[:1]
    nd, dd = synth.pack_frames(frames, MD)
    lens = _lib.lens_table(c['K'], np.tile([-0.1, 0.02, 1e-3, -1e-3, 0.0], (len(model.cameras), 1)))
    return dict(model=model, cams=model.cameras, cfg=cfg, conf=conf, lens=lens,
                nd=torch.tensor(nd[0], dtype=torch.int32, device='cuda:0'), dd=torch.tensor(dd[0], dtype=torch.float64, device='cuda:0'))


@pytest.fixture(scope='module')
def w32():
    from pam import hrnet
    net = hrnet.HRNetPose(32, 17, None, resolution=(256, 192), use_graph=True, max_dets=MD, autotune=False)
    for _ in range(3):                                   # the forward the step replays is captured up front
        net.features(net.input_buffer(3))
    torch.cuda.synchronize()
    return net


def dies_where_it_is_dropped(box):
    """box: a one-element list that holds the ONLY strong reference to an object with a ``handle``."""
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        obj, handle = weakref.ref(box[0]), weakref.ref(box[0].handle)
        with recorded_calls() as calls:
            box.clear()
            gone = list(calls)
        assert obj() is None, 'the object reaches itself: it waits for the cycle collector'
        assert handle() is None, 'the handle outlives its owner'
        assert gone.count('pam_destroy') == 1, gone
    finally:
        gc.enable()


PIPELINES = {
    'plain': dict(),
    'one_euro': dict(one_euro=True),
    'overlap_one_euro': dict(overlap_tracker=True, one_euro=True),
    'lens': dict(lens='table'),
    'view3d': dict(overlay=dict(view3d=dict(size=(64, 48)))),
}


@pytest.mark.parametrize('form', sorted(PIPELINES))
def test_a_dropped_pipeline_is_freed_by_reference_count(s1, form):
    from pam.pipeline import FramePipeline
    kw = dict(PIPELINES[form])
    if 'lens' in kw:
        kw['lens'] = s1['lens']
    box = [FramePipeline(s1['cams'], s1['cfg'], s1['conf'], HW, max_dets=MD, max_tracks=16, hrnet=False, **kw)]
    p = box[0]
    p.write_local(s1['dd'])
    p.undistort_local(s1['nd'])                          # (no launch without a table)
    p.track_step(0, s1['nd'])
    rec = p.results()
    assert rec['frame_id'] == 0 and ('pose3d_filtered' in rec) == ('one_euro' in kw)
    if 'overlay' in kw:
        out = p.overlay_step([torch.zeros(HW + (3,), dtype=torch.uint8, device=p.device) for _ in p.mine])
        assert tuple(out[-1].shape) == (48, 64, 3)
        del out
    del p, rec
    dies_where_it_is_dropped(box)


def test_a_dropped_tracker_is_freed_by_reference_count(s1):
    from pam.tracker import IterativeTracker
    box = [IterativeTracker(s1['model'].tracker.args, max_dets=MD, max_tracks=16, one_euro=True)]
    box[0].tracking_dev(0, s1['cams'], s1['nd'], s1['dd'])
    assert box[0].last['frame_id'] == 0 and 'one_euro' in box[0].last
    dies_where_it_is_dropped(box)


def test_a_dropped_pipeline_leaves_its_network_alive(w32):
    from pam.ivclabpose import Camera, fundamental_matrices
    from pam.pipeline import FramePipeline
    calib = synth.make_sequence('S1', n_frames=1, seed=3)['calib']
    P, K, RT = (calib[k][:2].astype(np.float32) for k in ('P', 'K', 'RT'))
    F = fundamental_matrices(K, RT)
    cams = [Camera(j, P[j], K[j], RT[j], F[j], w=HW[1], h=HW[0]) for j in range(2)]
    cfg = dict(synth.MATCHER_CFG['Shelf']); cfg.pop('CONF_THRESHOLD')
    cfg.update(EPI_THRESHOLD=1e6, INIT_THRESHOLD=1e6, JOINT_THRESHOLD=1e6)
    box = [FramePipeline(cams, cfg, -1e6, HW, max_dets=MD, net=w32, pose_nms=True)]
    p, dev = box[0], box[0].device
    frames = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (2,) + HW + (3,), dtype=np.uint8)).to(dev)
    ptrs = torch.tensor([frames[v].data_ptr() for v in range(2)], dtype=torch.int64, device=dev)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    boxes = torch.tensor([[20.0, 30.0, 80.0, 160.0], [200.0, 60.0, 100.0, 200.0], [10.0, 20.0, 90.0, 180.0]], dtype=torch.float32, device=dev)
    graphs = len(w32._graphs)
    p.pose_step(ptrs, i32([0, 0, 1]), i32([0, 1, 0]), boxes, n_det=i32([2, 1]))
    p.track_step(0, p.nms_n_det)
    assert len(p.results()['pose_nms']['n_det']) == 2
    del p
    dies_where_it_is_dropped(box)
    assert len(w32._graphs) == graphs                    # the captures stay with the network
    w32.features(w32.input_buffer(3))
    torch.cuda.synchronize()
