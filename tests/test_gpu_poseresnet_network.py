"""GPU: PoseResNet through the HIP executor (hrnet_hip.HipPoseResNet) on the calibrated network of poseresnet_calibrated.py (non-trivial
folded biases, per-channel scales, a non-zero head bias).  Every stage -- stem, layer1-4, each deconvolution, the heat-maps -- reads the
fp32 reference forward's own input to that stage rounded to bf16 and is compared with the fp32 stage on bf16-rounded weights
(test_gpu_hrnet_modules.metrics; bounds: TOL).  Then the public surface: the fused and un-fused layer1, replay == eager per configuration,
the planted-peak decode statistic, predict() through the graph buckets, the ivclabpose facade built from
configs/Shelf/model_configs_poseresnet50.yaml next to the CPU oracle tracker, and FramePipeline(net=<PoseResNet>) against the facade."""
import json
import os

import numpy as np
import pytest
import torch

import poseresnet_calibrated as PC
from test_gpu_hrnet_modules import METRICS, Checker, bf, issue, knobs, metrics

pytestmark = pytest.mark.gpu

# stage / head bounds of HRNet's per-module tests (test_gpu_hrnet_modules.TOL: 0.015) for R50; the deeper networks have 2 x / 3 x the
# blocks in layer3 and layer2-3, each block one more bf16 rounding of the residual stream, hence 0.03
TOL = {'r50': {k: 0.015 for k in METRICS}, 'deep': {k: 0.03 for k in METRICS}}
CASES = [(50, (256, 192), 1), (50, (256, 192), 5), (50, (256, 192), 20), (50, (384, 288), 1), (50, (384, 288), 5),
         (101, (256, 192), 1), (101, (256, 192), 5), (152, (256, 192), 1), (152, (256, 192), 5)]
RUN = 6                         # blocks per checked run of a stage (R50's longest layer)
NET_FLOOR_RATIO = 1.1           # as test_gpu_hrnet_modules.py: the whole network's heat-map error within 1.1 x what bf16 storage alone costs
STAGES = ('stem', 'layer1', 'layer2', 'layer3', 'layer4', 'deconv0', 'deconv1', 'deconv2')


class RChecker(Checker):
    def __call__(self, family, where, got, ref):
        assert tuple(got.shape) == tuple(ref.shape), (where, tuple(got.shape), tuple(ref.shape))
        m = metrics(got, ref)
        print('PARITY ' + json.dumps(dict(test=self.test, family=family, where=where, **{k: round(v, 6) for k, v in m.items()})))
        self.bad += ['%s %s: %s %.4g > %.4g' % (family, where, k, m[k], TOL[family][k]) for k in METRICS if not m[k] <= TOL[family][k]]


class Env(object):
    pass


_ENVS = {}


def env_for(depth):
    from pam import hrnet_hip
    if depth not in _ENVS:
        e = Env()
        e.dev = torch.device('cuda:0')
        folded = PC.folded_copy(depth)
        e.ref = PC.bf16_weights(folded).to(e.dev).eval()
        head = folded.final_layer
        folded.final_layer = torch.nn.Identity()
        e.hip = hrnet_hip.HipPoseResNet(folded, e.dev)
        e.head = head.to(e.dev)
        _ENVS.clear()                                           # one network's weights on the device at a time
        _ENVS[depth] = e
    return _ENVS[depth]


@pytest.fixture(autouse=True, scope='module')
def _no_tf32():
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved
    _ENVS.clear()


def _x8(x):
    n, _, h, w = x.shape
    return bf(torch.cat([x, torch.zeros((n, 5, h, w), dtype=x.dtype, device=x.device)], 1))


@pytest.mark.parametrize('depth,res,n', CASES, ids=['r%d-%dx%d-n%d' % (d, r[0], r[1], n) for d, r, n in CASES])
def test_every_stage_vs_fp32(depth, res, n):
    e = env_for(depth)
    hip, ref = e.hip, e.ref
    g = torch.Generator().manual_seed(3000 + 31 * n + res[0] + depth)
    x = torch.randn((n, 3) + res, generator=g).to(torch.bfloat16).to(e.dev)
    t = PC.stage_inputs(ref, x.float())
    fam = 'r50' if depth == 50 else 'deep'
    chk = RChecker('r%d %dx%d n%d' % (depth, res[0], res[1], n))
    dl = ref.deconv_layers
    for cfg in hip.CONFIGS:
        with knobs(hip, **hip.CONFIGS[cfg], stop_after='stem'):
            y = issue(hip, lambda: hip._features(_x8(x)))
        chk(fam, 'stem', y, t['stem'])
        with knobs(hip, **hip.CONFIGS[cfg]):
            y = issue(hip, lambda: hip._layer1(bf(t['stem'])))
        chk(fam, 'layer1 %s' % cfg, y, t['layer1'])
    for k in range(3):
        # a stage is checked in runs of at most RUN blocks, each reading the reference's own input to the run: R152's layer3 (36 blocks) as
        # one piece showed 0.031 (ch16 0.039) -- six times the bf16 roundings of the residual stream of R50's longest layer (6 blocks)
        blocks, rlayer = hip.layers[k], getattr(ref, 'layer%d' % (k + 2))
        xin = bf(t['layer%d' % (k + 1)])
        for b0 in range(0, len(blocks), RUN):
            with torch.no_grad():
                r = rlayer[b0:b0 + RUN](xin.float())
            y = issue(hip, lambda: _run_layer(hip, blocks[b0:b0 + RUN], xin))
            chk(fam, 'layer%d blocks %d-%d' % (k + 2, b0, min(len(blocks), b0 + RUN) - 1), y, r)
            xin = bf(r)
    prev = 'layer4'
    for k in range(3):
        xin = bf(t[prev])
        with torch.no_grad():
            r = dl[3 * k + 2](dl[3 * k + 1](dl[3 * k](xin.float())))
        y = issue(hip, lambda: hip.deconv(hip.deconvs[k], xin, relu=True))
        chk(fam, 'deconv%d' % k, y, r)
        prev = 'deconv%d' % k
    # the heat-maps: the product's head kernel (pam_head_heatmaps, 256 channels) on the last deconvolution's reference output
    f = bf(t['deconv2'])
    hm = issue(hip, lambda: _head(e, f))
    with torch.no_grad():
        r = ref.final_layer(f.float())
    chk(fam, 'heatmaps', hm, r)
    chk.done()


def _head(e, f):
    import ctypes as C
    n, c, h, w = f.shape
    hw = e.head.weight.detach().float().reshape(17, c).contiguous()
    hb = e.head.bias.detach().float().contiguous()
    hm = torch.empty((n, 17, h, w), dtype=torch.float32, device=f.device, memory_format=torch.channels_last)
    rc = e.hip.lib.pam_head_heatmaps(C.c_void_p(torch.cuda.current_stream(f.device).cuda_stream), n * h * w, C.c_void_p(f.data_ptr()), c,
                                     C.c_void_p(hw.data_ptr()), C.c_void_p(hb.data_ptr()), 17, C.c_void_p(hm.data_ptr()))
    assert rc == 0
    return hm


def _run_layer(hip, layer, x):
    for b in layer:
        x = hip._bottleneck(b, x)
    return x


def _net(depth=50, res=(256, 192), path=None, **kw):
    from pam import hrnet
    return hrnet.HRNetPose(depth, 17, path, model_name='PoseResNet', resolution=res, **kw)


def test_pose_resnet_replay_equals_eager_and_within_the_bf16_floor(tmp_path):
    from pam import hrnet_hip, selfcheck
    path = os.path.join(str(tmp_path), 'pose_resnet_50_256x192.pth')
    torch.save(PC.calibrated(50)[0], path)
    n, res = 20, (256, 192)
    net = _net(50, res, path, use_graph=True, max_crops=n)
    assert net.weights == path and net.depth == 50 and isinstance(net.hip, hrnet_hip.HipPoseResNet) and not net._flag_sync_ok()
    ref = PC.folded_copy(50).to(net.device).eval()
    x = torch.randn((n, 3) + res, generator=torch.Generator().manual_seed(79)).to(torch.bfloat16).to(net.device)
    x8 = net.input_buffer(n)
    x8.zero_()
    x8[:, :3] = x
    with torch.no_grad():
        h32 = ref(x.float())
        floor = float((PC.bf16_storage(ref)(x.float()) - h32).norm() / h32.norm())
    for name in hrnet_hip.HipPoseResNet.CONFIGS:
        net.config_for = lambda k, name=name: name
        net.drop_captures()
        hr = net.heatmaps(x8).clone()
        hr2 = net.heatmaps(x8).clone()
        assert net.hip.config_name == name and not any(net.flag_synced.values())
        with torch.no_grad():
            he = net._forward(x8, 'heatmaps').clone()
        torch.cuda.synchronize()
        assert tuple(hr.shape) == (n, 17, 64, 48)
        assert torch.equal(hr, hr2) and torch.equal(hr, he), name
        rel = float((he.float() - h32).norm() / h32.norm())
        print('R50 NETWORK config=%s rel=%.5f floor=%.5f' % (name, rel, floor))
        assert rel <= NET_FLOOR_RATIO * floor, (name, rel, floor)
        if name == hrnet_hip.HipPoseResNet.config_name:
            st = selfcheck.drift_statistics(h32, he.float())
            print('DRIFT ' + json.dumps(st))
            assert st['planted_peak_max_cells']['16'] == 0, st


def test_pose_resnet_predict_dump_format_through_the_graph_buckets():
    net = _net(50, (256, 192), None, use_graph=True, max_dets=8, graph_bucket=4)
    assert net.weights == 'random(seed=0)'
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (288, 360, 3), dtype=np.uint8) for _ in range(3)]
    boxes = [[[20.0, 30.0, 100.0, 200.0], [150.5, 40.25, 90.0, 180.0], [10.0, 5.0, 60.0, 120.0]], [], [[200.0, 60.0, 120.0, 210.0]]]
    pbl = [[dict(image_id=0, category_id=1, score=0.9, bbox=b, data=frames[v], feature=[]) for b in bs] for v, bs in enumerate(boxes)]
    dump = net.predict(pbl, batch_size=20)
    assert [len(v) for v in dump] == [3, 0, 1] and (4, 'features', 0) in net._graphs
    for v, items in enumerate(dump):
        for it, b in zip(items, boxes[v]):
            assert set(it) >= {'bbox', 'keypoints', 'keypoints_score', 'feature'}
            k = np.array(it['keypoints']).reshape(17, 3)
            assert np.allclose(k[:, 2], it['keypoints_score'])
            assert (k[:, 0] >= b[0] - 1e-3).all() and (k[:, 0] <= b[0] + b[2]).all()
            assert (k[:, 1] >= b[1] - 1e-3).all() and (k[:, 1] <= b[1] + b[3]).all()
    dump2 = net.predict(pbl, batch_size=3)
    for a, b in zip(dump, dump2):
        for ia, ib in zip(a, b):
            assert ia['keypoints'] == ib['keypoints']
    assert net.check_void() is False
    net.clear_void()


def _pose_cfg(tmp_path):
    from pam.dataset import GetConfig
    import pam
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_poseresnet50.yaml'))
    p = dict(cfg.POSE_MODELS.HRPOSE)
    assert p['C'] == 50 and p['MODEL_NAME'] == 'PoseResNet' and list(p['RESOLUTION']) == [256, 192]
    p['CHECKPOINT_FILE'] = os.path.join(str(tmp_path), 'pose_resnet_50_256x192.pth')
    torch.save({'model': PC.calibrated(50)[0]}, p['CHECKPOINT_FILE'])
    return p


def _rig_frames(seq):
    rng = np.random.default_rng(2)
    return [rng.integers(0, 256, (288, 360, 3), dtype=np.uint8) for _ in range(len(seq['frames'][0]))]


def test_facade_from_its_config_into_the_tracker_vs_the_oracle_and_frame_pipeline(tmp_path):
    """ivclabpose from model_configs_poseresnet50.yaml: PersonPoseDetect -> PersonTrack_Project3DPose next to the CPU oracle's tracker fed
    the same dump (ids, view sets bit-exact, 3D poses <= 1e-6); and FramePipeline(net=<the facade's PoseResNet>) on the same frames and
    boxes ends every frame with the same tracker record as a FramePipeline fed the facade's device keypoints."""
    from pam import synth
    from pam.ivclabpose import ivclabpose
    from pam.pipeline import FramePipeline
    from oracle import cpu_ref as O
    seq = synth.make_sequence('S1', n_frames=8, seed=5, occlusion_every=5, birth_death_frame=4)
    cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, _pose_cfg(tmp_path), dict(cfg, NAME='Iterative'), conf)
    net = model.pose_model
    assert net.model_name == 'PoseResNet' and net.depth == 50 and tuple(net.resolution) == (256, 192) and net.weights.endswith('.pth')
    cams = model.GetCameraParameters(seq['calib'], 360, 288)
    ref = O.OracleIvclabpose(cfg, conf)
    ref.GetCameraParameters(seq['calib'], F=np.stack([c.F for c in cams]))
    frames = _rig_frames(seq)
    V, md = len(frames), 8
    dev = net.device
    pipe = FramePipeline(cams, cfg, conf, (288, 360), max_dets=md, net=net)
    fed = FramePipeline(cams, cfg, conf, (288, 360), max_dets=md, hrnet=False)
    dframes = [torch.from_numpy(f).to(dev).contiguous() for f in frames]
    ptrs = torch.tensor([f.data_ptr() for f in dframes], dtype=torch.int64, device=dev)
    n_det = 0
    for t, views in enumerate(seq['frames']):
        pbl, _ = synth.to_dump_results(views)
        for v, persons in enumerate(pbl):
            for p in persons:
                p['data'] = frames[v]
        dump = model.PersonPoseDetect(imagelist=None, person_bbox_list=pbl, batch_size=20)
        plain = [[dict(it) for it in v] for v in dump]
        n_det += sum(len(v) for v in plain)
        a = model.PersonTrack_Project3DPose(t, pbl, dump, 'SVD')
        b = ref.PersonTrack_Project3DPose(t, pbl, plain, 'SVD')
        assert list(a[5]) == list(b[5]), (t, a[5], b[5])
        assert [list(map(int, c)) for c in a[0]] == [list(map(int, c)) for c in b[0]]
        assert a[4] == b[4]
        if len(a[5]):
            assert np.abs(np.asarray(a[3]) - np.asarray(b[3])).max() < 1e-6
        # the same crops through FramePipeline's own pose step
        vl = [v for v in range(V) for _ in pbl[v]]
        sl = [s for v in range(V) for s in range(len(pbl[v]))]
        bx = [list(p['bbox']) for v in range(V) for p in pbl[v]]
        cnt = torch.tensor([len(pbl[v]) for v in range(V)], dtype=torch.int32, device=dev)
        if vl:
            pipe.pose_step(ptrs, torch.tensor(vl, dtype=torch.int32, device=dev), torch.tensor(sl, dtype=torch.int32, device=dev),
                           torch.tensor(bx, dtype=torch.float32, device=dev))
        pipe.track_step(t, cnt)
        ra = pipe.results()
        rows = torch.zeros((V, md, 17, 3), dtype=torch.float64, device=dev)
        rows[:, :dump.device_det.shape[1]] = dump.device_det[:, :md]
        fed.track_step(t, cnt, rows)
        rb = fed.results()
        assert ra['n_tracks'] == rb['n_tracks'], t
        for ta, tb in zip(ra['tracks'], rb['tracks']):
            assert ta['track_id'] == tb['track_id'] and ta['emitted'] == tb['emitted'], t
            if ta['emitted']:
                assert np.array_equal(ta['pose3d'], tb['pose3d']), t
    assert n_det > 0
