"""GPU: ViTPose through the HIP executor (hrnet_hip.HipViTPose) on the calibrated network of vitpose_calibrated.py.

Every stage -- the patch embedding, the blocks in runs of at most RUN, the last LayerNorm, each deconvolution, the heat-maps -- reads
the fp32 reference forward's own input to that stage rounded to bf16.  There is no fixed bound: each metric of
test_gpu_hrnet_modules.metrics of the executor against the fp32 network must stay within NET_FLOOR_RATIO (the project's 1.1) of the same
metric of the bf16_storage emulation (vitpose_calibrated.emulate: fp32 arithmetic, bf16 weights, a bf16 rounding wherever the executor
stores, P included) against the fp32 network; both are printed as PARITY lines.  Then the public surface: the whole network's heat-maps
under the same rule, replay == eager bits, the planted-peak decode statistic, predict() through the graph buckets, ViTPose-L (a run of
two blocks, one predict()), the ivclabpose facade built from configs/Shelf/model_configs_vitpose_b.yaml next to the CPU oracle tracker,
and FramePipeline(net=<ViTPose-B>) against the facade."""
import json
import os

import numpy as np
import pytest
import torch

import vitpose_calibrated as VC
from test_gpu_hrnet_modules import METRICS, NET_FLOOR_RATIO, bf, issue, knobs, metrics

pytestmark = pytest.mark.gpu
RUN = 6                         # blocks per checked run
RES = (256, 192)


class FloorChecker(object):
    """Collects, per compared output, the executor's and the emulation's metrics against fp32; fails with every metric above the ratio."""

    def __init__(self, test):
        self.test, self.bad = test, []

    def __call__(self, where, got, emu, ref):
        assert tuple(got.shape) == tuple(emu.shape) == tuple(ref.shape), (where, tuple(got.shape), tuple(emu.shape), tuple(ref.shape))
        m, f = metrics(got, ref), metrics(emu, ref)
        print('PARITY ' + json.dumps(dict(test=self.test, where=where, hip={k: round(m[k], 6) for k in METRICS},
                                          bf16_storage={k: round(f[k], 6) for k in METRICS})))
        self.bad += ['%s: %s %.4g > %.2f x %.4g' % (where, k, m[k], NET_FLOOR_RATIO, f[k]) for k in METRICS
                     if not m[k] <= NET_FLOOR_RATIO * f[k]]

    def done(self):
        assert not self.bad, '\n'.join(self.bad[:40])


class Env(object):
    pass


_ENVS = {}


def env_for(variant):
    from pam import hrnet_hip
    if variant not in _ENVS:
        _ENVS.clear()                                           # one network's weights on the device at a time
        torch.cuda.empty_cache()
        e = Env()
        e.dev = torch.device('cuda:0')
        folded = VC.folded_copy(variant)
        e.ref = copy_to(folded, e.dev)                          # fp32 weights: what both sides are measured against
        e.emu = VC.bf16_weights(folded).to(e.dev).eval()        # bf16 weights, fp32 arithmetic: the emulation's module
        head = folded.keypoint_head.final_layer
        folded.keypoint_head.final_layer = torch.nn.Identity()
        e.hip = hrnet_hip.HipViTPose(folded, e.dev)
        e.head = head.to(e.dev)
        _ENVS[variant] = e
    return _ENVS[variant]


def copy_to(model, dev):
    import copy
    return copy.deepcopy(model).to(dev).eval()


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


def _run_blocks(hip, blocks, x):
    for b in blocks:
        x = hip.block(b, x)
    return x


def _block_runs(e, chk, xin_of, first, last):
    """blocks first .. last - 1 in runs of RUN, each run reading the fp32 reference's own input (xin_of(b0): a map), rounded to bf16"""
    for b0 in range(first, last, RUN):
        b1 = min(last, b0 + RUN)
        xin = bf(xin_of(b0))
        names = ['block%d' % i for i in range(b0, b1)]
        r = xin.float()
        for s in names:
            r = VC.stage_forward(e.ref, s, r)
        emu = VC.emulate(e.emu, xin.float(), names)
        y = issue(e.hip, lambda: _run_blocks(e.hip, e.hip.blocks[b0:b1], xin))
        chk('blocks %d-%d' % (b0, b1 - 1), y, emu, r)


@pytest.mark.parametrize('n', [1, 5])
def test_every_stage_within_the_bf16_storage_floor(n):
    e = env_for('B')
    hip = e.hip
    assert hip.STAGES == ('patch',) + tuple('block%d' % i for i in range(12)) + ('norm', 'deconv0', 'deconv1')
    g = torch.Generator().manual_seed(4000 + n)
    x = torch.randn((n, 3) + RES, generator=g).to(torch.bfloat16).to(e.dev)
    t = VC.stage_inputs(e.ref, x.float())
    chk = FloorChecker('vitpose-b n%d' % n)
    with knobs(hip, stop_after='patch'):
        y = issue(hip, lambda: hip._features(_x8(x)))
    chk('patch', y, VC.emulate(e.emu, x.float(), ['patch']), t['patch'])
    _block_runs(e, chk, lambda b0: t['patch'] if b0 == 0 else t['block%d' % (b0 - 1)], 0, 12)
    prev = 'block11'
    for s in ('norm', 'deconv0', 'deconv1'):
        xin = bf(t[prev])
        r = VC.stage_forward(e.ref, s, xin.float())
        emu = VC.emulate(e.emu, xin.float(), [s])
        if s == 'norm':
            y = issue(hip, lambda: hip.layernorm(hip.last_norm, xin))
        else:
            y = issue(hip, lambda: hip.deconv(hip.deconvs[int(s[6:])], xin, relu=True))
        chk(s, y, emu, r)
        prev = s
    # the heat-maps: the product's head kernel (256 channels) on the last deconvolution's reference output; the emulation's head is fp32 too
    f = bf(t['deconv1'])
    hm = issue(hip, lambda: _head(e, f))
    with torch.no_grad():
        r = e.ref.keypoint_head.final_layer(f.float())
    assert metrics(hm, r)['all'] <= 1e-5                        # float32 on both sides: no bf16 rounding in this step
    # stop_after walks the same chain: the whole forward stopped at a late stage equals the chain issued piece by piece from the crops
    with knobs(hip, stop_after='block1'):
        a = issue(hip, lambda: hip._features(_x8(x))).clone()
    with knobs(hip, stop_after='patch'):
        p = issue(hip, lambda: hip._features(_x8(x)))
    b = issue(hip, lambda: _run_blocks(hip, hip.blocks[:2], p))
    assert torch.equal(a, b)
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


def test_vitpose_l_a_run_of_two_blocks():
    e = env_for('L')
    assert (e.hip.dim, e.hip.heads, e.hip.depth) == (1024, 16, 24) and len(e.hip.STAGES) == 28
    x = torch.randn((2, 3) + RES, generator=torch.Generator().manual_seed(4100)).to(torch.bfloat16).to(e.dev)
    chk = FloorChecker('vitpose-l n2')
    p = VC.stage_forward(e.ref, 'patch', x.float())
    with knobs(e.hip, stop_after='patch'):
        y = issue(e.hip, lambda: e.hip._features(_x8(x)))
    chk('patch', y, VC.emulate(e.emu, x.float(), ['patch']), p)
    _block_runs(e, chk, lambda b0: p, 0, 2)
    chk.done()


def _net(c='B', path=None, **kw):
    from pam import hrnet
    return hrnet.HRNetPose(c, 17, path, model_name='ViTPose', resolution=RES, **kw)


def test_vitpose_b_replay_equals_eager_and_within_the_bf16_floor(tmp_path):
    from pam import hrnet_hip, selfcheck
    path = os.path.join(str(tmp_path), 'vitpose-b.pth')
    torch.save({'state_dict': VC.calibrated('B')[0]}, path)
    n = 5
    net = _net('B', path, use_graph=True, max_crops=n)
    assert net.weights == path and net.variant == 'B' and net.model_name == 'ViTPose' and isinstance(net.hip, hrnet_hip.HipViTPose)
    assert not net._flag_sync_ok()
    ref = VC.folded_copy('B').to(net.device).eval()
    x = torch.randn((n, 3) + RES, generator=torch.Generator().manual_seed(81)).to(torch.bfloat16).to(net.device)
    x8 = net.input_buffer(n)
    x8.zero_()
    x8[:, :3] = x
    with torch.no_grad():
        h32 = ref(x.float())
    emu = VC.emulate(VC.bf16_weights(ref), x.float())
    hr = net.heatmaps(x8).clone()
    hr2 = net.heatmaps(x8).clone()
    with torch.no_grad():
        he = net._forward(x8, 'heatmaps').clone()
    torch.cuda.synchronize()
    assert tuple(hr.shape) == (n, 17, 64, 48) and (n, 'heatmaps', 0) in net._graphs and not any(net.flag_synced.values())
    assert torch.equal(hr, hr2) and torch.equal(hr, he)
    chk = FloorChecker('vitpose-b network n%d' % n)
    chk('heatmaps', he.float(), emu, h32)
    chk.done()
    st = selfcheck.drift_statistics(h32, he.float())
    print('DRIFT ' + json.dumps(st))
    assert st['planted_peak_max_cells']['16'] == 0, st


def _predict_case(net, boxes, batch_size):
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (288, 360, 3), dtype=np.uint8) for _ in range(len(boxes))]
    pbl = [[dict(image_id=0, category_id=1, score=0.9, bbox=b, data=frames[v], feature=[]) for b in bs] for v, bs in enumerate(boxes)]
    dump = net.predict(pbl, batch_size=batch_size)
    assert [len(v) for v in dump] == [len(b) for b in boxes]
    for v, items in enumerate(dump):
        for it, b in zip(items, boxes[v]):
            assert set(it) >= {'bbox', 'keypoints', 'keypoints_score', 'feature'}
            k = np.array(it['keypoints']).reshape(17, 3)
            assert np.isfinite(k).all() and np.allclose(k[:, 2], it['keypoints_score'])
            assert (k[:, 0] >= b[0] - 1e-3).all() and (k[:, 0] <= b[0] + b[2]).all()
            assert (k[:, 1] >= b[1] - 1e-3).all() and (k[:, 1] <= b[1] + b[3]).all()
    return pbl, dump


def _boxes(counts):
    rng = np.random.default_rng(7)
    return [[[float(rng.uniform(0, 150)), float(rng.uniform(0, 60)), float(rng.uniform(60, 200)), float(rng.uniform(120, 220))]
             for _ in range(c)] for c in counts]


def test_vitpose_b_predict_through_the_graph_buckets():
    """1, 5 and 20 crops: the buckets of 4, 8 and 20 crops are captured; a call split into smaller batches gives the same keypoints."""
    net = _net('B', None, use_graph=True, max_dets=8, graph_bucket=4)
    assert net.weights == 'random(seed=0)'
    for counts, bucket in (([1, 0], 4), ([3, 0, 2], 8), ([7, 6, 7], 20)):
        pbl, dump = _predict_case(net, _boxes(counts), 20)
        assert (bucket, 'features', 0) in net._graphs, (counts, sorted(net._graphs))
    dump2 = net.predict(pbl, batch_size=8)                      # 20 crops as 8 + 8 + 4
    for a, b in zip(dump, dump2):
        for ia, ib in zip(a, b):
            assert ia['keypoints'] == ib['keypoints']
    assert net.check_void() is False
    net.clear_void()


def test_vitpose_l_predict_one_crop():
    net = _net(1024, None, use_graph=True, max_dets=8, graph_bucket=4, max_crops=4)
    assert net.variant == 'L' and net.hip.depth == 24
    _predict_case(net, _boxes([1]), 20)
    assert (4, 'features', 0) in net._graphs


def _pose_cfg(tmp_path):
    from pam.dataset import GetConfig
    import pam
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_vitpose_b.yaml'))
    p = dict(cfg.POSE_MODELS.HRPOSE)
    assert p['C'] == 'B' and p['MODEL_NAME'] == 'ViTPose' and list(p['RESOLUTION']) == [256, 192]
    p['CHECKPOINT_FILE'] = os.path.join(str(tmp_path), 'vitpose-b.pth')
    torch.save({'state_dict': VC.calibrated('B')[0]}, p['CHECKPOINT_FILE'])
    return p


def test_facade_from_its_config_into_the_tracker_vs_the_oracle_and_frame_pipeline(tmp_path):
    """ivclabpose from model_configs_vitpose_b.yaml: PersonPoseDetect -> PersonTrack_Project3DPose next to the CPU oracle's tracker fed
    the same dump (ids, view sets bit-exact, 3D poses <= 1e-6); and FramePipeline(net=<the facade's ViTPose-B>) on the same frames and
    boxes ends every frame with the same tracker record as a FramePipeline fed the facade's device keypoints."""
    from pam import synth
    from pam.ivclabpose import ivclabpose
    from pam.pipeline import FramePipeline
    from oracle import cpu_ref as O
    seq = synth.make_sequence('S1', n_frames=8, seed=5, occlusion_every=5, birth_death_frame=4)
    cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, _pose_cfg(tmp_path), dict(cfg, NAME='Iterative'), conf)
    net = model.pose_model
    assert net.model_name == 'ViTPose' and net.variant == 'B' and tuple(net.resolution) == (256, 192) and net.weights.endswith('.pth')
    cams = model.GetCameraParameters(seq['calib'], 360, 288)
    ref = O.OracleIvclabpose(cfg, conf)
    ref.GetCameraParameters(seq['calib'], F=np.stack([c.F for c in cams]))
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (288, 360, 3), dtype=np.uint8) for _ in range(len(seq['frames'][0]))]
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
