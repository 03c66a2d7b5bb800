"""GPU: HRNet-W32 (256 x 192 crops) through the HIP executor, piece by piece and whole, on the calibrated W32 network of
hrnet_calibrated_w.py (non-trivial folded biases and per-channel scales), with test_gpu_hrnet_modules.py's metrics and tolerances
(TOL there, unchanged) at 1, 5 and 20 crops: stem + layer1, the four transitions, every output of all eight HR modules in every
HipHRNetW32 configuration.  Then the public surface: HRNetPose(32, ...) heat-maps vs fp32, replay == eager in every configuration,
predict() through the graph buckets, and the ivclabpose facade built from configs/Shelf/model_configs_w32.yaml feeding the tracker
next to the CPU oracle tracker fed the same keypoints."""
import os

import numpy as np
import pytest
import torch

import hrnet_calibrated_w as HW
from test_gpu_hrnet_modules import Checker, bf, issue, knobs

pytestmark = pytest.mark.gpu

RES = (256, 192)
CROPS = [1, 5, 20]
STAGES = [('stage2', 0), ('stage3', 0), ('stage3', 1), ('stage3', 2), ('stage3', 3), ('stage4', 0), ('stage4', 1), ('stage4', 2)]


class Env(object):
    pass


@pytest.fixture(scope='module')
def env():
    from pam import hrnet_hip
    saved = (torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    e = Env()
    e.dev = torch.device('cuda:0')
    folded = HW.folded_copy(32)
    e.ref = HW.bf16_weights(folded).to(e.dev).eval()
    e.hip = hrnet_hip.HipHRNetW32(folded, e.dev)
    e.taps = {}
    try:
        yield e
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def taps(e, n):
    if n not in e.taps:
        g = torch.Generator().manual_seed(2000 + 31 * n)
        x = torch.randn((n, 3) + RES, generator=g).to(torch.bfloat16).to(e.dev)
        e.taps[n] = (x, HW.stage_inputs(e.ref, x.float()))
    return e.taps[n]


@pytest.mark.parametrize('n', CROPS)
def test_w32_head_vs_fp32(env, n):
    e, hip = env, env.hip
    x, t = taps(e, n)
    x8 = bf(torch.cat([x, torch.zeros((n, 5) + RES, dtype=x.dtype, device=x.device)], 1))
    chk = Checker('w32 head n%d' % n)
    for fused in (True, False):
        with knobs(hip, fuse_stem=fused, fuse_tail=fused, fuse_bneck=fused, fuse_bneck0=fused):
            y = issue(hip, lambda: hip._head(x8))
        chk('head', 'fused=%s' % fused, y, t['layer1'])
    chk.done()


@pytest.mark.parametrize('n', CROPS)
def test_w32_transitions_vs_fp32(env, n):
    e, hip, ref = env, env.hip, env.ref
    t = taps(e, n)[1]
    chk = Checker('w32 transitions n%d' % n)
    cases = [('t1[0]', hip.t1[0], bf(t['layer1']), ref.transition1[0]), ('t1[1]', hip.t1[1], bf(t['layer1']), ref.transition1[1]),
             ('t2', hip.t2, bf(t['stage3'][0][1]), ref.transition2[2]), ('t3', hip.t3, bf(t['stage4'][0][2]), ref.transition3[3])]
    for name, op, xin, sub in cases:
        with torch.no_grad():
            r = sub(xin.float())
        y = issue(hip, lambda: hip.conv(op, xin, relu=True))
        chk('transition', name, y, r)
    chk.done()


def _cases():
    from pam.hrnet_hip import HipHRNetW32
    base = dict(HipHRNetW32.CONFIGS[HipHRNetW32.config_name], merge_fuse=True, merge_up=True, multi_stream=True)
    cases = {}
    for name, cfg in HipHRNetW32.CONFIGS.items():
        for ms in (True, False):
            cases['%s-%s' % (name, 'ms' if ms else '1s')] = dict(base, **cfg, multi_stream=ms)
    cases['no_merge_fuse'] = dict(base, merge_fuse=False)
    cases['no_merge_up'] = dict(base, merge_up=False)
    return cases


CASES = _cases()


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('n', CROPS)
def test_w32_every_output_of_every_hr_module_vs_fp32(env, n, case):
    e, hip = env, env.hip
    chk = Checker('w32 modules n%d %s' % (n, case))
    t = taps(e, n)[1]
    with knobs(hip, **CASES[case]):
        for stage, m in STAGES:
            xs = [bf(q) for q in t[stage][m]]
            with torch.no_grad():
                r = getattr(e.ref, stage)[m]([q.float() for q in xs])
            out = issue(hip, lambda: hip._hr_module(getattr(hip, stage)[m], xs))
            assert len(out) == len(r), (stage, m)
            for i, (y, q) in enumerate(zip(out, r)):
                chk(stage, '%s[%d] out%d' % (stage, m, i), y, q)
    chk.done()


def test_w32_fused_blocks_are_bit_identical_inside_the_modules(env):
    """The whole W32 feature stack with the 32-channel blocks fused (k_bblock2_32) and as two k_conv3x3<32> launches: bit-identical."""
    e, hip = env, env.hip
    x, _ = taps(e, 5)
    x8 = bf(torch.cat([x, torch.zeros((5, 5) + RES, dtype=x.dtype, device=x.device)], 1))
    outs = []
    for cfg in ('w32_fused', 'w32_unfused'):
        with knobs(hip, **hip.CONFIGS[cfg]):
            outs.append(issue(hip, lambda: hip._features(x8)).clone())
    assert torch.equal(outs[0], outs[1])


NET_FLOOR_RATIO = 1.1           # as test_gpu_hrnet_modules.py: the heat-maps' error within 1.1 x what bf16 storage alone costs


def test_w32_pose_vs_fp32_and_replay_equals_eager_in_every_configuration(tmp_path):
    from pam import hrnet, hrnet_hip
    path = os.path.join(str(tmp_path), 'pose_hrnet_w32_256x192.pth')
    torch.save(HW.calibrated(32)[0], path)
    n = 3
    net = hrnet.HRNetPose(32, 17, path, resolution=RES, use_graph=True, max_crops=n)
    assert net.weights == path and net.width == 32 and isinstance(net.hip, hrnet_hip.HipHRNetW32)
    ref = HW.folded_copy(32).to(net.device).eval()
    x = torch.randn((n, 3) + RES, generator=torch.Generator().manual_seed(78)).to(torch.bfloat16).to(net.device)
    x8 = net.input_buffer(n)
    x8.zero_()
    x8[:, :3] = x
    with torch.no_grad():
        h32 = ref(x.float())
        floor = float((HW.bf16_storage(ref)(x.float()) - h32).norm() / h32.norm())
    bad = []
    for name in hrnet_hip.HipHRNetW32.CONFIGS:
        net.config_for = lambda k, name=name: name
        net.drop_captures()
        hr = net.heatmaps(x8).clone()
        hr2 = net.heatmaps(x8).clone()
        assert net.hip.config_name == name
        with torch.no_grad():
            he = net._forward(x8, 'heatmaps').clone()
        torch.cuda.synchronize()
        assert tuple(hr.shape) == (n, 17, 64, 48)
        assert torch.equal(hr, hr2) and torch.equal(hr, he), name
        rel = float((he.float() - h32).norm() / h32.norm())
        print('W32 NETWORK config=%s rel=%.5f floor=%.5f' % (name, rel, floor))
        if not rel <= NET_FLOOR_RATIO * floor:
            bad.append('%s: heat-map rel err %.4g > %.2f x the bf16 floor %.4g' % (name, rel, NET_FLOOR_RATIO, floor))
    assert not bad, bad


def test_w32_random_weights_vs_fp32():
    """HRNetPose(32, 17, None, resolution=(256, 192)) -- the product's seeded random weights -- as test_gpu_image.py checks W48 at 256 x 192."""
    from pam import hrnet
    net = hrnet.HRNetPose(32, 17, None, resolution=RES, use_graph=True)
    dev = net.device
    ref = hrnet.fold_batchnorm(hrnet.init_random(hrnet.PoseHighResolutionNet(32, 17), seed=0)).to(dev).eval()
    x32 = torch.randn((3, 3) + RES, generator=torch.Generator().manual_seed(4)).to(dev)
    x8 = torch.cat([x32, torch.zeros((3, 5) + RES, device=dev)], dim=1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        h32 = ref(x32.to(torch.bfloat16).float())
        hb = net.heatmaps(x8).clone()
        he = hrnet.HRNetPose(32, 17, None, resolution=RES, use_graph=False).heatmaps(x8)
    torch.cuda.synchronize()
    assert tuple(hb.shape) == (3, 17, 64, 48)
    assert torch.equal(hb, he)
    rel = ((hb.float() - h32).norm() / h32.norm()).item()
    assert rel < 0.03, rel


def _w32_pose_cfg():
    from pam.dataset import GetConfig
    import pam
    cfg = GetConfig(os.path.join(os.path.dirname(pam.__file__), 'configs', 'Shelf', 'model_configs_w32.yaml'))
    p = dict(cfg.POSE_MODELS.HRPOSE)
    assert p['C'] == 32 and list(p['RESOLUTION']) == [256, 192]
    p['CHECKPOINT_FILE'] = ''                                      # no checkpoint file here: the seeded random weights
    return p


def test_w32_predict_dump_format_through_the_graph_buckets():
    from pam import hrnet
    net = hrnet.HRNetPose(32, 17, None, resolution=RES, use_graph=True, max_dets=8, graph_bucket=4)
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
    dump2 = net.predict(pbl, batch_size=3)                           # batches of 3 + 1: other buckets, the same keypoints
    for a, b in zip(dump, dump2):
        for ia, ib in zip(a, b):
            assert ia['keypoints'] == ib['keypoints']


def test_w32_facade_from_its_config_into_the_tracker_vs_the_oracle():
    """ivclabpose built from the W32 config: PersonPoseDetect -> dump_results -> PersonTrack_Project3DPose, frame by frame, next to the
    CPU oracle's tracker fed the same dump: ids, view sets and 3D poses as the smoke test compares them."""
    from pam import synth
    from pam.ivclabpose import ivclabpose
    from oracle import cpu_ref as O
    seq = synth.make_sequence('S1', n_frames=8, seed=5, occlusion_every=5, birth_death_frame=4)
    cfg = dict(synth.MATCHER_CFG['Shelf']); conf = cfg.pop('CONF_THRESHOLD')
    model = ivclabpose({'NAME': ''}, _w32_pose_cfg(), dict(cfg, NAME='Iterative'), conf)
    assert model.pose_model.width == 32 and tuple(model.pose_model.resolution) == RES
    cams = model.GetCameraParameters(seq['calib'], 360, 288)
    ref = O.OracleIvclabpose(cfg, conf)
    ref.GetCameraParameters(seq['calib'], F=np.stack([c.F for c in cams]))
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (288, 360, 3), dtype=np.uint8) for _ in range(len(seq['frames'][0]))]
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
    assert n_det > 0
