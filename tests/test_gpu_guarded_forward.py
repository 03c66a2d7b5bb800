"""GPU: every launch the executors issue, at the networks' real shapes and tile plans, into sentinel-filled, banded memory
(tests/guarded_mem.py) -- the launches outside exact_ref.CASES included: k_upsample_add, k_upsample_concat, k_maxpool, k_spp, the lazy
transitions, the merged strided heads.

Per executor (built once per module, random weights), named configuration, crop / view count and -- HRNet -- multi_stream setting:
  (a) an eager forward with ``arena = None`` on a seeded bf16 input;
  (b) the same forward with ``arena = GuardArena`` and the input between poison bands, once per fill of guarded_mem.FILLS;
  (c) after a device synchronise: the outputs of (b) are bitwise those of (a), no band is damaged, no payload element is unwritten.
There is no tolerance here and no reference: (a) is compared with itself under other memory.  ``PARTIAL`` lists the allocations that
are legitimately written in part; it is empty.

Then the product's own arena (HRNetPose, captured replays): a replay's result must not depend on what the arena held before it --
NaN, +-1.7e38 or zeros -- nor on a smaller crop-count bucket having replayed into the same buffer in between."""
import pytest
import torch

import conv_plan_cases as P
import guarded_mem as G

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# (executor, shape, position in the forward) -> why it is written only in part.  Nothing is: every launcher writes all of every output.
PARTIAL = {}


class Nets(object):
    """The executors of this file, built on first use and kept for the module; one GuardArena, regrown when a case needs a larger one."""

    def __init__(self):
        self.made, self.arena = {}, None
        self.make = {name: (make, h, w, True) for name, make, h, w in P._pose_nets(DEV)}
        self.make.update({name: (make, h, w, False) for name, make, h, w in P._detectors(DEV)})

    def get(self, name):
        if name not in self.made:
            self.made[name] = self.make[name][0]()
        return (self.made[name],) + self.make[name][1:]

    def arena_of(self, nbytes):
        if self.arena is None or self.arena.half_bytes < nbytes:
            self.arena = None
            torch.cuda.empty_cache()
            self.arena = G.GuardArena(DEV, nbytes)
        self.arena.reset()
        return self.arena


@pytest.fixture(scope='module')
def nets():
    n = Nets()
    yield n
    n.made.clear(); n.arena = None
    torch.cuda.empty_cache()


def forward(hip, is_pose, x):
    with torch.no_grad():
        out = hip.features(x) if is_pose else hip.forward(x)
    return [out] if is_pose else list(out)


def capacity(hip, is_pose, n, h, w):
    """Bytes of a GuardArena for one n-item forward: a shape-only walk with a measuring arena, summed over all allocations plus bands."""
    probe = G.MeasuringArena()
    saved = (hip.multi_stream, hip.arena, hip.count, hip.prof)
    hip.multi_stream, hip.arena, hip.count, hip.prof = False, probe, None, None
    try:
        x = torch.empty((n, 8, h, w), dtype=torch.bfloat16, device='meta').contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            hip._features(x) if is_pose else hip.forward(x)
    finally:
        hip.multi_stream, hip.arena, hip.count, hip.prof = saved
    assert probe.n > 10
    return probe.capacity()


def guarded_forward(nets, name, config, n, multi_stream):
    hip, h, w, is_pose = nets.get(name)
    if config is not None:
        hip.apply_config(config)
    ms0, hip.multi_stream = hip.multi_stream, multi_stream
    try:
        x = P.x8(n, h, w, DEV, seed=100 + n)
        hip.arena = None
        want = [t.clone() for t in forward(hip, is_pose, x)]                         # (a)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t.float()).all()) for t in want)
        ar = nets.arena_of(capacity(hip, is_pose, n, h, w))
        xp, hd = G.poisoned(x, G.FILLS[0])
        bad = []
        for fill in G.FILLS:
            hd.refill(fill)
            ar.reset()
            hip.arena = ar
            got = forward(hip, is_pose, xp)                                          # (b)
            torch.cuda.synchronize()
            hip.arena = None
            tag = '%s %s n=%d multi_stream=%s fill %#06x' % (name, config, n, multi_stream, fill)
            lo, hi = ar.buf.data_ptr(), ar.buf.data_ptr() + 2 * ar.buf.numel()
            assert len(ar.allocs) > 10 and all(lo <= t.data_ptr() < hi for t in got), tag
            for i, (g, wnt) in enumerate(zip(got, want)):                            # (c)
                if not torch.equal(g.view(torch.int16), wnt.view(torch.int16)):
                    d = g.view(torch.int16) != wnt.view(torch.int16)
                    bad.append('%s: output %d differs from the unguarded forward in %d of %d elements (%d hold the sentinel)' % (
                        tag, i, int(d.sum()), d.numel(), int((d & (g.view(torch.int16) == G.as_i16(G.SENTINEL))).sum())))
            for v in ar.violations():
                bad.append('%s: band %s allocation %d %s: %d elements, %d .. %d bytes from the payload' % (
                    tag, v['side'], v['order'], v['shape'], v['changed'], v['first'], v['last']))
            for a, k in zip(ar.allocs, ar.unwritten()):
                if k and (name, a['shape'], a['order']) not in PARTIAL:
                    bad.append('%s: allocation %d %s: %d of %d elements never written' % (tag, a['order'], a['shape'], k, a['nbytes'] // 2))
            if len(bad) > 20:
                break
        assert not bad, '\n'.join(bad[:40])
    finally:
        hip.arena, hip._keep, hip.multi_stream = None, None, ms0


def _pose_cases():
    from pam import hrnet_hip
    for name, cls in (('hrnet_w48', hrnet_hip.HipHRNet), ('hrnet_w32', hrnet_hip.HipHRNetW32), ('poseresnet50', hrnet_hip.HipPoseResNet)):
        for config in cls.CONFIGS:
            for n in (1, 3):                                 # one crop, and an odd count: where items cross a crop boundary
                for ms in ((True, False) if name != 'poseresnet50' else (False,)):
                    yield pytest.param(name, config, n, ms, id='%s-%s-n%d-%s' % (name, config, n, 'streams' if ms else 'serial'))


@pytest.mark.parametrize('name,config,n,multi_stream', list(_pose_cases()))
def test_pose_forward_in_guarded_memory(nets, name, config, n, multi_stream):
    guarded_forward(nets, name, config, n, multi_stream)


@pytest.mark.parametrize('views', [1, 2])
@pytest.mark.parametrize('name', ['darknet53', 'yolov3_tiny', 'yolov3_spp'])
def test_detector_forward_in_guarded_memory(nets, name, views):
    guarded_forward(nets, name, None, views, False)


# ---- the product's arena: a replay does not depend on what the buffer held ----------------------------------------------------------------------
def _fill_arenas(net, bits):
    torch.cuda.synchronize()
    for ar in net._arenas.values():
        ar.buf.view(torch.int16).fill_(G.as_i16(bits))
    torch.cuda.synchronize()


@pytest.mark.parametrize('c,model_name,res', [(48, 'HRNet', (384, 288)), (32, 'HRNet', (256, 192)), (50, 'PoseResNet', (256, 192))],
                         ids=['hrnet_w48', 'hrnet_w32', 'poseresnet50'])
def test_replay_is_independent_of_the_arena_contents(c, model_name, res):
    from pam import hrnet
    net = hrnet.HRNetPose(c, 17, None, model_name=model_name, resolution=res, use_graph=True, max_crops=3)
    x3 = P.x8(3, res[0], res[1], DEV, seed=3)
    a = net.heatmaps(x3).clone()                             # captures, then replays
    torch.cuda.synchronize()
    assert (3, 'heatmaps', 0) in net._graphs and list(net._arenas) == [0] and bool(torch.isfinite(a).all())
    for bits in G.FILLS + (0x0000,):
        _fill_arenas(net, bits)
        b = net.heatmaps(x3)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(b).all()), 'fill %#06x' % bits
        assert torch.equal(b.view(torch.int32), a.view(torch.int32)), 'fill %#06x: %d of %d heat-map values differ' % (
            bits, int((b.view(torch.int32) != a.view(torch.int32)).sum()), a.numel())
    # a smaller bucket captured into the same slot shares the buffer: large, small, large -- each bitwise its own first result
    arena = net._arenas[0]
    x1 = P.x8(1, res[0], res[1], DEV, seed=1)
    s = net.heatmaps(x1).clone()
    torch.cuda.synchronize()
    assert (1, 'heatmaps', 0) in net._graphs and net._arenas[0] is arena
    for x, first, what in ((x3, a, 'the 3-crop replay after the 1-crop capture'), (x1, s, 'the 1-crop replay'), (x3, a, 'the 3-crop replay again')):
        y = net.heatmaps(x)
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), first.view(torch.int32)) and bool(torch.isfinite(y).all()), what
    assert not net.check_void()
