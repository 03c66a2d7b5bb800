"""HRNet-W48 / -W32 as PyTorch sees it: the public architecture in the official state-dict key layout (so that
``pose_hrnet_w48_384x288.pth`` and ``pose_hrnet_w32_256x192.pth`` load), BatchNorm folding, the seeded random initialisation, checkpoint
loading and the FLOP / byte counters.  The module is the weight container the HIP executor packs (hrnet_hip.py) and the fp32 checker the
tests and the drift measurement run; no forward of the product goes through it."""
import torch
import torch.nn as nn
import torch.nn.functional as Fnn

BN_EPS = 1e-5


def conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 3, stride, 1, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        y = Fnn.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return Fnn.relu(y + r)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        r = x if self.downsample is None else self.downsample(x)
        y = Fnn.relu(self.bn1(self.conv1(x)))
        y = Fnn.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return Fnn.relu(y + r)


class HighResolutionModule(nn.Module):
    def __init__(self, channels, num_blocks=4, multi_scale_output=True):
        super().__init__()
        nb = len(channels)
        self.branches = nn.ModuleList(
            [nn.Sequential(*[BasicBlock(c, c) for _ in range(num_blocks)]) for c in channels])
        fuse = []
        for i in range(nb if multi_scale_output else 1):
            row = []
            for j in range(nb):
                if j > i:
                    row.append(nn.Sequential(nn.Conv2d(channels[j], channels[i], 1, bias=False),
                                             nn.BatchNorm2d(channels[i]),
                                             nn.Upsample(scale_factor=2 ** (j - i), mode='nearest')))
                elif j == i:
                    row.append(None)
                else:
                    steps = []
                    for k in range(i - j):
                        if k == i - j - 1:
                            steps.append(nn.Sequential(conv3x3(channels[j], channels[i], 2), nn.BatchNorm2d(channels[i])))
                        else:
                            steps.append(nn.Sequential(conv3x3(channels[j], channels[j], 2), nn.BatchNorm2d(channels[j]),
                                                       nn.ReLU(inplace=False)))
                    row.append(nn.Sequential(*steps))
            fuse.append(nn.ModuleList(row))
        self.fuse_layers = nn.ModuleList(fuse)

    def forward(self, xs):
        xs = [b(x) for b, x in zip(self.branches, xs)]
        out = []
        for i, row in enumerate(self.fuse_layers):
            y = None
            for j, f in enumerate(row):
                t = xs[j] if f is None else f(xs[j])
                y = t if y is None else y + t
            out.append(Fnn.relu(y))
        return out


class PoseHighResolutionNet(nn.Module):
    """HRNet-W{c}: stem -> layer1 -> 3 multi-resolution stages -> 1x1 head (Appendix D of SURVEY.md)."""

    def __init__(self, c=48, num_joints=17):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.conv2 = nn.Conv2d(64, 64, 3, 2, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(64)
        down = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False), nn.BatchNorm2d(256))
        self.layer1 = nn.Sequential(Bottleneck(64, 64, downsample=down), Bottleneck(256, 64), Bottleneck(256, 64),
                                    Bottleneck(256, 64))
        ch = [c, 2 * c, 4 * c, 8 * c]
        self.transition1 = nn.ModuleList([
            nn.Sequential(conv3x3(256, ch[0]), nn.BatchNorm2d(ch[0]), nn.ReLU(inplace=False)),
            nn.Sequential(nn.Sequential(conv3x3(256, ch[1], 2), nn.BatchNorm2d(ch[1]), nn.ReLU(inplace=False)))])
        self.stage2 = nn.Sequential(HighResolutionModule(ch[:2]))
        self.transition2 = nn.ModuleList([None, None, nn.Sequential(
            nn.Sequential(conv3x3(ch[1], ch[2], 2), nn.BatchNorm2d(ch[2]), nn.ReLU(inplace=False)))])
        self.stage3 = nn.Sequential(*[HighResolutionModule(ch[:3]) for _ in range(4)])
        self.transition3 = nn.ModuleList([None, None, None, nn.Sequential(
            nn.Sequential(conv3x3(ch[2], ch[3], 2), nn.BatchNorm2d(ch[3]), nn.ReLU(inplace=False)))])
        self.stage4 = nn.Sequential(HighResolutionModule(ch), HighResolutionModule(ch),
                                    HighResolutionModule(ch, multi_scale_output=False))
        self.final_layer = nn.Conv2d(ch[0], num_joints, 1)

    def features(self, x):
        x = Fnn.relu(self.bn1(self.conv1(x)))
        x = Fnn.relu(self.bn2(self.conv2(x)))
        x = self.layer1(x)
        xs = [self.transition1[0](x), self.transition1[1](x)]
        xs = self.stage2[0](xs)
        xs = xs + [self.transition2[2](xs[-1])]
        for m in self.stage3:
            xs = m(xs)
        xs = xs + [self.transition3[3](xs[-1])]
        for m in self.stage4:
            xs = m(xs)
        return xs[0]

    def forward(self, x):
        return self.final_layer(self.features(x))


def init_random(model, seed=0):
    """Seeded He-normal convs, BN gamma=1 beta=0 mean=0 var=1 (real weights are unavailable offline)."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    m.bias.zero_()
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
            m.running_mean.zero_(); m.running_var.fill_(1.0)
    for m in model.modules():          # damp the residual branches so activations stay O(1) through ~80 blocks
        if isinstance(m, BasicBlock):
            nn.init.constant_(m.bn2.weight, 0.3)
        elif isinstance(m, Bottleneck):
            nn.init.constant_(m.bn3.weight, 0.3)
    return model


def count_flops(c=48, num_joints=17, h=384, w=288):
    """2*MAC of every conv for one crop, counted from the module table by a shape-only forward on the meta device."""
    model = PoseHighResolutionNet(c, num_joints).to('meta')
    total = [0]

    def hook(m, inp, out):
        total[0] += 2 * out.shape[1] * out.shape[2] * out.shape[3] * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        model(torch.empty(1, 3, h, w, device='meta'))
    for x in hs:
        x.remove()
    return total[0]


def algorithmic_work(n_crops, resolution=(384, 288), config=None):
    """Algorithmic work of one conv-stack forward (shape-only walks on the meta device):
    ``bytes``: EXECUTOR-INDEPENDENT unique HBM bytes of the module graph -- every BasicBlock / Bottleneck counted as input + its weights and
    biases + output (block interiors are not traffic the algorithm needs: a fused launch keeps them on chip), every other convolution as
    input + weights + bias + output, every fuse-layer sum as base + terms + output.  Un-fusing a block cannot raise this number.
    ``flops``; ``launches`` and ``bytes_as_executed`` (per launch: in + weights + bias [+ residual] + out) of the given executor
    configuration (HipHRNet.CONFIGS; None = the default)."""
    from .hrnet_hip import HipHRNet, TileCfg

    from . import _lib as _real

    class _MetaLib(object):
        def __getattr__(self, name):
            if name in ('pam_conv3x3_slab', 'pam_conv3x3_layout', 'pam_conv3x3_layout_ex'):       # pure host-side shape queries: the executor's plan depends on them
                return getattr(_real.load(), name)
            return lambda *a, **k: 0
    eng = HipHRNet.__new__(HipHRNet)
    eng.lib = _MetaLib(); eng.device = torch.device('meta'); eng.tile_cfg = TileCfg.AUTO; eng.multi_stream = False
    model = fold_batchnorm(PoseHighResolutionNet())
    model.final_layer = nn.Identity()
    HipHRNet._pack(eng, model, torch.device('meta'))
    eng.apply_config(config or HipHRNet.config_name)
    eng.count = dict(bytes=0, flops=0, launches=0)
    x = torch.empty((n_crops, 8, resolution[0], resolution[1]), dtype=torch.bfloat16, device='meta').contiguous(memory_format=torch.channels_last)
    eng._features(x)
    # the module graph itself: hooks on the blocks (whole), on the convolutions outside blocks, and the fuse sums from the module's shapes
    total = [0]
    inside = set()
    for m in model.modules():
        if isinstance(m, (BasicBlock, Bottleneck)):
            inside.update(id(c) for c in m.modules() if c is not m)
    pbytes = lambda m: sum(2 * p.numel() if p.dim() > 1 else 4 * p.numel() for p in m.parameters())

    def hook(m, inp, out):
        total[0] += 2 * (inp[0].numel() + out.numel()) + pbytes(m)
    hs = [m.register_forward_hook(hook) for m in model.modules()
          if isinstance(m, (BasicBlock, Bottleneck)) or (isinstance(m, nn.Conv2d) and id(m) not in inside)]

    def sum_hook(m, inp, out):                            # HighResolutionModule: out_i = relu(x_i + terms): base + each term at ITS resolution + out
        for i, o in enumerate(out):
            total[0] += 2 * 2 * o.numel()
            for j in range(len(out)):
                if j > i:                                 # 1x1 up-convolution's output, read through the nearest-neighbour upsample
                    total[0] += 2 * o.numel() // (4 ** (j - i))
                elif j < i:
                    total[0] += 2 * o.numel()
    hs += [m.register_forward_hook(sum_hook) for m in model.modules() if isinstance(m, HighResolutionModule)]
    with torch.no_grad():
        model.to('meta')(torch.empty((n_crops, 3, resolution[0], resolution[1]), device='meta'))
    for h in hs:
        h.remove()
    return dict(bytes=total[0], flops=eng.count['flops'], launches=eng.count['launches'], bytes_as_executed=eng.count['bytes'])


def fold_batchnorm(model):
    """Inference form: every (conv, BN) pair becomes one conv with bias (scale = gamma / sqrt(var + eps))."""
    def fold(conv, bn):
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        new = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, bias=True)
        with torch.no_grad():
            new.weight.copy_(conv.weight * s.reshape(-1, 1, 1, 1))
            new.bias.copy_(bn.bias - bn.running_mean * s + (conv.bias * s if conv.bias is not None else 0))
        return new

    def walk(mod):
        names = list(mod._modules.keys())
        for a, b in zip(names, names[1:]):
            ma, mb = mod._modules[a], mod._modules[b]
            if isinstance(ma, nn.Conv2d) and isinstance(mb, nn.BatchNorm2d):
                mod._modules[a] = fold(ma, mb)
                mod._modules[b] = nn.Identity()
        for m in mod._modules.values():
            if m is not None:
                walk(m)
    model = model.eval()
    walk(model)
    return model


_FOLDED_RANDOM = {}


def _folded_random_model(c, nof_joints, seed):
    """The seeded random-weight network, BN folded: built once per (c, joints, seed) and process (2.7 s of CPU work), copied per object --
    a test session or a bench run constructs dozens of networks over the same weights."""
    import copy
    key = (int(c), int(nof_joints), int(seed))
    if key not in _FOLDED_RANDOM:
        _FOLDED_RANDOM[key] = fold_batchnorm(init_random(PoseHighResolutionNet(c, nof_joints), seed))
    return copy.deepcopy(_FOLDED_RANDOM[key])


def load_folded_checkpoint(path, c, nof_joints):
    """A checkpoint file in the official key layout (the state dict itself or wrapped as {'model': ...}) -> the folded fp32 module
    HRNetPose packs (CPU)."""
    model = PoseHighResolutionNet(c, nof_joints)
    sd = torch.load(path, map_location='cpu')
    model.load_state_dict(sd.get('model', sd) if isinstance(sd, dict) else sd)
    return fold_batchnorm(model)
