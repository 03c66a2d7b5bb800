"""PoseResNet (Simple Baselines): the second model family of the pose backend (``HRNetPose(c, 17, ckpt, model_name='PoseResNet')``,
c = the ResNet depth 50 / 101 / 152).

A ResNet backbone (7x7 stride-2 stem, 3x3 stride-2 max-pool, four stages of Bottlenecks) and three 4x4 stride-2 transposed
convolutions (2048 / 256 / 256 -> 256 channels) up to a quarter of the input resolution, then a 1x1 head.  The module keeps the
upstream state-dict key layout (``conv1``, ``bn1``, ``layer1..4``, ``deconv_layers.{0,1,3,4,6,7}``, ``final_layer``), so a
``pose_resnet_{50,101,152}_*.pth`` file loads.  The HIP executor of the folded module is hrnet_hip.HipPoseResNet; the packers of its
two own kernels (csrc/pam_resnet.hip) live here with their CPU emulations."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as Fnn

from .hrnet_model import Bottleneck

DEPTHS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
MODEL_NAMES = ('PoseResNet', 'poseresnet', 'ResNet', 'resnet')
DECONV_CH = 256

# k_deconv4x4s2: output row oy = 2 iy - 1 + ky.  Output parity p (0: even, 1: odd) reads two taps t = 0, 1 of the input grid:
# (ky, input-row offset dy) for the output row 2 m + p is taken from input row m + dy.  Columns follow the same table.
DECONV_TAPS = (((1, 0), (3, -1)), ((2, 0), (0, 1)))


class PoseResNet(nn.Module):
    """Simple Baselines: ResNet-{50,101,152} -> 3 x (ConvTranspose2d 4x4 s2 + BN + ReLU) -> 1x1 head."""

    def __init__(self, resnet_size=50, nof_joints=17):
        super().__init__()
        if resnet_size not in DEPTHS:
            raise ValueError('PoseResNet: depth %r is not supported (Bottleneck ResNets 50 / 101 / 152 only)' % (resnet_size,))
        self.resnet_size = resnet_size
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        blocks = DEPTHS[resnet_size]
        self.layer1 = self._make_layer(64, blocks[0])
        self.layer2 = self._make_layer(128, blocks[1], 2)
        self.layer3 = self._make_layer(256, blocks[2], 2)
        self.layer4 = self._make_layer(512, blocks[3], 2)
        layers = []
        for _ in range(3):
            layers += [nn.ConvTranspose2d(self.inplanes, DECONV_CH, 4, 2, 1, 0, bias=False), nn.BatchNorm2d(DECONV_CH), nn.ReLU(inplace=True)]
            self.inplanes = DECONV_CH
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(DECONV_CH, nof_joints, 1)

    def _make_layer(self, planes, blocks, stride=1):
        down = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, down)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def stem(self, x):
        return self.maxpool(self.relu(self.bn1(self.conv1(x))))

    def features(self, x):
        x = self.stem(x)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.deconv_layers(x)

    def forward(self, x):
        return self.final_layer(self.features(x))


def init_random(model, seed=0):
    """Seeded He-normal convolutions (transposed ones too), BN as the identity, bn3 of every residual branch 0.3 (as hrnet_model.init_random)."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            cout = m.out_channels
            fan_out = cout * m.kernel_size[0] * m.kernel_size[1]
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    m.bias.zero_()
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
            m.running_mean.zero_(); m.running_var.fill_(1.0)
    for m in model.modules():
        if isinstance(m, Bottleneck):
            nn.init.constant_(m.bn3.weight, 0.3)
    return model


def fold_batchnorm(model):
    """Inference form: every (conv, BN) and (transposed conv, BN) pair becomes one layer with bias.  A Conv2d weight (Cout, Cin, kh, kw)
    is scaled along dim 0, a ConvTranspose2d weight (Cin, Cout, kh, kw) along dim 1."""
    def fold(conv, bn):
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        if isinstance(conv, nn.ConvTranspose2d):
            new = nn.ConvTranspose2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.output_padding, bias=True)
            scale = s.reshape(1, -1, 1, 1)
        else:
            new = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, bias=True)
            scale = s.reshape(-1, 1, 1, 1)
        new = new.to(conv.weight.dtype)
        with torch.no_grad():
            new.weight.copy_(conv.weight * scale)
            new.bias.copy_(bn.bias - bn.running_mean * s + (conv.bias * s if conv.bias is not None else 0))
        return new

    def walk(mod):
        names = list(mod._modules.keys())
        for a, b in zip(names, names[1:]):
            ma, mb = mod._modules[a], mod._modules[b]
            if isinstance(ma, (nn.Conv2d, nn.ConvTranspose2d)) and isinstance(mb, nn.BatchNorm2d):
                mod._modules[a] = fold(ma, mb)
                mod._modules[b] = nn.Identity()
        for m in mod._modules.values():
            if m is not None:
                walk(m)
    model = model.eval()
    walk(model)
    return model


_FOLDED_RANDOM = {}


def folded_random_model(depth, nof_joints=17, seed=0):
    """The seeded random-weight PoseResNet, BN folded: built once per (depth, joints, seed) and process, copied per call."""
    key = (int(depth), int(nof_joints), int(seed))
    if key not in _FOLDED_RANDOM:
        _FOLDED_RANDOM[key] = fold_batchnorm(init_random(PoseResNet(int(depth), nof_joints), seed))
    return copy.deepcopy(_FOLDED_RANDOM[key])


def checkpoint_state_dict(path_or_sd):
    """The state dict of a checkpoint: the file (or object) may be the state dict itself or {'model': sd}; a leading ``module.``
    (DataParallel) is dropped from every key."""
    sd = torch.load(path_or_sd, map_location='cpu') if isinstance(path_or_sd, str) else path_or_sd
    if isinstance(sd, dict) and 'model' in sd and isinstance(sd['model'], dict):
        sd = sd['model']
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}


def load_folded_checkpoint(path, depth, nof_joints=17):
    """A PoseResNet-{depth} checkpoint in the upstream key layout -> the folded fp32 module (CPU).  Files written before BatchNorm had
    ``num_batches_tracked`` load too; a file of another depth (missing or extra layers, other shapes) raises."""
    model = PoseResNet(int(depth), nof_joints)
    sd = checkpoint_state_dict(path)
    own = model.state_dict()
    missing = [k for k in own if k not in sd and not k.endswith('num_batches_tracked')]
    extra = [k for k in sd if k not in own]
    if missing or extra:
        raise RuntimeError('PoseResNet-%d checkpoint %s: %d keys missing (%s), %d unexpected (%s)' % (
            depth, path if isinstance(path, str) else '<object>', len(missing), missing[:3], len(extra), extra[:3]))
    for k, v in own.items():
        if k in sd and tuple(sd[k].shape) != tuple(v.shape):
            raise RuntimeError('PoseResNet-%d checkpoint: %s has shape %s, expected %s' % (depth, k, tuple(sd[k].shape), tuple(v.shape)))
    model.load_state_dict(sd, strict=False)
    return fold_batchnorm(model)


def count_flops(depth=50, resolution=(256, 192), nof_joints=17):
    """2 * MAC of one crop's backbone and deconvolutions, from shapes: the stem at its 3 real input channels, each transposed convolution
    at its 4 live taps per output pixel, the 1x1 head excluded."""
    model = PoseResNet(depth, nof_joints).to('meta')
    total = [0]

    def hook(m, inp, out):
        if m is model.final_layer:
            return
        if isinstance(m, nn.ConvTranspose2d):
            total[0] += 2 * out.numel() * m.in_channels * 4
        else:
            total[0] += 2 * out.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    with torch.no_grad():
        model(torch.empty(1, 3, resolution[0], resolution[1], device='meta'))
    for h in hs:
        h.remove()
    return total[0]


# -- k_resnet_stem: the MFMA A fragments of the 7x7 stride-2 convolution ---------------------------------------------------------------
def stem_fragments(conv):
    """[4 n-tiles j][7 ky][2 k-steps s][64 lanes][8] float32 (the caller casts): lane l holds, for output channel
    16 ((l & 15) >> 2) + 4 j + (l & 3), the 8 input channels of tap (ky, kx = 4 s + (l >> 4)); kx = 7 and input channels >= 3 are zero."""
    w = conv.weight.detach().float()
    cout, cin, kh, kw = w.shape
    assert cout == 64 and cin <= 8 and kh == 7 and kw == 7, tuple(w.shape)
    w8 = torch.zeros((64, 8, 7, 8), dtype=torch.float32)
    w8[:, :cin, :, :7] = w
    lanes = torch.arange(64)
    q, g = lanes & 15, lanes >> 4
    frag = torch.zeros((4, 7, 2, 64, 8), dtype=torch.float32)
    for j in range(4):
        ch = 16 * (q >> 2) + 4 * j + (q & 3)
        for s in range(2):
            kx = 4 * s + g
            frag[j, :, s] = w8[ch, :, :, kx].permute(2, 0, 1)          # [ky][lane][8 cin]
    return frag


# -- k_deconv4x4s2: the per-parity weight image --------------------------------------------------------------------------------------
def deconv_image_index(cin, cout):
    """Where each weight of a (Cin, Cout, 4, 4) transposed convolution goes in the image (flat element index), as a (Cin, Cout, 4, 4)
    int64 tensor.  Image order: [parity p = 2 py + px][cout slab s (64 channels)][k-step c (32 input channels)][tap t = 2 ty + tx]
    [n-tile j][lane l][8]; lane l holds output channel 64 s + 16 ((l & 15) >> 2) + 4 j + (l & 3) and input channels 32 c + 8 (l >> 4) .. + 7;
    tap (ty, tx) of parity (py, px) is (ky, kx) = (DECONV_TAPS[py][ty][0], DECONV_TAPS[px][tx][0]).  Every weight appears exactly 4 / 4 = once
    (each (ky, kx) belongs to one parity and one tap)."""
    assert cin % 32 == 0 and cout % 64 == 0
    idx = torch.empty((cin, cout, 4, 4), dtype=torch.int64)
    ci = torch.arange(cin)
    co = torch.arange(cout)
    c_step, g, e = ci // 32, (ci % 32) // 8, ci % 8
    s, r = co // 64, co % 64
    # r = 16 (q >> 2) + 4 j + (q & 3)  ->  q = 4 (r // 16) + (r & 3), j = (r % 16) // 4
    q = 4 * (r // 16) + (r & 3)
    j = (r % 16) // 4
    ncs = cin // 32
    nsl = cout // 64
    for py in range(2):
        for ty in range(2):
            ky = DECONV_TAPS[py][ty][0]
            for px in range(2):
                for tx in range(2):
                    kx = DECONV_TAPS[px][tx][0]
                    p, t = 2 * py + px, 2 * ty + tx
                    lane = q[None, :] + 16 * g[:, None]                         # [cin][cout]
                    base = ((((p * nsl + s[None, :]) * ncs + c_step[:, None]) * 4 + t) * 4 + j[None, :]) * 64
                    idx[:, :, ky, kx] = (base + lane) * 8 + e[:, None]
    return idx


def deconv_image(weight):
    """(Cin, Cout, 4, 4) -> the flat float32 image of ``deconv_image_index`` (the caller casts to bf16)."""
    cin, cout = weight.shape[:2]
    idx = deconv_image_index(cin, cout)
    img = torch.empty(cin * cout * 16, dtype=weight.dtype)
    img[idx.reshape(-1)] = weight.detach().reshape(-1)
    return img


def deconv_emulate(x, img, bias, cin, cout):
    """The four-parity GEMMs of k_deconv4x4s2 in the input's dtype (float64 in the tests), fed from the packed image:
    x (N, Cin, H, W) -> (N, Cout, 2H, 2W) + bias (no activation)."""
    n, _, h, w = x.shape
    nsl, ncs = cout // 64, cin // 32
    im = img.reshape(4, nsl, ncs, 4, 4, 64, 8)                              # [p][s][c][t][j][lane][8]
    lanes = torch.arange(64)
    q, g = lanes & 15, lanes >> 4
    xp = Fnn.pad(x, (1, 1, 1, 1))
    out = torch.zeros((n, cout, 2 * h, 2 * w), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            p = 2 * py + px
            acc = torch.zeros((n, cout, h, w), dtype=x.dtype)
            for ty in range(2):
                for tx in range(2):
                    dy, dx = DECONV_TAPS[py][ty][1], DECONV_TAPS[px][tx][1]
                    src = xp[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]           # input pixel (m + dy, n + dx)
                    # rebuild the (cout, cin) matrix of this tap from the image's fragments
                    wm = torch.zeros((cout, cin), dtype=x.dtype)
                    for s in range(nsl):
                        for j in range(4):
                            co = 64 * s + 16 * (q >> 2) + 4 * j + (q & 3)          # [lane]
                            for c in range(ncs):
                                ci = 32 * c + 8 * g[:, None] + torch.arange(8)[None, :]     # [lane][8]
                                wm[co[:, None].expand(64, 8), ci] = im[p, s, c, 2 * ty + tx, j].to(x.dtype)
                    acc += torch.einsum('oc,nchw->nohw', wm, src)
            out[:, :, py::2, px::2] = acc
    return out + bias.to(x.dtype).reshape(1, -1, 1, 1)
