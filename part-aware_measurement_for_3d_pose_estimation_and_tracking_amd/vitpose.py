"""ViTPose-B / -L, "classic decoder" (256 x 192): the third model family of the pose backend
(``HRNetPose(c, 17, ckpt, model_name='ViTPose', resolution=(256, 192))``, c = 'B' / 'L' or the width 768 / 1024).

A plain vision transformer -- 16 x 16 patches (stride 16, padding 2) of the 256 x 192 crop = 16 x 12 = 192 tokens, a learned position
table, ``depth`` pre-norm blocks (multi-head attention with head dimension 64 over all 192 tokens, then an MLP of ratio 4 with exact
GELU), a last LayerNorm -- and the Simple-Baselines head on the tokens read as a (D, 16, 12) map: two 4x4 stride-2 transposed
convolutions (-> 256 channels) with BN + ReLU, then a 1x1 convolution to the joints' 64 x 48 maps.  The module keeps the published
state-dict key layout (``backbone.patch_embed.proj``, ``backbone.pos_embed``, ``backbone.blocks.{i}.norm1|attn.qkv|attn.proj|norm2|
mlp.fc1|mlp.fc2``, ``backbone.last_norm``, ``keypoint_head.deconv_layers.{0,1,3,4}``, ``keypoint_head.final_layer``).  It is the fp32
weight container and test reference; the HIP executor of the folded module is hrnet_hip.HipViTPose (kernels: csrc/pam_vit.hip).
-S (head dimension 32), -H (head dimension 80), ViTPose+ and 384 x 288 are not supported."""
import copy

import torch
import torch.nn as nn

from . import poseresnet

MODEL_NAMES = ('ViTPose', 'vitpose')
VARIANTS = {'B': dict(dim=768, depth=12, heads=12), 'L': dict(dim=1024, depth=24, heads=16)}
RESOLUTION = (256, 192)
HEAD_DIM = 64
PATCH, PATCH_PAD = 16, 2
LN_EPS = 1e-6
DECONV_CH = 256
SUPPORTED = "ViTPose-B (c = 'B' or 768) and ViTPose-L (c = 'L' or 1024) at resolution (256, 192)"


def variant_of(c):
    """'B' / 'L' / 768 / 1024 -> 'B' | 'L'; anything else (the -S and -H variants by name or width included) raises ValueError."""
    if isinstance(c, str) and c.upper() in VARIANTS:
        return c.upper()
    if not isinstance(c, (str, bool)) and c is not None:
        for name, v in VARIANTS.items():
            if c == v['dim']:
                return name
    raise ValueError('ViTPose: variant c=%r is not supported (%s only; -S and -H have head dimensions 32 and 80)' % (c, SUPPORTED))


def check_resolution(resolution):
    if tuple(resolution) != RESOLUTION:
        raise ValueError('ViTPose: resolution %r is not supported (%s)' % (tuple(resolution), SUPPORTED))


class Attention(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        assert dim == heads * HEAD_DIM, (dim, heads)
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        b, t, d = x.shape
        q, k, v = self.qkv(x).reshape(b, t, 3, self.heads, HEAD_DIM).permute(2, 0, 3, 1, 4)      # each (B, heads, T, 64)
        p = torch.softmax((q @ k.transpose(-2, -1)) * HEAD_DIM ** -0.5, dim=-1)
        return self.proj((p @ v).transpose(1, 2).reshape(b, t, d))


class Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = Mlp(dim)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, PATCH, PATCH, PATCH_PAD)


class Backbone(nn.Module):
    def __init__(self, dim, depth, heads, tokens):
        super().__init__()
        self.patch_embed = PatchEmbed(dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, tokens + 1, dim))
        self.blocks = nn.ModuleList([Block(dim, heads) for _ in range(depth)])
        self.last_norm = nn.LayerNorm(dim, eps=LN_EPS)

    def embed(self, x):
        """(N, 3, H, W) -> (N, T, D): patches + the position table (row 0, the class token's, is added to every token)"""
        y = self.patch_embed.proj(x).flatten(2).transpose(1, 2)
        return y + self.pos_embed[:, 1:] + self.pos_embed[:, :1]

    def forward(self, x):
        x = self.embed(x)
        for b in self.blocks:
            x = b(x)
        return self.last_norm(x)


class KeypointHead(nn.Module):
    def __init__(self, dim, nof_joints):
        super().__init__()
        layers, cin = [], dim
        for _ in range(2):
            layers += [nn.ConvTranspose2d(cin, DECONV_CH, 4, 2, 1, 0, bias=False), nn.BatchNorm2d(DECONV_CH), nn.ReLU(inplace=True)]
            cin = DECONV_CH
        self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(DECONV_CH, nof_joints, 1)


class ViTPose(nn.Module):
    """variant: 'B' / 'L' (or 768 / 1024), or a dict(dim=, depth=, heads=) with dim == 64 heads (tests build small ones)."""

    def __init__(self, variant='B', nof_joints=17, resolution=RESOLUTION):
        super().__init__()
        cfg = dict(variant) if isinstance(variant, dict) else VARIANTS[variant_of(variant)]
        self.variant = variant if isinstance(variant, dict) else variant_of(variant)
        self.dim, self.depth, self.heads = cfg['dim'], cfg['depth'], cfg['heads']
        self.grid = (resolution[0] // PATCH, resolution[1] // PATCH)
        self.backbone = Backbone(self.dim, self.depth, self.heads, self.grid[0] * self.grid[1])
        self.keypoint_head = KeypointHead(self.dim, nof_joints)

    def token_map(self, tokens):
        """(N, T, D) -> (N, D, 16, 12)"""
        n, t, d = tokens.shape
        return tokens.transpose(1, 2).reshape(n, d, self.grid[0], self.grid[1])

    def features(self, x):
        return self.keypoint_head.deconv_layers(self.token_map(self.backbone(x)))

    def forward(self, x):
        return self.keypoint_head.final_layer(self.features(x))


def init_random(model, seed=0):
    """Seeded weights: truncated-normal-like (std 0.02) linears and position table as the published initialisation, LayerNorm and BN as
    the identity, He-normal (transposed) convolutions, zero biases."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * 0.02)
                m.bias.zero_()
            elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
                m.running_mean.zero_(); m.running_var.fill_(1.0)
        model.backbone.pos_embed.copy_(torch.randn(model.backbone.pos_embed.shape, generator=g) * 0.02)
    return model


def fold_batchnorm(model):
    """Inference form: the two (transposed convolution, BN) pairs of the head become transposed convolutions with bias."""
    return poseresnet.fold_batchnorm(model)


_FOLDED_RANDOM = {}


def folded_random_model(variant, nof_joints=17, seed=0):
    """The seeded random-weight ViTPose, BN folded: built once per (variant, joints, seed) and process, copied per call."""
    key = (variant_of(variant), int(nof_joints), int(seed))
    if key not in _FOLDED_RANDOM:
        _FOLDED_RANDOM[key] = fold_batchnorm(init_random(ViTPose(key[0], nof_joints), seed))
    return copy.deepcopy(_FOLDED_RANDOM[key])


def checkpoint_state_dict(path_or_sd):
    """The state dict of a checkpoint: under ``state_dict`` or at top level; a leading ``module.`` is dropped from every key and a class
    token (``backbone.cls_token``: the classic decoder never reads it) is ignored."""
    sd = torch.load(path_or_sd, map_location='cpu') if isinstance(path_or_sd, str) else path_or_sd
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    return {k: v for k, v in sd.items() if k != 'backbone.cls_token'}


def load_folded_checkpoint(path, variant, nof_joints=17):
    """A ViTPose-{B,L} checkpoint in the published key layout -> the folded fp32 module (CPU).  Missing and unexpected keys are named in
    the error; so is a tensor of another shape (a file of another variant)."""
    name = variant_of(variant)
    model = ViTPose(name, nof_joints)
    sd = checkpoint_state_dict(path)
    own = model.state_dict()
    missing = [k for k in own if k not in sd and not k.endswith('num_batches_tracked')]
    extra = [k for k in sd if k not in own]
    if missing or extra:
        raise RuntimeError('ViTPose-%s checkpoint %s: %d keys missing (%s), %d unexpected (%s)' % (
            name, path if isinstance(path, str) else '<object>', len(missing), ', '.join(missing[:8]), len(extra), ', '.join(extra[:8])))
    for k, v in own.items():
        if k in sd and tuple(sd[k].shape) != tuple(v.shape):
            raise RuntimeError('ViTPose-%s checkpoint: %s has shape %s, expected %s' % (name, k, tuple(sd[k].shape), tuple(v.shape)))
    model.load_state_dict(sd, strict=False)
    return fold_batchnorm(model)


def count_flops(variant='B', resolution=RESOLUTION, nof_joints=17):
    """2 * MAC of one crop's backbone and deconvolutions, from shapes: the patch embedding at its 3 real input channels, every linear
    layer, the two attention products of every block (Q K^T and P V), each transposed convolution at its 4 live taps per output pixel;
    the 1x1 head, LayerNorm, softmax and GELU excluded."""
    model = ViTPose(variant, nof_joints, resolution).to('meta')
    total = [0]

    def hook(m, inp, out):
        if m is model.keypoint_head.final_layer:
            return
        if isinstance(m, nn.ConvTranspose2d):
            total[0] += 2 * out.numel() * m.in_channels * 4
        elif isinstance(m, nn.Conv2d):
            total[0] += 2 * out.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]
        elif isinstance(m, nn.Linear):
            total[0] += 2 * out.numel() * m.in_features
        elif isinstance(m, Attention):
            b, t, d = inp[0].shape
            total[0] += 2 * 2 * b * t * t * d
    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Linear, Attention))]
    with torch.no_grad():
        model(torch.empty(1, 3, resolution[0], resolution[1], device='meta'))
    for h in hs:
        h.remove()
    return total[0]


def patch_matrix(conv):
    """The patch embedding's (D, 3, 16, 16) weight as the (D, 2048) matrix the patch kernel multiplies: K = (ky, kx, 8 channels), channels
    3 .. 7 zero (the crop kernel writes 8-channel pixels)."""
    w = conv.weight.detach().float()
    d = w.shape[0]
    assert tuple(w.shape[1:]) == (3, PATCH, PATCH), tuple(w.shape)
    w8 = torch.zeros((d, PATCH, PATCH, 8), dtype=torch.float32)
    w8[..., :3] = w.permute(0, 2, 3, 1)
    return w8.reshape(d, PATCH * PATCH * 8)


def position_bias(backbone):
    """(T, D) float32: pos[t + 1] + pos[0] + the patch convolution's bias -- what the patch kernel adds to token t."""
    pos = backbone.pos_embed.detach().float()[0]
    return (pos[1:] + pos[:1] + backbone.patch_embed.proj.bias.detach().float()[None, :]).contiguous()
