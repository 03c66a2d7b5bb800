"""The calibrated ViTPose test network (test infrastructure: nothing under the package imports this), built in the manner of
hrnet_calibrated.py: a seeded network in which nothing is the identity -- LayerNorm gamma ~ U[0.5, 1.5] and beta ~ N(0, 0.3), linear and
patch biases ~ N(0, 0.1), the seeded position table, the head's BN with drawn gamma / beta and running statistics calibrated on one
seeded 256 x 192 batch, a non-zero head bias.  The outputs of the residual branches (attn.proj, mlp.fc2: weights and biases) are damped
by hrnet_calibrated.RESIDUAL_DAMP, as the last BN of every residual branch is there.

``emulate`` is the bf16_storage emulation of the executor: fp32 arithmetic, bf16 weights, and a bf16 rounding wherever
hrnet_hip.HipViTPose stores -- the patch embedding, every LayerNorm, qkv, the attention output, both residual sums, the GELU output, the
deconvolutions -- and on P, the exponentials that enter the P V product."""
import copy

import torch
import torch.nn as nn

from pam import vitpose
from hrnet_calibrated import SEED, CALIB_SHAPE, GAMMA, RESIDUAL_DAMP, BETA_STD

_CACHE = {}
BIAS_STD = 0.1


def _build(variant, seed):
    g = torch.Generator().manual_seed(seed)
    model = vitpose.init_random(vitpose.ViTPose(variant, 17), seed=seed)
    damped = set()
    for b in model.backbone.blocks:
        damped |= {id(b.attn.proj), id(b.mlp.fc2)}
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (nn.LayerNorm, nn.BatchNorm2d)):
                n = m.weight.numel()
                m.weight.copy_(GAMMA[0] + (GAMMA[1] - GAMMA[0]) * torch.rand(n, generator=g))
                m.bias.copy_(BETA_STD * torch.randn(n, generator=g))
            if isinstance(m, nn.BatchNorm2d):
                m.momentum = None
                m.reset_running_stats()
            if isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(BIAS_STD * torch.randn(m.bias.shape, generator=g))
            if id(m) in damped:
                m.weight.mul_(RESIDUAL_DAMP); m.bias.mul_(RESIDUAL_DAMP)
        x = torch.randn(CALIB_SHAPE, generator=torch.Generator().manual_seed(seed + 1))
        model.train()
        model(x)
    model.eval()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.momentum = 0.1
    state = {k: v.clone() for k, v in model.state_dict().items()}
    folded = vitpose.fold_batchnorm(copy.deepcopy(model)).eval()
    for p in folded.parameters():
        p.requires_grad_(False)
    return state, folded


def calibrated(variant='B', seed=SEED):
    """-> (state_dict in the published key layout, folded fp32 module); the same objects for every call of a process (do not modify)."""
    if (variant, seed) not in _CACHE:
        _CACHE[(variant, seed)] = _build(variant, seed)
    return _CACHE[(variant, seed)]


def folded_copy(variant='B', seed=SEED):
    return copy.deepcopy(calibrated(variant, seed)[1])


def bf16_weights(model):
    """Every linear / conv / transposed conv weight rounded to bf16 as the packing rounds it; biases, LayerNorm parameters and the
    position table stay fp32 (the executor keeps them in float32)."""
    m = copy.deepcopy(model)
    with torch.no_grad():
        for c in m.modules():
            if isinstance(c, (nn.Linear, nn.Conv2d, nn.ConvTranspose2d)):
                c.weight.copy_(c.weight.to(torch.bfloat16).float())
    return m


def _rnd(t):
    return t.to(torch.bfloat16).float()


def _same(t):
    return t


def block_forward(b, x, r=_same):
    """One pre-norm block in fp32 with r applied wherever the executor stores (r = identity: the plain fp32 block)."""
    n, t, d = x.shape
    qkv = r(b.attn.qkv(r(b.norm1(x)))).reshape(n, t, 3, b.attn.heads, vitpose.HEAD_DIM).permute(2, 0, 3, 1, 4)
    s = (qkv[0] @ qkv[1].transpose(-2, -1)) * 0.125
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (r(e) @ qkv[2]) / e.sum(-1, keepdim=True)                   # P rounded for the product, divided by the sum of the unrounded
    x = r(x + b.attn.proj(r(o.transpose(1, 2).reshape(n, t, d))))
    return r(x + b.mlp.fc2(r(b.mlp.act(b.mlp.fc1(r(b.norm2(x)))))))


def deconv_forward(model, k, x):
    dl = model.keypoint_head.deconv_layers
    return dl[3 * k + 2](dl[3 * k + 1](dl[3 * k](x)))


def stage_forward(model, stage, x, r=_same):
    """One stage of hrnet_hip.HipViTPose.STAGES on its own: 'patch' reads crops (N, 3, H, W), the 'block*' and 'norm' stages read and
    return token MAPS (N, D, 16, 12), the deconvolutions feature maps."""
    with torch.no_grad():
        if stage == 'patch':
            return model.token_map(r(model.backbone.embed(x)))
        if stage.startswith('deconv'):
            return r(deconv_forward(model, int(stage[6:]), x))
        tok = x.flatten(2).transpose(1, 2)
        tok = r(model.backbone.last_norm(tok)) if stage == 'norm' else block_forward(model.backbone.blocks[int(stage[5:])], tok, r)
        return model.token_map(tok)


def stage_inputs(model, x):
    """The fp32 forward of the folded model on x (N, 3, H, W), tapped after every stage the executor can stop at (maps, as
    stage_forward returns them) plus 'heatmaps'."""
    out = {}
    stages = ('patch',) + tuple('block%d' % i for i in range(model.depth)) + ('norm', 'deconv0', 'deconv1')
    for s in stages:
        x = stage_forward(model, s, x)
        out[s] = x
    with torch.no_grad():
        out['heatmaps'] = model.keypoint_head.final_layer(x)
    return out


def emulate(model_bf16w, x, stages=None):
    """The bf16_storage emulation (module docstring) through `stages` (default: the whole network -> heat-maps): model_bf16w is
    bf16_weights(folded); x is the first stage's input."""
    whole = stages is None
    if whole:
        stages = ('patch',) + tuple('block%d' % i for i in range(model_bf16w.depth)) + ('norm', 'deconv0', 'deconv1')
    for s in stages:
        x = stage_forward(model_bf16w, s, x, _rnd)
    if whole:
        with torch.no_grad():
            x = model_bf16w.keypoint_head.final_layer(x)
    return x
