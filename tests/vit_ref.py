"""ViTPose ("classic decoder") restated in float64 NumPy from its published definition (test infrastructure: nothing under the package
imports this, and this imports nothing from the package -- neither vitpose.py nor the packing).

    patch embedding  Conv2d(3, D, 16, stride 16, padding 2) on the 256 x 192 crop -> 16 x 12 = 192 tokens
    position table   x = x + pos[:, 1:] + pos[:, :1]                       (pos (1, T + 1, D))
    blocks           x += proj(attn(LN1(x))); x += fc2(GELU(fc1(LN2(x))))  (LayerNorm eps 1e-6, heads of 64 channels, scale 1/8,
                                                                            softmax over all keys, exact GELU, MLP ratio 4)
    last_norm        LayerNorm
    head             tokens as (D, 16, 12); 2 x [ConvTranspose2d(., 256, 4, stride 2, padding 1) + BN + ReLU]; Conv2d(256, J, 1)

``forward(sd, x, heads, fault=None)`` takes the state dict in the published key layout as float64 arrays.  ``fault`` plants one
deviation (FAULTS) so that the comparison of test_vit_ref.py can be shown to catch it."""
import math

import numpy as np
from scipy.special import erf as _erf

FAULTS = ('pos_row0', 'no_scale', 'tanh_gelu', 'post_norm', 'pad0')


def layernorm(x, g, b, eps=1e-6):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def linear(x, w, b):
    return np.einsum('...k,nk->...n', x, w) + b


def patch_embed(x, w, b, pad=2):
    """x (N, 3, H, W), w (D, 3, 16, 16) -> (N, T, D), tokens row by row"""
    n, c, h, wd = x.shape
    xp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad))
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    th, tw = (h + 2 * pad - 16) // 16 + 1, (wd + 2 * pad - 16) // 16 + 1
    patches = np.stack([np.stack([xp[:, :, 16 * i:16 * i + 16, 16 * j:16 * j + 16] for j in range(tw)], 1) for i in range(th)], 1)   # (N, th, tw, 3, 16, 16)
    return np.einsum('pk,dk->pd', patches.reshape(n * th * tw, -1), w.reshape(w.shape[0], -1)).reshape(n, th * tw, -1) + b, (th, tw)


def attention(x, wqkv, bqkv, wproj, bproj, heads, scale=True):
    n, t, d = x.shape
    hd = d // heads
    qkv = linear(x, wqkv, bqkv).reshape(n, t, 3, heads, hd)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    s = np.einsum('nqhc,nkhc->nhqk', q, k) * (hd ** -0.5 if scale else 1.0)
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    return linear(np.einsum('nhqk,nkhc->nqhc', p, v).reshape(n, t, d), wproj, bproj)


def deconv4x4s2(x, w):
    """ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1): x (N, Cin, H, W), w (Cin, Cout, 4, 4) -> (N, Cout, 2H, 2W)"""
    n, _, h, wd = x.shape
    full = np.zeros((n, w.shape[1], 2 * h + 2, 2 * wd + 2))
    for ky in range(4):
        for kx in range(4):
            full[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += np.einsum('nchw,co->nohw', x, w[:, :, ky, kx])
    return full[:, :, 1:1 + 2 * h, 1:1 + 2 * wd]


def batchnorm(x, p, pre, eps=1e-5):
    s = p[pre + '.weight'] / np.sqrt(p[pre + '.running_var'] + eps)
    return (x - p[pre + '.running_mean'][None, :, None, None]) * s[None, :, None, None] + p[pre + '.bias'][None, :, None, None]


def forward(sd, x, heads, fault=None, stop=None):
    """sd: {key: float64 array} in the published layout; x (N, 3, H, W) float64 -> the (N, J, H / 4, W / 4) heat-maps (stop='tokens': the
    (N, T, D) tokens behind last_norm)."""
    assert fault is None or fault in FAULTS, fault
    bb = 'backbone.'
    tok, (th, tw) = patch_embed(x, sd[bb + 'patch_embed.proj.weight'], sd[bb + 'patch_embed.proj.bias'], pad=0 if fault == 'pad0' else 2)
    pos = sd[bb + 'pos_embed']
    t = th * tw
    tok = tok + pos[:, 1:1 + t] + (0.0 if fault == 'pos_row0' else pos[:, :1])
    depth = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith(bb + 'blocks.'))
    for i in range(depth):
        p = bb + 'blocks.%d.' % i
        ln = lambda y, name: layernorm(y, sd[p + name + '.weight'], sd[p + name + '.bias'])
        att = lambda y: attention(y, sd[p + 'attn.qkv.weight'], sd[p + 'attn.qkv.bias'], sd[p + 'attn.proj.weight'], sd[p + 'attn.proj.bias'],
                                  heads, scale=fault != 'no_scale')
        mlp = lambda y: linear(gelu(linear(y, sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias']), tanh=fault == 'tanh_gelu'),
                               sd[p + 'mlp.fc2.weight'], sd[p + 'mlp.fc2.bias'])
        if fault == 'post_norm':
            tok = ln(tok + att(tok), 'norm1')
            tok = ln(tok + mlp(tok), 'norm2')
        else:
            tok = tok + att(ln(tok, 'norm1'))
            tok = tok + mlp(ln(tok, 'norm2'))
    tok = layernorm(tok, sd[bb + 'last_norm.weight'], sd[bb + 'last_norm.bias'])
    if stop == 'tokens':
        return tok
    n, _, d = tok.shape
    y = tok.transpose(0, 2, 1).reshape(n, d, th, tw)
    kh = 'keypoint_head.'
    for i in (0, 3):
        y = deconv4x4s2(y, sd[kh + 'deconv_layers.%d.weight' % i])
        y = np.maximum(batchnorm(y, sd, kh + 'deconv_layers.%d' % (i + 1)), 0.0)
    return np.einsum('nchw,jc->njhw', y, sd[kh + 'final_layer.weight'][:, :, 0, 0]) + sd[kh + 'final_layer.bias'][None, :, None, None]
