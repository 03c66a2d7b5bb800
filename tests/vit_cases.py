"""Shared by the ViT kernel tests (test infrastructure: nothing under the package imports this): the launch helper, the exact
integer-valued cases of the linear and patch-embedding kernels with their float64 references -- computed once per case and process,
read by test_gpu_vit_kernels.py and test_gpu_vit_guarded.py and never modified -- and the acceptance rule of the real-valued checks.

Exact cases: operands are small integers (|x| <= 3, weights in {-1, 0, 1}, integer bias / residual / position table), so every product
and every float32 partial sum is an integer below 2^24 and exact whatever the summation order; the kernel's one bf16 rounding of the
exact sum is the only rounding, and the reference applies the same rounding to the float64 result."""
import functools

import numpy as np
import torch

import image_ref as IR

DEV = torch.device('cuda:0')
LINEAR_SHAPES = [(16, 64, 64), (192, 768, 2304), (208, 3072, 768), (192 * 3, 1024, 4096)]      # (M, K, N)
PATCH_SHAPES = [(32, 16, 64), (32, 32, 128), (256, 192, 768)]                                    # (H, W, D), each with N = 1 and 3


def engine():
    """A bare launcher object: the executor's launch methods without a network."""
    from pam import _lib, hrnet_hip
    e = hrnet_hip.HipViTPose.__new__(hrnet_hip.HipViTPose)
    e.lib, e.device, e.count = _lib.load(), DEV, None
    return e


def tokens_cl(x2d, dev=DEV):
    """(M, C) -> the channels-last bf16 tensor (1, C, M, 1) on the device: M tokens of C channels, dense in memory"""
    m, c = x2d.shape
    return x2d.to(torch.bfloat16).to(dev).reshape(1, m, 1, c).permute(0, 3, 1, 2)


def rows(t):
    """a channels-last activation (N, C, h, w) -> (N h w, C) on the CPU, float64"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu()


def to_bf16_f64(v):
    """float64 tensor of values exact in float32 -> their bf16 rounding (RNE), as float64"""
    return v.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def linear_exact(m, k, n):
    g = torch.Generator().manual_seed(1000 + m + k + n)
    x = torch.randint(-3, 4, (m, k), generator=g).double()
    w = torch.randint(-1, 2, (n, k), generator=g).double()
    b = torch.randint(-8, 9, (n,), generator=g).double()
    r = torch.randint(-16, 17, (m, n), generator=g).double()
    s = x @ w.t() + b
    assert float(s.abs().max()) + 16 < 2 ** 24 and 3 * k < 2 ** 24
    return dict(x=x, w=w, b=b, r=r, want=to_bf16_f64(s), want_res=to_bf16_f64(s + r))


@functools.lru_cache(maxsize=None)
def patch_exact(n, h, w, d):
    """Integer crops with non-zero values in every pixel up to the edge (and in the 5 padding channels, whose weights are zero)."""
    g = torch.Generator().manual_seed(2000 + n + h + w + d)
    x8 = torch.randint(1, 4, (n, 8, h, w), generator=g).double() * (torch.randint(0, 2, (n, 8, h, w), generator=g).double() * 2 - 1)
    wt = torch.randint(-1, 2, (d, 3, 16, 16), generator=g).double()
    t = (h // 16) * (w // 16)
    pos = torch.randint(-8, 9, (t, d), generator=g).double()
    cols = torch.nn.functional.unfold(x8[:, :3], 16, padding=2, stride=16)               # (N, 768, T), float64
    s = torch.einsum('nkt,dk->ntd', cols, wt.reshape(d, -1)) + pos[None]
    return dict(x8=x8, w=wt, pos=pos, want=to_bf16_f64(s).reshape(n * t, d))


def accepted(got, ref, delta):
    """A result is accepted iff it is the bf16 rounding of some value within delta of the reference: rounding is monotone, so iff it lies
    between the roundings of ref - delta and ref + delta.  got, ref, delta: float64 arrays -> the boolean array."""
    got, ref, delta = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(delta, np.float64)
    return (got >= IR.bf16_rne(ref - delta)) & (got <= IR.bf16_rne(ref + delta))


def report(name, got, ref, delta):
    """Prints the figures of one real-valued check (`pytest -s`) and returns the number of elements outside the bound."""
    got, ref, delta = [np.asarray(a, np.float64) for a in (got, ref, delta)]
    ok = accepted(got, ref, delta)
    err = np.abs(got - ref)
    slack = err / np.maximum(delta + 0.5 * IR.bf16_ulp(ref), 1e-300)
    print('VITCHECK %s: %d elements, %d outside, max |err| %.3e, max err / (delta + half a bf16 ulp) %.3f' % (
        name, got.size, int((~ok).sum()), float(err.max()), float(slack.max())))
    return int((~ok).sum())
