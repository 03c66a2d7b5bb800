"""GPU: the token kernels of csrc/pam_vit.hip.

Linear and patch embedding are pinned to exact bits with integer-valued operands (vit_cases.py).  GELU, LayerNorm and attention are
real-valued and compared with float64 under per-element bounds derived from the kernels' stated arithmetic; a result is accepted iff it
is a bf16 rounding of some value within delta of the reference (vit_cases.accepted).  No element is excluded.

  linear + GELU  the accumulator v is within dv = K 2^-24 sum|x w| of the float64 sum (the issue's bound; it holds the bias add too:
                 the test's biases are far below (K - 1) sum|x w|).  gelu(v) = 0.5 v (1 + erf(v / sqrt 2)) has |gelu'| <= 1.13, so dv
                 costs 1.13 dv.  The float32 evaluation adds: erff's own error, at most ERFF_ULP ulps of a value below 1, i.e.
                 ERFF_ULP 2^-24, times 0.5 |v|; the rounding of 1 + e (<= 2^-24, times 0.5 |v|); the rounding of the last product
                 (2^-24 |y|); the rounded argument v 0.70710678f, |dt| <= 2^-23 |t|, through erf' = 1.13 exp(-t^2): below
                 0.5 |v| 1.13 |t| exp(-t^2) 2^-23 <= 0.42 2^-23 for every v.   delta = 1.13 dv + (0.5 (ERFF_ULP + 1) |v| + |y| + 1) 2^-24.
                 ERFF_ULP comes from a device-versus-float64 sweep of erff over every float32 in [-8, 8] (the ROCm
                 installation documents no bound).
  LayerNorm      delta = (D 2^-23) (|gamma| |xhat| + |beta|), xhat the float64 normalised value.
  attention      delta = 2^-9 sum_j p_j |v_j| + 2^-18 max|v|: P's bf16 rounding plus float32 slack.  One bf16 rounding is up to 2^-8
                 relative, and a kernel that rounds P once missed this bound on the MI355X (13 of 110592 elements, by up to 1.15 x):
                 k_vit_attention feeds P to the product as two bf16 terms and stays at 0.65 of the bound."""
import math

import numpy as np
import pytest
import torch

import vit_cases as V

pytestmark = pytest.mark.gpu
DEV = V.DEV
ERFF_ULP = 2.0               # the sweep's largest error, rounded up to a whole ulp


@pytest.fixture(scope='module')
def eng():
    return V.engine()


def packed(w, b):
    from pam import packing
    return packing.PackedLinear(w.float(), None if b is None else b.float(), DEV)


# ---- exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
@pytest.mark.parametrize('m,k,n', V.LINEAR_SHAPES)
def test_linear_exact(eng, m, k, n, residual):
    d = V.linear_exact(m, k, n)
    op = packed(d['w'], d['b'])
    y = eng.linear(op, V.tokens_cl(d['x']), res=V.tokens_cl(d['r']) if residual else None)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (1, n, m, 1)
    assert torch.equal(V.rows(y), d['want_res' if residual else 'want'])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w,d', V.PATCH_SHAPES)
def test_patch_embed_exact(eng, h, w, d, n):
    from pam import vitpose
    c = V.patch_exact(n, h, w, d)
    conv = torch.nn.Conv2d(3, d, 16, 16, 2)
    with torch.no_grad():
        conv.weight.copy_(c['w'].float())
    op = packed(vitpose.patch_matrix(conv), None)
    x8 = c['x8'].to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    y = eng.patch_embed(op, c['pos'].float().to(DEV), x8)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (n, d, h // 16, w // 16)
    assert torch.equal(V.rows(y), c['want'])


def test_refusals(eng):
    """PAM_E_ARG (-1) on a null pointer and on every stated constraint, without a launch."""
    import ctypes as C
    lib, P = eng.lib, C.c_void_p
    buf = torch.zeros(1 << 16, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    p, q = P(buf.data_ptr()), P(f.data_ptr())
    lin = lambda *a: lib.pam_vit_linear_bf16(None, *a)
    assert lin(None, p, q, None, p, 16, 64, 64, 0) == -1 and lin(p, None, q, None, p, 16, 64, 64, 0) == -1
    assert lin(p, p, None, None, p, 16, 64, 64, 0) == -1 and lin(p, p, q, None, None, 16, 64, 64, 0) == -1
    assert lin(p, p, q, None, p, 16, 96, 64, 0) == -1 and lin(p, p, q, None, p, 16, 64, 96, 0) == -1       # K, N % 64
    assert lin(p, p, q, None, p, 0, 64, 64, 0) == -1 and lin(p, p, q, None, p, 16, 64, 64, 2) == -1
    assert lin(p, p, q, p, p, 16, 64, 64, 1) == -1                                                         # residual with GELU
    assert lin(p, p, q, None, p, 1 << 20, 1024, 64, 0) == -1                                               # M K 2 = 2^31: the frontier
    pe = lambda *a: lib.pam_vit_patch_embed_bf16(None, *a)
    assert pe(None, p, q, p, 1, 32, 16, 64) == -1 and pe(p, p, None, p, 1, 32, 16, 64) == -1
    assert pe(p, p, q, p, 1, 24, 16, 64) == -1 and pe(p, p, q, p, 1, 32, 8, 64) == -1 and pe(p, p, q, p, 1, 32, 16, 32) == -1
    assert pe(p, p, q, p, 2731, 256, 192, 64) == -1                                                        # N H W 16 >= 2^31
    ln = lambda *a: lib.pam_vit_layernorm_bf16(None, *a)
    assert ln(None, q, q, p, 1, 64, 1e-6) == -1 and ln(p, q, None, p, 1, 64, 1e-6) == -1
    assert ln(p, q, q, p, 1, 96, 1e-6) == -1 and ln(p, q, q, p, 1, 2112, 1e-6) == -1 and ln(p, q, q, p, 0, 64, 1e-6) == -1
    at = lambda *a: lib.pam_vit_attention_bf16(None, *a)
    assert at(None, p, 1, 16, 1) == -1 and at(p, None, 1, 16, 1) == -1
    assert at(p, p, 1, 8, 1) == -1 and at(p, p, 1, 24, 1) == -1 and at(p, p, 1, 208, 1) == -1 and at(p, p, 0, 16, 1) == -1
    assert at(p, p, 1, 16, 0) == -1 and at(p, p, 65536, 16, 1) == -1
    torch.cuda.synchronize()


# ---- real-valued --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,k,n', [(16, 64, 64), (192, 768, 3072), (208, 1024, 4096)])
def test_linear_gelu_within_the_derived_bound(eng, m, k, n):
    g = torch.Generator().manual_seed(m + k + n)
    x = torch.randn((m, k), generator=g).to(torch.bfloat16)
    w = (torch.randn((n, k), generator=g) * (2.0 / k ** 0.5)).to(torch.bfloat16)
    b = torch.randn(n, generator=g) * 0.5
    y = eng.linear(packed(w, b), V.tokens_cl(x), gelu=True)
    torch.cuda.synchronize()
    xd, wd = x.double(), w.double()
    v = xd @ wd.t() + b.double()
    ref = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    dv = k * 2.0 ** -24 * (xd.abs() @ wd.abs().t())
    delta = 1.13 * dv + (0.5 * (ERFF_ULP + 1.0) * v.abs() + ref.abs() + 1.0) * 2.0 ** -24
    assert float(v.abs().max()) > 4.0 and float(v.min()) < -3.0           # both tails of the GELU are reached
    assert V.report('gelu %s' % ((m, k, n),), V.rows(y).numpy(), ref.numpy(), delta.numpy()) == 0


def ln_rows(kind, m, d, g):
    if kind == 'normal':
        return torch.randn((m, d), generator=g) * 1.5 + 0.3
    dev = {'mean100_dev0.01': 0.01, 'mean100_dev0.5': 0.5}[kind]
    return 100.0 + dev * torch.randn((m, d), generator=g)


@pytest.mark.parametrize('kind', ['normal', 'mean100_dev0.01', 'mean100_dev0.5'])
@pytest.mark.parametrize('m', [1, 7, 192])
@pytest.mark.parametrize('d', [64, 768, 1024])
def test_layernorm_within_the_derived_bound(eng, d, m, kind):
    """mean100_dev0.01 is the issue's case (in bf16 such a row is 100.0 throughout: the variance is zero and the result is beta);
    mean100_dev0.5 keeps the offset and survives the rounding to bf16 as 99.5 / 100 / 100.5: the case a one-pass variance loses."""
    g = torch.Generator().manual_seed(d + 7 * m + len(kind))
    x = ln_rows(kind, m, d, g).to(torch.bfloat16)
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    beta = 0.2 * torch.randn(d, generator=g)
    y = eng.layernorm((gamma.to(DEV), beta.to(DEV), 1e-6), V.tokens_cl(x))
    torch.cuda.synchronize()
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    xhat = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + 1e-6)
    ref = xhat * gamma.double() + beta.double()
    delta = (d * 2.0 ** -23) * (gamma.double().abs() * xhat.abs() + beta.double().abs())
    assert V.report('layernorm D=%d M=%d %s' % (d, m, kind), V.rows(y).numpy(), ref.numpy(), delta.numpy()) == 0


def attention_ref(qkv, heads):
    """qkv (B, T, 3, heads, 64) float64 -> (out (B, T, heads 64), sum_j p_j |v_j| alike, max|v|)"""
    q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)]          # (B, heads, T, 64)
    s = (q @ k.transpose(-2, -1)) * 0.125
    p = torch.softmax(s, dim=-1)
    b, h, t, _ = q.shape
    back = lambda o: o.permute(0, 2, 1, 3).reshape(b, t, h * 64)
    return back(p @ v), back(p @ v.abs()), float(v.abs().max()), s


def run_attention(eng, qkv, heads):
    b, t = qkv.shape[:2]
    dev = qkv.to(torch.bfloat16).to(DEV).reshape(b, t, 1, 3 * heads * 64).permute(0, 3, 1, 2)      # (B, 3 heads 64, T, 1) channels-last
    y = eng.attention(dev, heads)
    torch.cuda.synchronize()
    return y.permute(0, 2, 3, 1).reshape(b, t, heads * 64).double().cpu()


@pytest.mark.parametrize('b', [1, 3])
@pytest.mark.parametrize('heads', [1, 12, 16])
@pytest.mark.parametrize('t', [16, 48, 192])
def test_attention_within_the_derived_bound(eng, t, heads, b):
    g = torch.Generator().manual_seed(t + 5 * heads + b)
    qkv = torch.randn((b, t, 3, heads, 64), generator=g)
    qkv[:, :, :2] *= 0.8                                                     # scores of a few units: a softmax that is neither flat nor one-hot
    qkv = qkv.to(torch.bfloat16).double()
    ref, pav, vmax, _ = attention_ref(qkv, heads)
    delta = 2.0 ** -9 * pav + 2.0 ** -18 * vmax
    got = run_attention(eng, qkv, heads)
    assert V.report('attention T=%d heads=%d B=%d' % (t, heads, b), got.numpy(), ref.numpy(), delta.numpy()) == 0


def test_attention_with_a_score_spread_of_80(eng):
    """Scores from -40 to +40 in every row: exp of an un-subtracted maximum would overflow nothing yet, but exp(40) / exp(-40) leaves
    float32's range as a ratio -- and with the row's own offset of +100 below, exp(s) itself overflows unless the maximum is subtracted."""
    t, heads, b = 192, 2, 1
    g = torch.Generator().manual_seed(80)
    qkv = torch.randn((b, t, 3, heads, 64), generator=g) * 0.25
    # channel 0 carries the spread: q0 = 8, k0 = -40 .. +40 in steps -> s = q0 k0 / 8; channel 1 adds +100 to every score of the row
    qkv[:, :, 0, :, 0] = 8.0
    qkv[:, :, 1, :, 0] = torch.linspace(-40.0, 40.0, t)[None, :, None]
    qkv[:, :, 0, :, 1] = 16.0
    qkv[:, :, 1, :, 1] = 50.0
    qkv = qkv.to(torch.bfloat16).double()
    ref, pav, vmax, s = attention_ref(qkv, heads)
    assert float((s.max(-1).values - s.min(-1).values).min()) >= 79.0 and float(s.max()) > 89.0       # exp(89) overflows float32
    delta = 2.0 ** -9 * pav + 2.0 ** -18 * vmax
    got = run_attention(eng, qkv, heads)
    assert bool(np.isfinite(got.numpy()).all())
    assert V.report('attention spread 80', got.numpy(), ref.numpy(), delta.numpy()) == 0
