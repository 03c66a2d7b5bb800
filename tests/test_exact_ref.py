"""CPU: the exact integer references of tests/exact_ref.py checked on their own -- the arithmetic helpers against brute force and
torch's bf16 cast, and, for EVERY case and regime of the tables the GPU tests launch (tests/test_gpu_exact.py): the exactness bound
(every sum below 2^24), the share of sharp outputs in each sharp regime, the spread and the ties of the rounding regime, and that each
planted fault (applied to the reference, never to a kernel) changes the reference's output in the regime meant to expose it."""
import pytest
import torch

import exact_ref as E

IDS = [c['id'] for c in E.CASES]
_clean = {}


def clean(case, regime):
    """The clean evaluation of (case, regime); kept for the tests of one case only."""
    if _clean.get('id') != case['id']:
        _clean.clear()
        _clean['id'] = case['id']
    if regime not in _clean:
        _clean[regime] = E.evaluate(case, regime)
    return _clean[regime]


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 5, 7, 9, 6, 3, 1), (1, 3, 9, 5, 4, 3, 2), (2, 8, 6, 7, 5, 1, 1), (1, 4, 7, 7, 3, 1, 2), (1, 2, 1, 1, 2, 3, 2)])
def test_direct_convolution_equals_brute_force(shape):
    n, cin, h, w, cout, k, stride = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-3, 4, (n, cin, h, w), generator=g)
    wt = torch.randint(-1, 2, (cout, cin, k, k), generator=g)
    pad = k // 2
    ho, wo = E.out_hw(h, w, k, stride)
    xp = torch.zeros((n, cin, h + 2 * pad, w + 2 * pad), dtype=torch.int64)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    want = torch.zeros((n, cout, ho, wo), dtype=torch.int64)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            want += torch.einsum('oc,nchw->nohw', wt[:, :, ky, kx], win)
    got = E.conv_direct(x.double(), wt.double(), stride, pad)
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got, want.double())


def test_transposed_convolution_as_a_direct_one_equals_its_definition():
    g = torch.Generator().manual_seed(4)
    n, cin, cout, h, w = 2, 3, 4, 3, 5
    x = torch.randint(-3, 4, (n, cin, h, w), generator=g)
    wd = torch.randint(-1, 2, (cout, cin, 4, 4), generator=g)
    wt = E.deconv_weight(wd)                                             # (Cin, Cout, 4, 4), as nn.ConvTranspose2d holds it
    want = torch.zeros((n, cout, 2 * h + 2, 2 * w + 2), dtype=torch.int64)          # output (2 i - 1 + ky, 2 j - 1 + kx), shifted by one
    for i in range(h):
        for j in range(w):
            want[:, :, 2 * i:2 * i + 4, 2 * j:2 * j + 4] += torch.einsum('nc,cokl->nokl', x[:, :, i, j], wt)
    got = E.conv_direct(E.deconv_as_conv(x.double()), wd.double(), 1, 2)
    assert torch.equal(got, want[:, :, 1:-1, 1:-1].double())


def test_rne_bf16_ties_to_even_and_agrees_with_the_cast():
    # 257 lies between 256 (even mantissa) and 258 (odd): down; 259 between 258 and 260: up; 513 / 515 / 517 are no ties
    t = torch.tensor([257.0, 259.0, -257.0, -259.0, 513.0, 514.0, 515.0, 518.0, 255.0, 0.0, -0.0, 65792.0])
    assert E.rne_bf16(t).tolist() == [256.0, 260.0, -256.0, -260.0, 512.0, 512.0, 516.0, 520.0, 255.0, 0.0, -0.0, 65536.0]
    assert E.is_tie(t).tolist() == [True, True, True, True, False, True, False, True, False, False, False, True]
    assert E.trunc_bf16(t).tolist() == [256.0, 258.0, -256.0, -258.0, 512.0, 512.0, 512.0, 516.0, 255.0, 0.0, -0.0, 65536.0]
    g = torch.Generator().manual_seed(1)
    for v in (torch.randn(20000, generator=g) * 1000, torch.randint(-70000, 70000, (20000,), generator=g).float(),
              torch.randn(20000, generator=g) * 1e-3, torch.arange(-4096, 4097).float()):
        assert torch.equal(E.rne_bf16(v), v.to(torch.bfloat16).float())
        assert torch.equal(E.rne_bf16(v.double()), v.to(torch.bfloat16).float())
    assert E.rne_bf16(torch.tensor([300.0])).dtype == torch.float32
    with pytest.raises(AssertionError):
        E.rne_bf16(torch.tensor([0.1], dtype=torch.float64))              # not a float32: the caller lost track of a rounding


def test_leaky32_is_one_float32_multiply():
    v = torch.tensor([-7.0, -1.0, 0.0, 3.0, -300.0], dtype=torch.float64)
    got = E.leaky32(v)
    assert got.dtype == torch.float32
    tenth = torch.tensor(0.1, dtype=torch.float32)
    assert got.tolist() == [float(tenth * -7), float(tenth * -1), 0.0, 3.0, float(tenth * -300)]
    assert float(got[0].double()) != -0.7                                 # the float32 product, not the real number


def test_generator_ranges_and_determinism():
    case = next(c for c in E.CASES if c['id'] == 'bn-2x7x5-later-next')
    for regime in E.regimes(case):
        D, _ = E.evaluate(case, regime)
        D2, _ = E.evaluate(case, regime)
        for k, t in D.t.items():
            if t is None or k.endswith('.sign'):
                continue
            assert torch.equal(t, D2.t[k]) and torch.equal(t, t.round())
            lo, hi = float(t.min()), float(t.max())
            if k.startswith('w'):
                assert -1 <= lo and hi <= 1
            elif k.startswith('b'):
                assert -8 <= lo and hi <= 8
            else:
                assert 0 <= lo and hi <= 3, k                            # layer1 is fed post-ReLU tensors only
    sharp = E.Data(case, 'sharp-0')
    E.REFS['bneck'](sharp, E.Run(), case)
    assert sharp.dens['w2'] == E.DENSE_W and sharp.dens['w3'] < 0.1 and sharp.dens['w1n'] < 0.1


def test_tables():
    assert len(set(IDS)) == len(IDS)
    for c in E.CASES:
        assert c['variants'], c['id']
        assert E.gflop(c) <= 5.0, (c['id'], E.gflop(c))                 # one evaluation of the reference
        assert c['n'] <= 3 or c['id'] in ('c3-48-rounds', 'cs-192-small', 'slab32-384', 'slab32-384-lin'), c['id']


# ---- every case, every regime -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', E.CASES, ids=IDS)
def test_exactness_sharpness_and_rounding_conditions(case):
    regs = E.regimes(case)
    assert regs[-1] == 'rounding' and len(regs) == len(E.STAGE_K[case['family']](case)) + 1
    for regime in regs:
        D, R = clean(case, regime)
        assert R.outs and set(R.outs) <= set(R.bound)
        for name, bound in R.bound.items():
            assert bound < E.LIMIT, (case['id'], regime, name, bound)
        for name, o in R.outs.items():
            assert torch.equal(o['ref'], o['ref'].to(torch.bfloat16).float())
            if regime != 'rounding':
                need = E.SHARP_LINEAR if o['linear'] else E.SHARP_ACT
                assert o['sharp'] >= need, (case['id'], regime, name, o['sharp'])
        if regime == 'rounding':
            for name, o in R.outs.items():
                assert o['big'] >= E.ROUNDING_BIG, (case['id'], name, o['big'])
            ties = sum(o['ties'] for o in R.outs.values())
            numel = sum(o['numel'] for o in R.outs.values())
            if case['id'] == 'stem-1x4x4':
                # the one case that cannot hold 100 ties: one pixel of x0 and of y1, 128 compared outputs in all.  About one output in
                # eight can be a tie (half are ReLU'd away, about a quarter of the others sit on an odd multiple of half a step)
                assert numel == 128 and ties >= 1, (ties, numel)
            else:
                assert ties >= E.ROUNDING_TIES, (case['id'], ties, numel)


@pytest.mark.parametrize('case', E.CASES, ids=IDS)
def test_planted_faults_change_the_reference(case):
    for fault, stage in E.applicable_faults(case):
        kind = E.FAULTS[fault][1]
        regime = 'rounding' if kind == 'rounding' else 'sharp-%d' % stage
        D, R = clean(case, regime)
        _, Rf = E.evaluate(case, regime, fault, stage, base=R, data=D)
        assert Rf.applied, (case['id'], fault, stage)
        assert set(Rf.outs) == set(R.outs)
        differ = sum(int((Rf.outs[n]['ref'] != R.outs[n]['ref']).sum()) for n in R.outs)
        assert differ > 0, (case['id'], regime, fault, stage, E.FAULTS[fault][0])
