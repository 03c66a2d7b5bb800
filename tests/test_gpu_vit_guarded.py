"""GPU: the ViT kernels in sentinel-filled, banded memory (tests/guarded_mem.py), under the rules of test_gpu_guarded_forward.py.

The exact cases of vit_cases.py (linear with and without residual, patch embedding) are launched with their outputs carved from a
GuardArena and their inputs -- activation and residual -- between poison bands, once per fill of guarded_mem.FILLS: the result must be
the exact bits, no band may be damaged and no output element left unwritten.  Then one whole ViTPose-B forward at 1 and 3 crops the same
way against its own unguarded result (guarded_forward of test_gpu_guarded_forward.py), and the product's arena: a captured replay gives
the same bits whatever the buffer held before."""
import pytest
import torch

import conv_plan_cases as P
import guarded_mem as G
import test_gpu_guarded_forward as GF
import vit_cases as V

pytestmark = pytest.mark.gpu
DEV = V.DEV


@pytest.fixture(scope='module')
def eng():
    return V.engine()


def _guarded(eng, nbytes, launch, inputs, want, tag):
    """launch(*poisoned inputs) under every fill: exact bits, intact bands, every output element written"""
    ar = G.GuardArena(DEV, nbytes + 8 * G.GUARD + 4 * G.ALIGN)
    views = [G.poisoned(t, G.FILLS[0]) for t in inputs]
    bad = []
    try:
        for fill in G.FILLS:
            for _, h in views:
                h.refill(fill)
            ar.reset()
            eng.arena = ar
            y = launch(*[v for v, _ in views])
            torch.cuda.synchronize()
            eng.arena = None
            assert len(ar.allocs) == 1 and ar.buf.data_ptr() <= y.data_ptr() < ar.buf.data_ptr() + 2 * ar.buf.numel()
            if not torch.equal(V.rows(y), want):
                bad.append('%s fill %#06x: %d of %d elements differ from the exact result' % (tag, fill, int((V.rows(y) != want).sum()), want.numel()))
            rep = ar.report()
            if rep:
                bad.append('%s fill %#06x: %s' % (tag, fill, rep))
    finally:
        eng.arena = None
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
@pytest.mark.parametrize('m,k,n', V.LINEAR_SHAPES)
def test_linear_exact_in_guarded_memory(eng, m, k, n, residual):
    from pam import packing
    d = V.linear_exact(m, k, n)
    op = packing.PackedLinear(d['w'].float(), d['b'].float(), DEV)
    ins = [V.tokens_cl(d['x']).contiguous(memory_format=torch.channels_last)] + ([V.tokens_cl(d['r']).contiguous(memory_format=torch.channels_last)] if residual else [])
    _guarded(eng, 2 * m * n, lambda x, r=None: eng.linear(op, x, res=r), ins, d['want_res' if residual else 'want'],
             'linear %s%s' % ((m, k, n), ' + residual' if residual else ''))


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w,d', V.PATCH_SHAPES)
def test_patch_embed_exact_in_guarded_memory(eng, h, w, d, n):
    from pam import packing, vitpose
    c = V.patch_exact(n, h, w, d)
    conv = torch.nn.Conv2d(3, d, 16, 16, 2)
    with torch.no_grad():
        conv.weight.copy_(c['w'].float())
    op = packing.PackedLinear(vitpose.patch_matrix(conv), None, DEV)
    pos = c['pos'].float().to(DEV)
    x8 = c['x8'].to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    _guarded(eng, 2 * n * (h // 16) * (w // 16) * d, lambda x: eng.patch_embed(op, pos, x), [x8], c['want'], 'patch %s n=%d' % ((h, w, d), n))


class Nets(object):
    """What guarded_forward asks of test_gpu_guarded_forward.Nets, for the one executor of this file."""

    def __init__(self):
        self.hip, self.arena = None, None

    def get(self, name):
        from pam import hrnet_hip, vitpose
        if self.hip is None:
            self.hip = hrnet_hip.HipViTPose(vitpose.folded_random_model('B'), DEV)
        return self.hip, 256, 192, True

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
    n.hip = n.arena = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize('n', [1, 3])
def test_vitpose_b_forward_in_guarded_memory(nets, n):
    GF.guarded_forward(nets, 'vitpose_b', 'vit', n, False)


def test_replay_is_independent_of_the_arena_contents():
    GF.test_replay_is_independent_of_the_arena_contents('B', 'ViTPose', (256, 192))
