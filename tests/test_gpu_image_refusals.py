"""GPU: what the image-side entry points (csrc/pam_head.hip, csrc/pam_crop.hip) refuse and what they accept, through the C ABI.
A refused call returns PAM_E_ARG (-1) before anything is launched: every output and the scratch buffer sit between guard bands and must
still hold their sentinel afterwards.  n == 0 is PAM_OK and writes nothing either, but only after the arguments were judged.  The DARK and
affine entries have their refusal tests in test_gpu_dark.py and test_gpu_affine_crop.py.
Smallest head shape of the suite: 32 channels, a 7 x 5 map, 1 crop (dark_ref.dark_inputs: rows plain, mirrored, spare); a 2 x 2 x 3 frame."""
import numpy as np
import pytest
import torch

import dark_ref as D
import image_ref as R
from test_gpu_flip import FlipHead
from test_gpu_image_shapes import Guarded, stream, up

pytestmark = pytest.mark.gpu

J = R.J
C_, H, W, N = 32, 7, 5, 1


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from pam import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def hd(lib, dev):
    feat, wt, b, boxes, _ = D.dark_inputs(C_, H, W, N)
    return FlipHead(lib, dev, feat, wt, b, boxes)


class Outputs(object):
    """One guarded buffer per output of the head entries, the scratch sized for the largest request (the soft decode's)."""

    def __init__(self, lib, hd, dev):
        self.scratch = Guarded(int(lib.pam_head_decode_soft_scratch_bytes(N, H, W)), torch.uint8, dev)
        self.det = Guarded(3 * hd.slots * J * 3, torch.float64, dev)
        self.kp = Guarded(hd.rows * J * 3, torch.float32, dev)
        self.heat = Guarded(hd.nf * hd.P * J, torch.float32, dev)
        self.all = (self.scratch, self.det, self.kp, self.heat)

    def untouched(self):
        torch.cuda.synchronize()
        return all(g.intact() and g.untouched(g.t) for g in self.all)


def head_args(hd, out, dev):
    """Valid arguments of the head entries by name; a case overrides some of them."""
    return dict(stream=stream(dev), n=N, flip_row0=N, h=H, w=W, feat=hd.f.data_ptr(), C=C_, wt=hd.wt.data_ptr(), bias=hd.b.data_ptr(), J=J, beta=4.0,
                flags=1, heat=out.heat.ptr(), view_of=hd.view_of.data_ptr(), slot_of=hd.slot_of.data_ptr(), boxes=hd.boxes.data_ptr(),
                slots=hd.slots, det=out.det.ptr(), kp=out.kp.ptr(), scratch=out.scratch.ptr(), n_pix=N * H * W, hm=hd.f.data_ptr(), nchw=0)


ORDER = {
    'pam_head_heatmaps': 'stream n_pix feat C wt bias J heat',
    'pam_head_decode': 'stream n h w feat C wt bias J heat view_of slot_of boxes slots det kp scratch',
    'pam_head_decode_soft': 'stream n h w feat C wt bias J beta heat view_of slot_of boxes slots det kp scratch',
    'pam_head_decode_flip': 'stream n flip_row0 h w feat C wt bias J flags heat view_of slot_of boxes slots det kp scratch',
    'pam_decode_heatmaps': 'stream n hm nchw h w view_of slot_of boxes slots det kp',
}
REQUIRED = {                                       # the pointers an entry cannot do without; `heat` is pam_head_heatmaps' output
    'pam_head_heatmaps': ['feat', 'wt', 'heat'],
    'pam_head_decode': ['feat', 'wt', 'view_of', 'slot_of', 'boxes', 'det', 'scratch'],
    'pam_head_decode_soft': ['feat', 'wt', 'view_of', 'slot_of', 'boxes', 'det', 'scratch'],
    'pam_head_decode_flip': ['feat', 'wt', 'view_of', 'slot_of', 'boxes', 'det', 'scratch'],
    'pam_decode_heatmaps': ['hm', 'view_of', 'slot_of', 'boxes', 'det'],
}
COUNT = {'pam_head_heatmaps': 'n_pix'}            # the name of the entry's crop / pixel count


def refused_cases(entry):
    names = ORDER[entry].split()
    cases = [{COUNT.get(entry, 'n'): -1}] + [{p: None} for p in REQUIRED[entry]]
    for key, values in (('h', (0, -1)), ('w', (0, -1)), ('C', (0, 12)), ('J', (16,))):
        cases += [{key: v} for v in values if key in names]
    if entry == 'pam_head_decode_soft':
        cases += [{'beta': 0.0}, {'beta': -1.0}, {'beta': float('nan')}]
    if entry == 'pam_head_decode_flip':
        cases += [{'flags': 8}, {'flags': 2}, {'flags': 6}, {'flags': 1, 'flip_row0': N - 1}]
    return cases


@pytest.mark.parametrize('entry', sorted(ORDER))
def test_head_entries_refuse_bad_arguments(lib, dev, hd, entry):
    """n < 0, each required pointer null in turn, a map extent <= 0, C of 0 and of 12, J of 16; beta of 0, -1 and NaN; flags outside the
    mask, SHIFT without MERGE, MERGE with flip_row0 < n: -1, and nothing written.  n == 0 with otherwise valid arguments: 0, nothing
    written; n == 0 with a bad argument is still refused."""
    out = Outputs(lib, hd, dev)
    base = head_args(hd, out, dev)
    names = ORDER[entry].split()
    fn = getattr(lib, entry)
    count = COUNT.get(entry, 'n')
    cases = refused_cases(entry)
    for case in cases:
        assert fn(*[dict(base, **case)[k] for k in names]) == -1, (entry, case)
    assert fn(*[dict(base, **{count: 0})[k] for k in names]) == 0, entry
    for case in cases[1:]:                                              # the refusal is decided before n == 0 returns
        if 'flip_row0' in case:                                         # (flip_row0 < n does not hold at n == 0)
            continue
        assert fn(*[dict(base, **dict(case, **{count: 0}))[k] for k in names]) == -1, (entry, case, 'n == 0')
    assert out.untouched(), entry


def test_scratch_sizes_refuse_bad_shapes(lib):
    for name in ('pam_head_decode_scratch_bytes', 'pam_head_decode_soft_scratch_bytes', 'pam_head_decode_flip_scratch_bytes'):
        fn = getattr(lib, name)
        assert fn(-1, H, W) == -1 and fn(N, 0, W) == -1 and fn(N, H, 0) == -1, name
        assert fn(0, H, W) == 0, name
    b = int(lib.pam_head_decode_scratch_bytes(3, 96, 72))
    assert b == 3 * 27 * J * 8 and int(lib.pam_head_decode_soft_scratch_bytes(3, 96, 72)) == b + b // 8 * 16


def test_optional_pointers_may_be_null(lib, dev, hd):
    """Null bias, heat-map and kp pointers are accepted by every entry that has them; the call then writes the det rows of its crop
    (the heat-maps for pam_head_heatmaps) and nothing else."""
    for entry in sorted(ORDER):
        out = Outputs(lib, hd, dev)
        base = head_args(hd, out, dev)
        maps = None
        if entry == 'pam_decode_heatmaps':
            maps = torch.from_numpy(hd.heatmaps()[:N]).to(dev).contiguous()
            base['hm'] = maps.data_ptr()
        null = dict(bias=None, kp=None) if entry == 'pam_head_heatmaps' else dict(bias=None, heat=None, kp=None)
        assert getattr(lib, entry)(*[dict(base, **null)[k] for k in ORDER[entry].split()]) == 0, entry
        torch.cuda.synchronize()
        assert all(g.intact() for g in out.all), entry
        assert out.kp.untouched(out.kp.t), entry
        if entry == 'pam_head_heatmaps':
            assert out.det.untouched(out.det.t) and not out.heat.untouched(out.heat.t[:N * H * W * J]), entry
        else:
            assert out.heat.untouched(out.heat.t), entry
            d = out.det.t.reshape(3, hd.slots, J, 3)
            assert not out.det.untouched(d[0, 0]) and out.det.untouched(torch.stack([d[i % 3, i // 3] for i in range(N, 3 * hd.slots)])), entry


def test_flip_entry_without_flags_is_the_plain_decode(hd):
    """pam_head_decode_flip with flags = 0 writes det, kp and heat-map rows byte-equal to pam_head_decode's."""
    for heat in (False, True):
        assert hd.decode(0, heat=heat)[3] == hd.decode(0, heat=heat, plain_entry=True)[3]


def test_crop_entries_refuse_bad_arguments(lib, dev):
    """pam_preprocess_crops_ex / _flip on a 2 x 2 x 3 frame: fewer output rows than crops (than twice the crops), out_c = 4 and
    out_h = 0 give -1 and write nothing; n == 0 is 0 and writes nothing; the valid call writes its rows."""
    frame = up(np.arange(12, dtype=np.uint8).reshape(2, 2, 3), dev)
    ptrs = torch.tensor([frame.data_ptr()], dtype=torch.int64, device=dev)
    view_of = torch.zeros(1, dtype=torch.int32, device=dev)
    boxes = torch.tensor([[0.0, 0.0, 2.0, 2.0]], dtype=torch.float32, device=dev)
    oh, ow = 4, 3
    for name, rows in (('pam_preprocess_crops_ex', 1), ('pam_preprocess_crops_flip', 2)):
        fn = getattr(lib, name)
        out = Guarded(rows * oh * ow * 8, torch.bfloat16, dev)

        def call(n=1, n_total=rows, out_h=oh, out_c=8):
            return fn(stream(dev), n, n_total, ptrs.data_ptr(), 2, 2, view_of.data_ptr(), boxes.data_ptr(), out_h, ow, out_c, out.ptr(), 0)
        for kw in (dict(n_total=rows - 1), dict(out_c=4), dict(out_h=0), dict(n=0, out_c=4)):
            assert call(**kw) == -1, (name, kw)
        assert call(n=0) == 0 and call(n=0, n_total=0) == 0, name
        torch.cuda.synchronize()
        assert out.intact() and out.untouched(out.t), name
        assert call() == 0 and call(out_c=3) == 0, name
        torch.cuda.synchronize()
        assert out.intact() and not out.untouched(out.t), name
