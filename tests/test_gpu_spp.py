"""GPU: pam_spp_concat_nhwc_bf16 (YOLOv3-SPP's three stride-1 max-pools and the route over them, one launch) through the C ABI against
yolov3.darknet_maxpool + cat, bit for bit except that a zero may have either sign (include/pam.h), at the smallest shapes where it can go
wrong (spp_ref.CASES: maps smaller than the windows, non-square maps, the networks' maps, the kernel's limit; one vector of channels, a
channel count that is no multiple of a slab, 512 channels; 1, 3 and 5 views), with a guard band around the output, and every argument the
contract refuses.  The same shapes run on the CPU against the loop restatement of the contract in test_yolo_spp_cpu.py."""
import ctypes as C

import pytest
import torch

import spp_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4096                 # bf16 elements in front of and behind the output
SENTINEL = 0x5a5b            # their bit pattern (bf16 1.5e16: no pool of the planted inputs gives it)


def _lib():
    from pam import _lib
    return _lib.load()


def _guarded(numel):
    """A flat int16 buffer of sentinels and the address of the `numel` output elements in its middle (16-byte aligned)."""
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=DEV)
    assert (buf.data_ptr() + 2 * GUARD) % 16 == 0
    return buf, C.c_void_p(buf.data_ptr() + 2 * GUARD)


def _check(fn, case, *extra):
    n, c, h, w, sizes = case
    x = R.planted_input(n, c, h, w, 100 * h + w + c)
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous()                          # NHWC
    keep = xd.clone()
    numel = n * h * w * 4 * c
    buf, out = _guarded(numel)
    assert fn(None, C.c_void_p(xd.data_ptr()), out, n, h, w, c, *sizes, *extra) == 0
    torch.cuda.synchronize()
    assert torch.equal(R.bits(xd), R.bits(keep)), 'the input was written'
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + numel:] == SENTINEL).all()), 'a write outside the output'
    got = buf[GUARD:GUARD + numel].view(torch.bfloat16).reshape(n, h, w, 4 * c).cpu()
    want = R.torch_spp(x.float(), sizes).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
    ok = R.same_up_to_zero_sign(got, want)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        raise AssertionError('%d of %d elements differ; first (n, y, x, channel) %s: got %s want %s; channel blocks hit %s' % (
            len(bad), ok.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item(), sorted(set((bad[:, 3] // c).tolist()))))
    assert torch.equal(R.bits(got[..., 3 * c:]), R.bits(x.permute(0, 2, 3, 1)))        # the copy of the input: bitwise, zero signs included
    assert bool(torch.isinf(got[..., :3 * c]).any()) and bool((got[..., :3 * c] == R.BIG).any())     # the plants came through the pools


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_spp_bits_vs_darknet_maxpool(case):
    _check(_lib().pam_spp_concat_nhwc_bf16, case)


@pytest.mark.parametrize('slab', [8, 16, 32, 64])
@pytest.mark.parametrize('case', [R.CASES[6], R.CASES[7], R.CASES[8], R.CASES[9]], ids=[R.CASE_IDS[k] for k in (6, 7, 8, 9)])
def test_spp_every_slab_gives_the_same_bits(case, slab):
    """The channel slab per workgroup is a tuning choice (tools/bench_spp.py measures it): every value the entry accepts is correct, at 24
    channels (a last slab of 8 or 24 real channels), at the limit map (where 32 and 64 fall back to 16: 64 KB of LDS) and at 512 channels."""
    _check(_lib().pam_spp_concat_slab_nhwc_bf16, case, slab)


def test_spp_negative_zero_and_zero_channels():
    """Zero-padded or all-zero channels stay zero (of either sign); a map of -0.0 and 0.0 gives zeros; a window whose largest value is
    negative gives exactly that value."""
    lib = _lib()
    n, c, h, w = 2, 16, 13, 13
    x = torch.zeros((n, h, w, c), dtype=torch.bfloat16)
    x[..., 1] = -0.0
    x[:, ::2, :, 2] = -0.0
    x[..., 3] = -1.5
    x[:, 6, 6, 3] = -0.25
    xd = x.to(DEV)
    buf, out = _guarded(n * h * w * 4 * c)
    assert lib.pam_spp_concat_nhwc_bf16(None, C.c_void_p(xd.data_ptr()), out, n, h, w, c, 5, 9, 13) == 0
    torch.cuda.synchronize()
    got = buf[GUARD:-GUARD].view(torch.bfloat16).reshape(n, h, w, 4, c).cpu()
    assert bool((got[..., :3].float() == 0).all())
    assert torch.equal(R.bits(got[:, :, :, 3]), R.bits(x))
    for k, r in enumerate((6, 4, 2)):
        p = got[:, :, :, k, 3].float()
        inside = torch.zeros((h, w), dtype=torch.bool)
        inside[6 - r:6 + r + 1, 6 - r:6 + r + 1] = True
        assert bool((p[:, inside] == -0.25).all()) and bool((p[:, ~inside] == -1.5).all())


def test_spp_rejects_what_the_contract_rejects():
    """Every PAM_E_ARG case of include/pam.h; all are argument checks that return before a launch: after each one the output (and its
    guard band) still holds the sentinel everywhere."""
    from pam import _lib as L
    lib = L.load()
    assert L.SPP_MAX_HW == 32
    n, h, w, c = 1, 8, 8, 16
    xd = torch.zeros((n, h, w, c), dtype=torch.bfloat16, device=DEV)
    buf, out = _guarded(n * h * w * 4 * c)
    px = C.c_void_p(xd.data_ptr())
    good = (n, h, w, c, 5, 9, 13)
    bad = [(None, out) + good, (px, None) + good]
    for k, v in ((0, 0), (0, -1), (1, 0), (1, -3), (2, 0), (2, -1),          # N, H, W <= 0
                 (3, 12), (3, 4), (3, 0), (3, -8),                            # C % 8 != 0, C <= 0
                 (1, 33), (2, 33), (1, 64),                                   # a map above PAM_SPP_MAX_HW
                 (4, 4), (5, 8), (6, 12),                                     # an even size
                 (4, 1), (6, 15), (4, -5),                                    # outside 3 .. 13
                 (5, 5), (5, 3), (6, 9), (6, 7)):                             # not strictly ascending
        a = list(good)
        a[k] = v
        bad.append((px, out) + tuple(a))
    bad.append((px, out, n, h, w, c, 13, 9, 5))
    for args in bad:
        assert lib.pam_spp_concat_nhwc_bf16(None, *args) == -1, args[2:]
        assert lib.pam_spp_concat_slab_nhwc_bf16(None, *args, 32) == -1, args[2:]
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), args[2:]
    for slab in (0, 4, 12, 24, 128, -8):
        assert lib.pam_spp_concat_slab_nhwc_bf16(None, px, out, *good, slab) == -1, slab
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert lib.pam_spp_concat_nhwc_bf16(None, px, out, *good) == 0                # and the good call does write
    torch.cuda.synchronize()
    assert bool((buf[GUARD:-GUARD] == 0).all()) and bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def test_engine_spp_tallies_and_profiles_one_launch():
    """ConvEngine.spp: the (N, 4C, H, W) channels-last result, bytes = 2 x (in + out) and no FLOPs in the tally, one profile record named
    after the kernel, and a shape-only walk on the meta device launches nothing."""
    from pam import _lib, hrnet_hip
    e = hrnet_hip.ConvEngine()
    e.lib = _lib.load(); e.device = torch.device(DEV)
    e.count = dict(bytes=0, flops=0, launches=0); e.prof = []
    x = R.planted_input(2, 64, 13, 13, 5).to(DEV).contiguous(memory_format=torch.channels_last)
    y = e.spp(x, (5, 9, 13))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 256, 13, 13) and y.is_contiguous(memory_format=torch.channels_last)
    assert e.count == dict(bytes=2 * (x.numel() + y.numel()), flops=0, launches=1)
    assert len(e.prof) == 1 and e.prof[0]['family'] == 'k_spp' and e.prof[0]['flops'] == 0 and e.prof[0]['bytes'] == e.count['bytes']
    want = R.torch_spp(x.float().cpu(), (5, 9, 13)).to(torch.bfloat16)
    assert bool(R.same_up_to_zero_sign(y.cpu(), want).all())
    y.zero_()
    e.prof[0]['fn'](); torch.cuda.synchronize()                                   # the record re-issues exactly that launch
    assert bool(R.same_up_to_zero_sign(y.cpu(), want).all())
    m = e.spp(torch.empty((2, 64, 13, 13), dtype=torch.bfloat16, device='meta'), (5, 9, 13))
    assert tuple(m.shape) == (2, 256, 13, 13) and e.count['launches'] == 2 and len(e.prof) == 1
    with pytest.raises(_lib.PamError, match='pam_spp_concat_nhwc_bf16 failed'):
        e.spp(x, (5, 9, 12))
