"""CPU: the guarded-memory helper of tests/guarded_mem.py checked on its own (device 'cpu'): a clean pass reports nothing, and every
fault -- planted in the buffer by the test itself, never in a kernel -- is reported with the right allocation, side and distance."""
import pytest
import torch

import guarded_mem as G

S = G.as_i16(G.SENTINEL)
SHAPES = [(2, 48, 5, 3), (1, 8, 3, 7), (3, 64, 2, 2), (1, 3, 5, 5)]     # 2880, 336, 1536 and 150 bytes: only the third is a multiple of 256


def arena():
    a = G.GuardArena('cpu', 1 << 20)
    return a, [a.alloc(*s) for s in SHAPES]


def fill_all(ts):
    for i, t in enumerate(ts):
        t.copy_(torch.full(t.shape, float(i + 1)))                       # a torch op writes every payload element


def test_sentinel_is_a_positive_nan_and_fills_are_what_they_say():
    v = torch.tensor([S, G.as_i16(0x7F00), G.as_i16(0xFF00)], dtype=torch.int16).view(torch.bfloat16).float()
    assert S > 0 and bool(torch.isnan(v[0])) and not bool(torch.signbit(v[0]))
    assert 1.6e38 < float(v[1]) < 1.8e38 and float(v[2]) == -float(v[1])
    assert G.FILLS == (0x7FE5, 0x7F00, 0xFF00) and G.GUARD == 4096


def test_layout_alignment_bands_and_record():
    a, ts = arena()
    end = 0
    for k, (t, rec) in enumerate(zip(ts, a.allocs)):
        n, c, h, w = SHAPES[k]
        assert rec['order'] == k and rec['shape'] == SHAPES[k] and rec['nbytes'] == 2 * n * c * h * w
        assert t.data_ptr() % 256 == 0 and t.data_ptr() == a.buf.data_ptr() + rec['offset']
        assert tuple(t.shape) == SHAPES[k] and t.stride() == (h * w * c, 1, w * c, c) and t.dtype == torch.bfloat16
        assert rec['front'] == end and rec['offset'] - rec['front'] >= 2 * G.GUARD              # the band in front: from the last band's end
        assert rec['back'] == rec['offset'] + rec['nbytes'] + 2 * G.GUARD                      # the band behind: at the last byte + 1, no slack
        end = rec['back']
        assert bool((a.payload(rec) == S).all())                                              # a payload starts out as sentinel
    assert a.violations() == [] and a.unwritten() == [r['nbytes'] // 2 for r in a.allocs]
    assert a.buf.dtype == torch.int16 and a.half_bytes == 1 << 20
    a.epoch()
    assert len(a.allocs) == 4


def test_clean_pass_reports_nothing():
    a, ts = arena()
    fill_all(ts)
    assert a.violations() == [] and a.unwritten() == [0, 0, 0, 0] and a.report() == ''


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_planted_faults_are_reported_with_allocation_side_and_distance(k):
    a, ts = arena()
    rec = a.allocs[k]
    lo, hi = rec['offset'] // 2, (rec['offset'] + rec['nbytes']) // 2
    plant = [('behind', hi, 0),                                          # just behind the payload: its last byte + 1, also for the
             ('before', lo - 1, 0),                                      # sizes that are no multiple of 256; just before it
             ('behind', hi + G.GUARD - 1, 2 * (G.GUARD - 1)),            # the far end of the band behind
             ('before', rec['front'] // 2, 2 * (lo - 1 - rec['front'] // 2))]   # the far end of the band in front
    for side, at, dist in plant:
        a.reset()
        ts = [a.alloc(*s) for s in SHAPES]
        fill_all(ts)
        a.buf[at] = 0x3F80                                               # 1.0
        assert a.violations() == [dict(order=k, shape=SHAPES[k], offset=rec['offset'], side=side, first=dist, last=dist, changed=1)], (side, at)
        assert a.unwritten() == [0, 0, 0, 0]
        assert 'allocation %d' % k in a.report() and side in a.report()
    # two damaged elements in one band: nearest and farthest distance, and the count
    a.reset()
    fill_all([a.alloc(*s) for s in SHAPES])
    a.buf[hi + 3] = 0; a.buf[hi + 16] = 0
    assert a.violations() == [dict(order=k, shape=SHAPES[k], offset=rec['offset'], side='behind', first=6, last=32, changed=2)]


def test_an_unwritten_payload_element_is_counted_for_its_allocation():
    a, ts = arena()
    fill_all(ts)
    a.payload(a.allocs[2])[17] = S
    a.payload(a.allocs[3])[0] = S; a.payload(a.allocs[3])[-1] = S
    assert a.unwritten() == [0, 0, 1, 2] and a.violations() == []
    assert 'allocation 2 (3, 64, 2, 2): 1 of 768 elements never written' in a.report()


def test_comparison_is_on_raw_bits():
    """Another NaN in a band is damage (a float comparison could not tell), and a written NaN of another payload is not 'unwritten'."""
    a, ts = arena()
    fill_all(ts)
    rec = a.allocs[0]
    a.buf[(rec['offset'] + rec['nbytes']) // 2 + 5] = 0x7FC0
    a.payload(rec)[3] = 0x7FC0
    v = a.violations()
    assert len(v) == 1 and v[0]['first'] == 10 and a.unwritten() == [0, 0, 0, 0]


def test_reset_refills_and_forgets():
    a, ts = arena()
    fill_all(ts)
    a.buf[a.allocs[1]['back'] // 2 - 1] = 0
    assert a.violations()
    a.reset()
    assert a.allocs == [] and bool((a.buf == S).all())
    t = a.alloc(*SHAPES[0])
    assert t.data_ptr() % 256 == 0 and a.allocs[0]['order'] == 0 and a.violations() == []


def test_arena_too_small_raises():
    a = G.GuardArena('cpu', 4 * G.GUARD + 1024)
    a.alloc(1, 8, 2, 2)
    with pytest.raises(RuntimeError):
        a.alloc(1, 8, 64, 64)


def test_measuring_arena_covers_what_the_guard_arena_takes():
    m = G.MeasuringArena()
    for n, c, h, w in SHAPES:
        m.count(2 * n * c * h * w)
    a = G.GuardArena('cpu', m.capacity())
    for s in SHAPES:
        a.alloc(*s)
    assert m.n == 4 and a.peak <= m.capacity()


@pytest.mark.parametrize('shape', [(2, 48, 5, 3), (1, 8, 4, 4), (3, 144, 2, 3)])
def test_poisoned_view_strides_alignment_bands_and_refill(shape):
    g = torch.Generator().manual_seed(7)
    t = torch.randint(-3, 4, shape, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    v, hd = G.poisoned(t, 0x7F00)
    assert torch.equal(v, t) and v.stride() == t.stride() and v.data_ptr() % 256 == 0
    assert v.is_contiguous(memory_format=torch.channels_last)
    front, back = hd.bands()
    assert front.numel() >= G.GUARD and back.numel() == G.GUARD
    assert front.data_ptr() + 2 * front.numel() == v.data_ptr()                                # the bands touch the payload
    assert back.data_ptr() == v.data_ptr() + 2 * t.numel()
    assert bool((front == G.as_i16(0x7F00)).all()) and bool((back == G.as_i16(0x7F00)).all())
    for fill in G.FILLS + (0x0000,):
        hd.refill(fill)
        assert torch.equal(v, t)                                                               # refill leaves the payload unchanged
        assert bool((front == G.as_i16(fill)).all()) and bool((back == G.as_i16(fill)).all())
    # a channel slice of the wide tensor keeps the strides the engine asserts
    s = v[:, 8:8 + shape[1] // 2]
    assert s.stride() == t[:, 8:8 + shape[1] // 2].stride() and s.stride(1) == 1 and s.stride(3) == shape[1]


def test_poisoned_refuses_what_is_not_dense_channels_last_bf16():
    t = torch.zeros((2, 16, 4, 4), dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        G.poisoned(t, 0)                                                 # NCHW
    with pytest.raises(AssertionError):
        G.poisoned(t.contiguous(memory_format=torch.channels_last)[:, :8], 0)
    with pytest.raises(AssertionError):
        G.poisoned(t.float().contiguous(memory_format=torch.channels_last), 0)


def test_conv_engine_carves_its_outputs_from_a_guard_arena():
    from pam import engine
    e = engine.ConvEngine()
    e.arena = G.GuardArena('cpu', 1 << 20)
    y = e._new(2, 48, 5, 3, torch.device('cpu'))
    z = e._new(1, 64, 2, 2, torch.device('cpu'))
    lo, hi = e.arena.buf.data_ptr(), e.arena.buf.data_ptr() + 2 * e.arena.buf.numel()
    for t, rec in zip((y, z), e.arena.allocs):
        assert lo <= t.data_ptr() < hi and t.data_ptr() == lo + rec['offset'] and tuple(t.shape) == rec['shape']
        assert t.is_contiguous(memory_format=torch.channels_last) and t.dtype == torch.bfloat16
    assert e.arena.unwritten() == [2 * 48 * 5 * 3, 64 * 2 * 2]
    y.zero_(); z.zero_()
    assert e.arena.report() == ''
    # a shape-only walk only counts
    m = e.arena = G.MeasuringArena()
    e._new(2, 48, 5, 3, torch.device('meta'))
    assert m.n == 1 and m.total >= 2 * 2 * 48 * 5 * 3 + 4 * G.GUARD
