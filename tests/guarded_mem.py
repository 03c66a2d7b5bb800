"""Sentinel-filled, banded activation memory for the conv-stack tests (a plain helper, imported like exact_ref.py; CPU or GPU).

Three things a value comparison cannot see on memory that comes from the caching allocator:
  * an output element the kernel never wrote can hold the right answer already -- a block another variant of the same case just freed,
    or zeros, which is what half of a ReLU output is;
  * a store outside the output lands in nobody's tensor (in the product it lands in the next activation of the arena);
  * a load outside the input reads whatever lies there, usually zeros, and a zero added to a sum changes nothing.

``GuardArena`` stands in for engine.ActivationArena (``ConvEngine.arena``): every output a launcher asks for is carved out of ONE int16
buffer that holds ``SENTINEL`` everywhere.  A payload starts on a 256-byte boundary as in the product's arena, starts out as sentinel
itself, and lies between two bands of at least ``GUARD`` sentinel elements: the band behind it begins at its last byte + 1 with no
slack, the band in front of it reaches back to the end of the previous allocation's band (so every element of the buffer belongs to a
payload or to a band).  Nothing is ever reused (``epoch()`` does nothing).  ``violations()`` names every band that no longer holds the
sentinel -- on raw bits -- and ``unwritten()`` counts the payload elements that still do.

``SENTINEL`` = 0x7FE5 is a positive bf16 NaN whose payload no rounding of the kernels produces (a NaN they make is the canonical
0x7FC0 / 0xFFC0 or carries an operand's payload, and the operands here are integers).  Positive, because the epilogues' ReLU is a packed
signed-integer max with 0: a negative pattern would be "written" as 0 by a kernel that only clamps what it finds.

``poisoned(t, fill)`` puts an INPUT between two bands of ``GUARD`` elements of ``fill``, at a 256-byte-aligned address and with the
strides of the original, so that a load outside the tensor that reaches a result changes that result.  ``FILLS`` holds the three
patterns a launch is repeated under, and all three are needed:
  * 0x7F00 = +1.7e38 and 0xFF00 = -1.7e38: a stray element that is multiplied by a weight of +1 or -1 (the exact tests' weights are
    -1, 0, 1) adds +-1.7e38 to a sum whose honest part is below 2^24.  Under a ReLU only the positive one of the two products survives
    -- +fill for w = +1, -fill for w = -1 --, so each sign of weight needs its own fill; a linear output shows under both;
  * 0x7FE5 = NaN: a stray element times a ZERO weight is 0 for either finite fill and shows under neither, while NaN * 0 is NaN and
    poisons the sum.  NaN alone would not do: what a kernel only compares (a max-pool tap, a clamp) can drop a NaN and keep +-1.7e38,
    and an integer ReLU turns a NaN whose sign bit came out set into 0, which is what half of the reference holds.
For a channel slice the WIDE tensor is the payload: the neighbour channels hold generated integers already (exact_ref.ref_conv)."""
import torch

SENTINEL = 0x7FE5            # positive bf16 NaN, as int16 32741
GUARD = 4096                 # bf16 elements of band on each side: the value of the other guarded tests (a condition, not a measurement)
FILLS = (0x7FE5, 0x7F00, 0xFF00)
ALIGN = 256                  # bytes, engine.ActivationArena's rounding


def as_i16(bits):
    """A 16-bit pattern as the int16 value that holds it."""
    bits = int(bits) & 0xFFFF
    return bits - 0x10000 if bits & 0x8000 else bits


class GuardArena(object):
    """What ConvEngine._new and the executors use of ActivationArena -- alloc, count, epoch, buf, half_bytes -- over sentinel-filled,
    banded memory that is never reused.  ``allocs``: one dict(order, offset, nbytes, shape) per call of alloc, offsets in bytes."""

    def __init__(self, device, capacity_bytes):
        self.half_bytes = int(capacity_bytes) // ALIGN * ALIGN
        self.buf = torch.full((self.half_bytes // 2,), as_i16(SENTINEL), dtype=torch.int16, device=device)
        self.base = self.buf.data_ptr() % ALIGN     # (a CPU buffer is aligned to 64 bytes only: payloads are aligned by ADDRESS)
        self.allocs = []
        self.off = 0                 # byte offset of the first byte behind the last band
        self.peak = 0

    def epoch(self):
        pass

    def count(self, nbytes):
        """Accounting of a shape-only walk (nothing is carved): the bytes alloc would have taken."""
        start = (self.base + self.off + 2 * GUARD + ALIGN - 1) // ALIGN * ALIGN - self.base
        self.off = start + int(nbytes) + 2 * GUARD
        self.peak = max(self.peak, self.off)

    def alloc(self, n, c, h, w):
        nbytes = 2 * n * c * h * w
        lo = self.off                                                    # the front band begins where the previous back band ended
        start = (self.base + lo + 2 * GUARD + ALIGN - 1) // ALIGN * ALIGN - self.base
        end = start + nbytes                                             # the back band begins at the payload's last byte + 1
        if end + 2 * GUARD > 2 * self.buf.numel():
            raise RuntimeError('GuardArena too small: %d bytes, allocation %d of %s needs %d' %
                               (2 * self.buf.numel(), len(self.allocs), (n, c, h, w), end + 2 * GUARD))
        self.off = end + 2 * GUARD
        self.peak = max(self.peak, self.off)
        self.allocs.append(dict(order=len(self.allocs), offset=start, nbytes=nbytes, shape=(n, c, h, w), front=lo, back=self.off))
        return self.buf[start // 2:end // 2].view(torch.bfloat16).as_strided((n, c, h, w), (h * w * c, 1, w * c, c))

    def payload(self, a):
        """The raw int16 elements of allocation a (an entry of ``allocs``)."""
        return self.buf[a['offset'] // 2:(a['offset'] + a['nbytes']) // 2]

    def reset(self):
        """Refills everything handed out so far (payloads and bands) and forgets the allocations."""
        self.buf[:min(self.buf.numel(), self.peak // 2 + GUARD)].fill_(as_i16(SENTINEL))
        self.allocs = []
        self.off = 0

    def _bands(self):
        for a in self.allocs:
            yield a, 'before', a['front'] // 2, a['offset'] // 2
            yield a, 'behind', (a['offset'] + a['nbytes']) // 2, a['back'] // 2

    def violations(self):
        """One dict per damaged band: allocation (order, shape, offset), side 'before' | 'behind', first / last = bytes between the
        payload's edge and the nearest / farthest damaged element (0 = the element that touches the payload, on either side),
        changed = damaged elements."""
        bands = list(self._bands())
        if not bands:
            return []
        s = as_i16(SENTINEL)
        counts = torch.stack([(self.buf[lo:hi] != s).sum() for _, _, lo, hi in bands]).cpu().tolist()
        out = []
        for (a, side, lo, hi), k in zip(bands, counts):
            if not k:
                continue
            idx = (self.buf[lo:hi] != s).nonzero().flatten()
            i0, i1 = int(idx[0]), int(idx[-1])
            if side == 'behind':
                first, last = 2 * i0, 2 * i1
            else:
                first, last = 2 * (hi - 1 - lo - i1), 2 * (hi - 1 - lo - i0)
            out.append(dict(order=a['order'], shape=a['shape'], offset=a['offset'], side=side, first=first, last=last, changed=int(k)))
        return out

    def unwritten(self):
        """Per allocation, the number of payload elements that still hold SENTINEL."""
        if not self.allocs:
            return []
        s = as_i16(SENTINEL)
        return torch.stack([(self.payload(a) == s).sum() for a in self.allocs]).cpu().tolist()

    def report(self):
        """'' when every band is intact and every payload element was written, else the findings as text."""
        lines = ['band %(side)s allocation %(order)d %(shape)s: %(changed)d elements changed, %(first)d .. %(last)d bytes from the payload' % v
                 for v in self.violations()]
        lines += ['allocation %d %s: %d of %d elements never written' % (a['order'], a['shape'], k, a['nbytes'] // 2)
                  for a, k in zip(self.allocs, self.unwritten()) if k]
        return '\n'.join(lines)


class MeasuringArena(object):
    """Sizes a GuardArena from a shape-only (meta device) walk of an executor: the SUM of all allocations with their bands and rounding
    (an ActivationArena's peak is its largest epoch).  ``buf`` is None as in a measuring ActivationArena."""
    buf, half_bytes = None, None

    def __init__(self):
        self.total, self.n = 0, 0

    def epoch(self):
        pass

    def count(self, nbytes):
        self.total += (int(nbytes) + ALIGN - 1) // ALIGN * ALIGN + 4 * GUARD + ALIGN
        self.n += 1

    def capacity(self):
        return self.total + 4 * GUARD + 2 * ALIGN


class Poisoned(object):
    """The buffer behind a poisoned view: ``refill(fill)`` rewrites the two bands (and nothing of the payload)."""

    def __init__(self, buf, start, numel):
        self.buf, self.start, self.numel = buf, start, numel

    def refill(self, fill):
        self.buf[:self.start].fill_(as_i16(fill))
        self.buf[self.start + self.numel:].fill_(as_i16(fill))

    def bands(self):
        """(elements in front of the payload, elements behind it), raw int16."""
        return self.buf[:self.start], self.buf[self.start + self.numel:]


def poisoned(t, fill):
    """t: a dense channels-last bf16 tensor -> (view, handle): the same values at a 256-byte-aligned address inside a buffer of t's
    device, with the strides of t, >= GUARD elements of `fill` in front of the first element and exactly GUARD behind the last."""
    assert t.dtype == torch.bfloat16 and t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last), (t.dtype, t.shape, t.stride())
    numel = t.numel()
    buf = torch.empty(numel + 2 * GUARD + ALIGN // 2, dtype=torch.int16, device=t.device)
    start = GUARD + ((-(buf.data_ptr() + 2 * GUARD)) % ALIGN) // 2
    buf = buf[:start + numel + GUARD]
    h = Poisoned(buf, start, numel)
    h.refill(fill)
    view = buf[start:start + numel].view(torch.bfloat16).as_strided(tuple(t.shape), t.stride())
    view.copy_(t)
    assert view.data_ptr() % ALIGN == 0 and view.stride() == t.stride()
    return view, h
