"""Frame egress for the drivers (reference: src/testmodel.py:76-80, one cv2.imwrite per camera per frame on the main
thread): ``FrameWriter`` is ``ingest.FrameLoader`` turned round.  The annotated BGR frames stay on the device; ``submit`` issues ONE
pam_jpeg_forward per frame set -- colour conversion, downsampling, forward DCT and quantisation -- and the copy of the int16 coefficients
into a pinned staging buffer on a copy stream of its own, behind an event on the consumer's stream, and returns.  Worker threads wait
for the slot's event, run the Huffman pass (pam_jpeg_encode, no GIL) and write the file.  The ring has ``depth`` slots: ``submit`` blocks
while all are in flight, ``close`` drains them.

The default is quality 75 at 4:2:0, Pillow's defaults, and the arithmetic is libjpeg's: the files are byte for byte what
``Image.fromarray(rgb).save(path)`` writes from the same pixels."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SAMPLINGS = {'444': (1, 1), '422': (2, 1), '420': (2, 2)}


def coef_words(width, height, hs, vs):
    """int16 words of one image's coefficient buffer (PamJpegInfo's layout, three components)."""
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return 64 * mw * mh * (hs * vs + 2)


class _Slot(object):
    def __init__(self):
        self.pinned = self.device = self.event = None
        self.frames = ()
        self.pending = 0
        self.out = {}


class FrameWriter(object):
    """Writes frame sets of CUDA BGR uint8 (H, W, 3) tensors as JPEG files.  ``submit(frame_id, frames, paths)`` returns as soon as the
    work is issued; the frames must not be written to until ``close()`` or until ``depth`` later submits have returned.  Counters:
    ``submitted`` / ``written`` (files), ``bytes_written``, ``waits`` (submits that found the ring full)."""

    def __init__(self, device, quality=75, sampling='420', workers=4, depth=4):
        import torch
        from . import _lib
        self.torch, self.L, self.lib = torch, _lib, _lib.load()
        self.device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        self.quality, self.hs, self.vs = int(quality), SAMPLINGS[sampling][0], SAMPLINGS[sampling][1]
        tables = np.zeros((2, 64), dtype=np.uint16)
        if self.lib.pam_jpeg_quality_tables(self.quality, tables.ctypes.data) != 0:
            raise ValueError('quality %r is outside 1 .. 100' % (quality,))
        self.quant = torch.from_numpy(tables[[0, 1, 1]].copy()).to(self.device)          # per component, as pam_jpeg_forward reads them
        self.copy_stream = torch.cuda.Stream(self.device)
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.slots = [_Slot() for _ in range(max(1, depth))]
        self._free = list(range(len(self.slots)))
        self._cv = threading.Condition()
        self._error = None
        self.submitted = self.written = self.bytes_written = self.waits = 0

    def _take_slot(self):
        with self._cv:
            if not self._free:
                self.waits += 1
            while not self._free and self._error is None:
                self._cv.wait()
            if self._error is not None:
                raise self._error
            return self.slots[self._free.pop(0)]

    def _encode(self, slot, k, path, width, height, first, words):
        """Worker thread: one image of a slot -> its file."""
        try:
            slot.event.synchronize()
            p = self.L.PamJpegEncodeParams(width=width, height=height, h_samp=self.hs, v_samp=self.vs, quality=self.quality)
            cap = C.c_size_t(0)
            self.lib.pam_jpeg_encode_bound(width, height, self.hs, self.vs, C.byref(cap))
            out = slot.out.get(k)
            if out is None or out.size < cap.value:
                out = slot.out[k] = np.empty(cap.value, dtype=np.uint8)
            n = C.c_size_t(0)
            coef = slot.pinned.numpy()[first:first + words]
            rc = self.lib.pam_jpeg_encode(coef.ctypes.data, words, C.byref(p), out.ctypes.data, out.size, C.byref(n))
            if rc != 0:
                raise self.L.PamError('pam_jpeg_encode failed (%d) for %s' % (rc, path))
            with open(path, 'wb') as f:
                f.write(memoryview(out)[:n.value])
            err = None
        except BaseException as e:                       # handed to the next submit / close
            err, n = e, C.c_size_t(0)
        with self._cv:
            if err is not None and self._error is None:
                self._error = err
            if err is None:
                self.written += 1
                self.bytes_written += n.value
            slot.pending -= 1
            if slot.pending == 0:
                slot.frames = ()
                self._free.append(self.slots.index(slot))
            self._cv.notify_all()

    def submit(self, frame_id, frames, paths):
        """frames: CUDA uint8 (H, W, 3) BGR tensors, contiguous; paths: one file name each.  More than 32 frames take a launch per 32."""
        torch = self.torch
        if len(frames) != len(paths):
            raise ValueError('%d frames, %d paths' % (len(frames), len(paths)))
        if not frames:
            return
        for f in frames:
            if not (f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
                raise ValueError('FrameWriter takes contiguous uint8 (H, W, 3) CUDA tensors')
        slot = self._take_slot()
        sizes = [(int(f.shape[1]), int(f.shape[0])) for f in frames]
        words = [coef_words(w, h, self.hs, self.vs) for w, h in sizes]
        firsts = [int(x) for x in np.cumsum([0] + words[:-1])]
        total = sum(words)
        if slot.pinned is None or slot.pinned.numel() < total:
            slot.pinned = torch.empty(total, dtype=torch.int16).pin_memory()
            slot.device = torch.empty(total, dtype=torch.int16, device=self.device)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))              # the frames are complete on the consumer's stream
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            for lo in range(0, len(frames), self.L.JPEG_MAX_IMAGES):
                part = range(lo, min(lo + self.L.JPEG_MAX_IMAGES, len(frames)))
                images = (self.L.PamJpegFwdImage * len(part))()
                for im, k in zip(images, part):
                    im.dev_bgr, im.dev_quant = frames[k].data_ptr(), self.quant.data_ptr()
                    im.dev_coef = slot.device.data_ptr() + 2 * firsts[k]
                    im.width, im.height, im.h_samp, im.v_samp = sizes[k][0], sizes[k][1], self.hs, self.vs
                rc = self.lib.pam_jpeg_forward(self.copy_stream.cuda_stream, len(part), images)
                if rc != 0:
                    with self._cv:
                        self._free.append(self.slots.index(slot))
                    raise self.L.PamError('pam_jpeg_forward failed (%d)' % rc)
            slot.pinned[:total].copy_(slot.device[:total], non_blocking=True)
            slot.event = torch.cuda.Event()
            slot.event.record(self.copy_stream)
        slot.frames = tuple(frames)                      # alive until the kernel that reads them has run
        slot.pending = len(frames)
        self.submitted += len(frames)
        for k, path in enumerate(paths):
            self.pool.submit(self._encode, slot, k, path, sizes[k][0], sizes[k][1], firsts[k], words[k])

    def close(self):
        """Waits for every file to be written, stops the workers and raises what a worker failed with."""
        with self._cv:
            while len(self._free) < len(self.slots):
                self._cv.wait()
        self.pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error
