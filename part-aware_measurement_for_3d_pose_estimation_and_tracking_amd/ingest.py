"""Frame ingest for the drivers (reference: src/dataset.py:36-45, one cv2.imread per camera per frame on the
main thread).  With the per-frame compute at a few milliseconds, decoding C JPEGs per frame is the bottleneck of a real run,
so frames are decoded by a pool of worker threads a few frames ahead (PIL/libjpeg-turbo releases the GIL), written as BGR
uint8 HxWx3 -- cv2.imread's layout -- into pinned host buffers and, when a device is given, uploaded on a dedicated copy
stream; the consumer only waits on an event.  Frame order is preserved.

``device_decode=True`` (with a device) moves the parallel half of a baseline JPEG's decode onto the device: a worker reads the file and runs
the Huffman pass alone (pam_jpeg_entropy, no GIL) into a pinned int16 buffer of quantised coefficients; the main thread uploads them and
issues ONE pam_jpeg_reconstruct per frame set on the copy stream, which writes the same BGR uint8 (H, W, 3) tensors.  A file the entropy
pass does not take (progressive, CMYK, a PNG, ...) goes through the Pillow path, for that camera and that frame alone."""
import os
import threading
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np


JPEG_HEAD = 256        # int16 words in front of the coefficients in a staging buffer: 3 x 64 quantisation words, padded to 512 bytes


def decode_bgr(path, out=None):
    """One image file -> BGR uint8 (H, W, 3), optionally into a preallocated array."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    if out is None:
        return np.ascontiguousarray(rgb[:, :, ::-1])
    out[...] = rgb[:, :, ::-1]
    return out


def timestamp_of(dataset_name, first_file):
    base = os.path.basename(first_file)
    return int(base.split('_')[-1].split('.')[0]) if dataset_name == 'Panoptic' else base.split('.')[0]


class FrameLoader(object):
    """Iterates (frame_index, imagelist, timestamp) over ``frames`` (list over frames of list over cameras of file names),
    ``depth`` frames ahead on ``workers`` threads.  imagelist entries are NumPy BGR arrays, or CUDA uint8 tensors when
    ``device`` is given (pinned staging + async copy on a side stream)."""

    def __init__(self, dataset_name, frames, indices=None, workers=8, depth=4, device=None, device_decode=False):
        self.name, self.frames = dataset_name, frames
        self.indices = list(range(len(frames))) if indices is None else list(indices)
        self.depth = max(1, depth)
        self.pool = ThreadPoolExecutor(max_workers=max(1, workers))
        self.device = device
        self._pinned = {}
        self._slot_events = {}
        self._lock = threading.Lock()
        self.device_decode = bool(device_decode) and device is not None
        self.device_decoded = 0                          # files rebuilt on the device / files that took the Pillow path instead
        self.fallbacks = 0
        if device is not None:
            import torch
            self.torch = torch
            self.copy_stream = torch.cuda.Stream(device)
        if self.device_decode:
            from . import _lib
            self._jpeg = _lib
            self._jpeg_lib = _lib.load()

    def _pinned_for(self, slot, cam, shape):
        key = (slot, cam, tuple(shape))
        with self._lock:
            buf = self._pinned.get(key)
            if buf is None:
                buf = self._pinned[key] = self.torch.empty(tuple(shape), dtype=self.torch.uint8).pin_memory()
        return buf

    def _decode_pinned(self, path, slot, cam):
        """Worker thread: one image file -> BGR uint8 straight into the slot's pinned staging buffer (round 5: the main thread used to
        copy every decoded image into pinned memory itself, 12 MB per Shelf frame set, which capped the device path at ~125 frame sets/s
        on the GPU hosts against 245 for the decode alone)."""
        from PIL import Image
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'))
        pin = self._pinned_for(slot, cam, rgb.shape)
        np.copyto(pin.numpy(), rgb[:, :, ::-1])
        return pin

    def _coef_pinned_for(self, slot, cam, words):
        """The slot's pinned int16 staging buffer for one camera's coefficients: grown, never shrunk (files of one camera differ in
        nothing but content as a rule, so this allocates once)."""
        key = (slot, cam, 'coef')
        with self._lock:
            buf = self._pinned.get(key)
            if buf is None or buf.numel() < words:
                buf = self._pinned[key] = self.torch.empty(words, dtype=self.torch.int16).pin_memory()
        return buf

    def _entropy_pinned(self, path, slot, cam):
        """Worker thread: one file -> (info, pinned int16 [JPEG_HEAD words: the quantisation tables | coef_words coefficients]); the
        Huffman pass is the only decoding done on the host.  (None, BGR pinned buffer) through Pillow for a file the pass does not take."""
        L, lib = self._jpeg, self._jpeg_lib
        with open(path, 'rb') as f:
            data = f.read()
        info = L.PamJpegInfo()
        if lib.pam_jpeg_probe(data, len(data), info) == 0 and not info.unsupported:
            words = int(info.coef_words)
            pin = self._coef_pinned_for(slot, cam, JPEG_HEAD + words)
            host = pin.numpy()
            host[:192].view(np.uint16)[:] = np.ctypeslib.as_array(info.quant).reshape(-1)
            if lib.pam_jpeg_entropy(data, len(data), info, host[JPEG_HEAD:].ctypes.data, words) == 0:
                return info, pin[:JPEG_HEAD + words]
        return None, self._decode_pinned(path, slot, cam)

    def _reconstruct(self, jobs):
        """Main thread, copy stream current: the coefficient uploads and one launch pair per (at most 32) images of the frame set.
        jobs: (info, pinned) per device-decoded camera -> the BGR tensors in the same order."""
        torch, L = self.torch, self._jpeg
        outs = []
        for lo in range(0, len(jobs), L.JPEG_MAX_IMAGES):
            part = jobs[lo:lo + L.JPEG_MAX_IMAGES]
            images = (L.PamJpegImage * len(part))()
            keep = []
            for im, (info, pin) in zip(images, part):
                coef = pin.to(self.device, non_blocking=True)            # these two live and die on the copy stream
                planes = torch.empty(int(info.coef_words), dtype=torch.uint8, device=self.device)
                out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=self.device)
                im.dev_quant, im.dev_coef = coef.data_ptr(), coef.data_ptr() + 2 * JPEG_HEAD
                im.dev_planes, im.dev_out = planes.data_ptr(), out.data_ptr()
                im.width, im.height, im.n_comp, im.h_samp, im.v_samp = info.width, info.height, info.n_comp, info.h_samp[0], info.v_samp[0]
                keep.append((coef, planes))
                outs.append(out)
            rc = self._jpeg_lib.pam_jpeg_reconstruct(self.copy_stream.cuda_stream, len(part), images)
            if rc != 0:
                raise L.PamError('pam_jpeg_reconstruct failed (%d)' % rc)
        return outs

    def _submit(self, k):
        files = self.frames[self.indices[k]]
        if self.device is None:
            return [self.pool.submit(decode_bgr, f) for f in files]
        slot = k % (self.depth + 1)
        prev = self._slot_events.get(slot)
        if prev is not None:
            prev.synchronize()                           # the async copy out of this pinned slot (depth + 1 frames ago) has finished: safe to overwrite
        work = self._entropy_pinned if self.device_decode else self._decode_pinned
        return [self.pool.submit(work, f, slot, c) for c, f in enumerate(files)]

    def __iter__(self):
        pending = deque()
        nxt = 0
        n = len(self.indices)
        while nxt < n and len(pending) < self.depth:
            pending.append((nxt, self._submit(nxt))); nxt += 1
        while pending:
            k, futs = pending.popleft()
            imgs = [f.result() for f in futs]
            ts = timestamp_of(self.name, self.frames[self.indices[k]][0])
            if self.device is None:
                if nxt < n:
                    pending.append((nxt, self._submit(nxt))); nxt += 1
                yield self.indices[k], imgs, ts
                continue
            torch = self.torch
            slot = k % (self.depth + 1)
            out = []
            consumer = torch.cuda.current_stream(self.device)
            with torch.cuda.stream(self.copy_stream):
                if self.device_decode:
                    jobs = [r for r in imgs if r[0] is not None]
                    rebuilt = iter(self._reconstruct(jobs)) if jobs else iter(())
                    self.device_decoded += len(jobs)
                    self.fallbacks += len(imgs) - len(jobs)
                for pin in imgs:
                    if self.device_decode:
                        t = next(rebuilt) if pin[0] is not None else pin[1].to(self.device, non_blocking=True)
                    else:
                        t = pin.to(self.device, non_blocking=True)
                    # the block belongs to copy_stream's pool; the consumer reads it on ITS stream after only a wait_event, so tell
                    # the caching allocator -- otherwise the block can be handed to the next frame's copy while kernels still read it
                    t.record_stream(consumer)
                    out.append(t)
                ev = torch.cuda.Event(); ev.record(self.copy_stream)
            self._slot_events[slot] = ev
            consumer.wait_event(ev)
            if nxt < n:                                  # frame k + depth takes the slot of frame k - 1, whose copy was issued a step ago
                pending.append((nxt, self._submit(nxt))); nxt += 1
            yield self.indices[k], out, ts

    def close(self):
        self.pool.shutdown(wait=False)
