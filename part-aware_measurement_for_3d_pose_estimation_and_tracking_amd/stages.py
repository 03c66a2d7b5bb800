"""The optional stages' host side, written once for the reference-shaped facade (ivclabpose -> HRNetPose.predict -> IterativeTracker,
testmodel) and for FramePipeline: plain functions and small classes that own buffers.  None of them ever holds a pipeline, a tracker
or a network -- a stage object holds tensors and at most a _lib.Handle, so whoever owns one is still freed by reference count alone
(tests/test_gpu_lifetimes.py)."""
import numpy as np

from . import _lib


class OneEuro(object):
    """The One-Euro output filter of one handle (pam_one_euro; the rules: include/pam.h): the configuration on the handle, the device
    buffers (``dev`` = pose, meta) and their pinned twins (``host``); ``fetched``: whether the last step sent its rows to the host."""
    fetched = False

    def __init__(self, handle, cfg):
        handle.set_one_euro(cfg)
        self.handle, self.dev, self.host = handle, handle.one_euro_buffers(), handle.one_euro_buffers(pinned=True)

    def step(self, stream, frame_id, fetch=True):
        """The filter launch behind the frame kernel that was just issued on ``stream`` (the torch stream that is current there), and
        with ``fetch`` its two buffers on their way to pinned host memory, in front of the record's copy.  The launch is idempotent
        per frame, so it may follow every attempt of a retried frame."""
        pose, meta = self.dev
        self.handle.one_euro(stream, frame_id, pose, meta)
        self.fetched = bool(fetch)
        if fetch:
            self.host[0].copy_(pose, non_blocking=True); self.host[1].copy_(meta, non_blocking=True)

    def rows(self, rec):
        """The fetched rows, decoded (Handle.decode_one_euro), once they are seen to follow the decoded record ``rec``: same count, same
        ids in the same order (both follow the state's list)."""
        f = _lib.Handle.decode_one_euro(np.asarray(self.host[0]), np.asarray(self.host[1]), 0)
        if f['n_tracks'] != rec['n_tracks'] or f['ids'].tolist() != [t['track_id'] for t in rec['tracks']]:
            raise _lib.PamError('the One-Euro rows do not follow the record (ids %s)' % (f['ids'].tolist(),))
        return f

    def add_to(self, rec):
        f = self.rows(rec)
        rec['pose3d_filtered'] = f['pose']
        rec['filter_meta'] = dict(n_fresh=f['n_fresh'], ids=f['ids'], fresh=f['fresh'], samples=f['samples'])


class CropTableInfo(object):
    """The info words of the frame's device-built crop table (pam_crop_table) on their way into the record: ``info`` is the table's
    device tensor (None: the frame had no such table), ``fetch`` sends it behind the record's copy."""
    info, fetched = None, False

    def __init__(self):
        import torch
        self.host = torch.zeros(4, dtype=torch.int32).pin_memory()

    def fetch(self):
        self.fetched = self.info is not None
        if self.fetched:
            self.host.copy_(self.info, non_blocking=True)

    def add_to(self, rec):
        w = self.host.numpy()
        rec['crop_table'] = dict(rows=int(w[0]), wanted=int(w[1]), status=int(w[2]))


class PoseNmsOut(object):
    """What pam_pose_nms writes for ``views`` views of ``slots`` slots: ``words`` = [n_det | keep_from] int32 (``n_det`` (views,) and
    ``keep_from`` (views, slots) are views of it), ``pose_score`` (views, slots) float64, and a pinned twin of the words (``host``) that
    travels behind the record's copy.  ``live``: this frame's step filled the buffers; ``fetched``: the last fetch sent them."""
    live, fetched = False, False

    def __init__(self, views, slots, device):
        import torch
        self.views, self.slots = views, slots
        self.words = torch.zeros(views + views * slots, dtype=torch.int32, device=device)
        self.n_det, self.keep_from = self.words[:views], self.words[views:].view(views, slots)
        self.keep_from.fill_(-1)
        self.pose_score = torch.zeros((views, slots), dtype=torch.float64, device=device)
        self.host = torch.zeros(views + views * slots, dtype=torch.int32).pin_memory()

    def nothing_kept(self):
        """A frame without crops: nothing decoded, nothing kept."""
        self.n_det.zero_(); self.keep_from.fill_(-1)
        self.live = True

    def fetch(self):
        self.fetched = self.live
        if self.fetched:
            self.host.copy_(self.words, non_blocking=True)

    @staticmethod
    def kept(words, views, slots):
        """Host words [n_det | keep_from] -> per view the original slots the filter kept, ascending."""
        return [[int(s) for s in words[views + v * slots:views + v * slots + int(words[v])]] for v in range(views)]

    def add_to(self, rec):
        a, nv = self.host.numpy(), self.views
        rec['pose_nms'] = dict(n_det=[int(x) for x in a[:nv]], keep_from=a[nv:].reshape(nv, self.slots).copy())


def after_decode(stream, det, n_det, rows, nms=None, nms_fetch=(), lens=None, max_dets=None):
    """What follows the last decode into ``det`` ((V, det_slots, 17, 3) float64, counts n_det), on ``stream``: the OKS-NMS first -- its
    areas come from raw-image boxes -- then the lens step on the rows below the filter's counts.  rows = (view_of, slot_of, boxes) of the
    decode; nms = (n_det_out, keep_from, pose_score, _lib.pose_nms' keywords) or None; nms_fetch: (pinned, device) pairs copied right
    behind the filter; lens = (table, info, views or None) or None.  -> the counts the tracker takes.  With both off nothing is issued."""
    if nms is not None:
        _lib.pose_nms(stream, det, n_det, rows[0], rows[1], rows[2], nms[0], nms[1], nms[2], max_dets=max_dets, **nms[3])
        n_det = nms[0]
        for host, dev in nms_fetch:
            host.copy_(dev, non_blocking=True)
    if lens is not None:
        _lib.undistort_keypoints(stream, det, n_det, lens[0], lens[1], max_dets=max_dets, views=lens[2])
    return n_det
