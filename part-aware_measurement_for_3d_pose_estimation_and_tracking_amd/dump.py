"""``DumpResults``: the lazy list ``HRNetPose.predict`` returns -- the reference's ``dump_results`` plus the same keypoints still on the
device, in the tracker's input layout."""
import numpy as np
import torch

from .stages import PoseNmsOut


class DumpResults(list):
    """``dump_results`` of the reference (list per view of person dicts) + the same keypoints still on the device.

    The per-person dicts are built LAZILY: ``predict`` only enqueues the device -> host copy of the keypoints; the first access to the
    list's content (indexing, iteration, comparison, printing, copying, pickling ...) waits for that copy and fills the per-view lists
    in place.  Until then nobody can have edited the dicts, so the device copy is trivially the truth."""
    device_det = None        # (views, max_dets, 17, 3) float64 rows (y, x, score) at (view, slot)
    device_n_det = None      # (views,) int32
    device_eff = None        # HRNetPose(box_transform='affine' / 'udp'): (n, 4) float32 effective boxes the call's crops and decode went through
    _poses_host = None       # per view (n, 17, 3) float64 (y, x, score): what ivclabpose._unpack would rebuild from the dicts
    _pending = None          # (pinned host keypoints, event, views, boxes, per-view counts) until the first access
    _nms = None              # HRNetPose(pose_nms=True): (pinned [n_det_out | keep_from], pinned pose_score, views, slots) of the call's filter
    _witness = None

    def attach(self, det, n_det, poses_host):
        self.device_det, self.device_n_det, self._poses_host = det, n_det, poses_host
        self._seal()

    def attach_pending(self, det, n_det, host_kp, event, views, boxes, cnt):
        self.device_det, self.device_n_det = det, n_det
        self._pending = (host_kp, event, views, boxes, cnt)

    def _seal(self):
        # complete witness of what the tracker would read from the dicts (ivclabpose._unpack: 'keypoints' AND 'keypoints_score'):
        # object identities + a hash of all 51 + 17 numbers per person -- an interior edit or a re-scored joint invalidates it
        self._witness = [[(id(it), id(it['keypoints']), id(it['keypoints_score']),
                           hash(tuple(it['keypoints'])), hash(tuple(it['keypoints_score']))) for it in items] for items in list.__iter__(self)]

    _net = None              # the HRNetPose that made this dump and the device side of its call (re-run when a gate gave up)
    _issue = None

    def redo_if_void(self):
        """The forwards of this call are void when a device-side gate of one of them timed out (HRNetPose.check_void): run the call's
        device side again -- the object is on stream events by then -- into the same buffers.  -> True when it did.  The reference's
        predict never returns keypoints it later disowns (/root/reference/src/ivclabpose.py:208-212); neither does this."""
        net = self._net
        if net is None or self._issue is None or self._pending is None or not net.check_void():
            return False
        net.clear_void()
        self._pending = (self._pending[0], self._issue()) + tuple(self._pending[2:])
        return True

    def _host_rows(self):
        """(n, 17, 3) float64 (x, y, score) rows of the call, waiting for the copy predict() enqueued."""
        self._pending[1].synchronize()
        if self.redo_if_void():
            self._pending[1].synchronize()
        return self._pending[0].numpy().astype(np.float64)

    @property
    def poses_host(self):
        if self._poses_host is None and self._pending is not None:
            kp_h, cnt = self._host_rows(), self._pending[4]
            yxs = kp_h[:, :, [1, 0, 2]]
            first = np.concatenate([[0], np.cumsum(cnt)])
            kept = self._kept()
            # (filtered: compacted like the device buffer, so that the record's matched_det indices index it)
            self._poses_host = [yxs[first[v]:first[v + 1]] if kept is None else yxs[[first[v] + s for s in kept[v]]].reshape(-1, 17, 3)
                                for v in range(len(cnt))]
        return self._poses_host

    def _kept(self):
        """Per view the original slots the call's OKS-NMS kept, ascending (None without the filter); valid once _host_rows has waited."""
        if self._nms is None:
            return None
        ki, _, V, S = self._nms
        return PoseNmsOut.kept(ki.numpy() if torch.is_tensor(ki) else ki, V, S)

    @poses_host.setter
    def poses_host(self, value):
        self._poses_host = value

    def _materialise(self):
        if self._pending is None:
            return
        kp_h = self._host_rows()
        _, _, views, boxes, cnt = self._pending
        _ = self.poses_host
        self._pending = None
        self._issue = None                                 # (the call's frames and tables are released with it)
        n = len(views)
        flat = kp_h.reshape(n, 51).tolist()
        score = kp_h[:, :, 2].tolist()
        kept = self._kept()
        if kept is None:
            for i in range(n):
                list.__getitem__(self, views[i]).append(dict(bbox=list(boxes[i]), keypoints=flat[i], keypoints_score=score[i], feature=[]))
        else:                                              # the kept persons only, in slot order, each with its own box and its new score
            first = np.concatenate([[0], np.cumsum(cnt)])
            ps = self._nms[1].numpy()
            for v, slots in enumerate(kept):
                for k, s in enumerate(slots):
                    i = int(first[v]) + s
                    list.__getitem__(self, v).append(dict(bbox=list(boxes[i]), keypoints=flat[i], keypoints_score=score[i], feature=[],
                                                          pose_score=float(ps[v, k])))
            self._nms = (self._nms[0].numpy().copy(), ps.copy()) + tuple(self._nms[2:])       # (the pinned buffers go back to the ring)
        self._seal()

    def device_valid(self):
        """True while the dicts are exactly what predict() returned: never looked at yet, or same objects and every keypoint /
        keypoints_score value untouched (the tracker reads both, /root/reference/src/ivclabpose.py:236-244).  Any edit -- masking or
        re-scoring joints between PersonPoseDetect and PersonTrack_Project3DPose -- sends the call through the host dicts again."""
        if self.device_det is None:
            return False
        if self._pending is not None:
            return True
        if self._witness is None or len(self._witness) != list.__len__(self):
            return False
        for items, wit in zip(list.__iter__(self), self._witness):
            if len(items) != len(wit):
                return False
            for it, (a, b, c, hk, hs) in zip(items, wit):
                k, sc = it.get('keypoints'), it.get('keypoints_score')
                if id(it) != a or id(k) != b or id(sc) != c or len(k) != 51 or len(sc) != 17:
                    return False
                if hash(tuple(k)) != hk or hash(tuple(sc)) != hs:
                    return False
        return True


def _lazy(name):
    base = getattr(list, name)

    def method(self, *a, **k):
        self._materialise()
        return base(self, *a, **k)
    method.__name__ = name
    return method


# every way Python code (and the C helpers that go through the iterator protocol for list SUBCLASSES: list(), json, pickle, copy)
# can see the content first fills it in; __len__ is the number of views and needs no data
for _n in ('__getitem__', '__iter__', '__reversed__', '__contains__', '__eq__', '__ne__', '__lt__', '__le__', '__gt__', '__ge__', '__repr__',
           '__add__', '__iadd__', '__mul__', '__imul__', '__rmul__', '__setitem__', '__delitem__', '__reduce_ex__', 'append', 'extend',
           'insert', 'pop', 'remove', 'index', 'count', 'copy', 'sort', 'reverse', 'clear'):
    setattr(DumpResults, _n, _lazy(_n))
del _n


def _radd(self, other):
    # `[] + dump`: list.__add__ of the LEFT operand is a C fast path that reads a list subclass's items directly (it would see the empty
    # per-view lists); Python tries the right operand's __radd__ first when its type is a subclass of the left one's -- fill in here
    self._materialise()
    return list(other) + list(list.__iter__(self))


DumpResults.__radd__ = _radd
