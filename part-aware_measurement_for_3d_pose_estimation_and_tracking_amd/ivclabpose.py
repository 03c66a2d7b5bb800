"""Drop-in façade: the reference's ``ivclabpose`` / ``Camera`` surface (/root/reference/src/ivclabpose.py:35-287)
with the matching / triangulation / tracking path running on MI355X through libpam_hip.so.

Kept: constructor signature and config attribute names, ``GetCameraParameters``, ``PersonDetect``,
``PersonPoseDetect``, ``PersonTrack_Project3DPose`` and its 9-tuple.  The YOLOv3 detector is outside the path
(SURVEY 8f rank 1): with DETECT_MODELS.NONE person boxes must be supplied by the caller."""
import numpy as np
import torch

from .tracker import IterativeTracker, NUM_JOINTS


class _Args(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _cfg(obj, key):
    return obj[key] if isinstance(obj, dict) else getattr(obj, key)


def _opt(block, key, default=None):
    """An optional key of a config block (a dict or an attribute bag; the block itself may be missing)."""
    if block is None:
        return default
    return block.get(key, default) if isinstance(block, dict) else getattr(block, key, default)


# DETECT_MODELS.<KEY>.NAME values that build a person detector: 'YOLOv3' (the reference's; yolov3.YOLOv3) and 'YOLOv4' (yolov4.YOLOv4)
DETECTOR_NAMES = ('YOLOv3', 'YOLOv4')

# The optional keys of a POSE_MODELS.HRPOSE block that set a decode option of HRNetPose (none of them in the reference's YAMLs):
# (key, attribute, conversion, set when the key is absent).  Applied in this order: the property setters refuse combinations
# (HRNetPose._decode_option), so which error a bad YAML gets depends on it.
#   SOFT_ARGMAX_BETA > 0: the soft-arg-max of pam_head_decode_soft with that inverse temperature in place of the hard arg-max (parity
#   mode; 0 leaves it off)
#   SHIFT_HEATMAP / POST_PROCESS / FLIP_TEST: the official names (TEST.* of the HRNet and Simple Baselines configs), off when absent: the
#   protocol the published checkpoints were evaluated under
#   BLUR_KERNEL / DARK: the DARK decode (Zhang et al., CVPR 2020); BLUR_KERNEL absent: 17 for maps of 96 rows or more, otherwise 11
#   OKS_NMS / OKS_THRE / IN_VIS_THRE (TEST.OKS_THRE / TEST.IN_VIS_THRE; OKS_NMS switches the step on): every pose rescored and each
#   view's duplicates removed on the device before the tracker (pam_pose_nms)
POSE_OPTIONS = (('SOFT_ARGMAX_BETA', 'soft_beta', lambda v: float(v) or None, False), ('SHIFT_HEATMAP', 'shift_heatmap', bool, False),
                ('POST_PROCESS', 'post_process', bool, True), ('BLUR_KERNEL', 'blur_kernel', int, False), ('DARK', 'dark', bool, True),
                ('FLIP_TEST', 'flip_test', bool, True), ('OKS_NMS', 'pose_nms', bool, True), ('OKS_THRE', 'oks_thre', float, False),
                ('IN_VIS_THRE', 'in_vis_thre', float, False))


def one_euro_from_matcher(m):
    """The optional block ONE_EURO {FREQ, MINCUTOFF, BETA, DCUTOFF} of a PERSON_MATCHERS.ITERATIVE block (not in the reference's YAMLs,
    whose filters are built with fixed values and never called) -> the dict IterativeTracker(one_euro=) takes, keys in lower case, a
    missing key left to its default (_lib.ONE_EURO_3D); None when the block is absent."""
    blk = _opt(m, 'ONE_EURO')
    if blk is None or blk is False:
        return None
    return {} if blk is True else {str(k).lower(): v for k, v in dict(blk).items()}


def box_transform_options(p):
    """The optional keys BOX_TRANSFORM / BOX_SCALE of a POSE_MODELS.HRPOSE block (not in the reference's YAMLs) -> (box_transform,
    box_scale) as HRNetPose takes them; absent keys give ('stretch', 1.25), a BOX_TRANSFORM other than 'stretch' / 'affine' / 'udp' or a
    BOX_SCALE that is not > 0 is a ValueError (_lib.check_box_transform)."""
    from . import _lib
    return _lib.check_box_transform(_opt(p, 'BOX_TRANSFORM'), _opt(p, 'BOX_SCALE'))


class Camera(object):
    """Calibrated view: P, K, RT (float32), F[other] (float32), RK_INV (float32), position (float64).
    distCoef (not in the reference, whose lens methods are identity stubs): (k1, k2, p1, p2, k3) of the camera's lens, OpenCV / Panoptic
    order; None or all zeros = an ideal pin-hole.  P, F and RK_INV describe the IDEAL camera either way: points of the raw image go
    through ``undistort_points`` before they meet them (on the product path the device does that, pam_undistort_keypoints)."""

    def __init__(self, cid, P, K, RT, F, w=640, h=480, distCoef=None):
        self.cid, self.P, self.K, self.RT, self.F, self.w, self.h = cid, P, K, RT, F, w, h
        self.RK_INV = np.linalg.inv(RT[:, :3]) @ np.linalg.inv(K)
        self.position = np.linalg.inv(np.vstack([RT, [0, 0, 0, 1]]))[:3, 3]
        self.distCoef, self.lens = None, None
        if distCoef is not None:
            from . import _lib
            self.distCoef = np.asarray(distCoef, dtype=np.float64).reshape(5)
            table = _lib.lens_table(np.asarray(K)[None], self.distCoef[None])
            self.lens = table[0] if table is not None else None            # the row of the device table, None for a pin-hole

    def undistort(self, im):
        return im                    # images are not resampled: the keypoints are moved instead

    def _rows_xy(self, points2d, fn):
        pts = np.asarray(points2d, dtype=np.float64)
        if self.lens is None or pts.size == 0:
            return points2d
        out = pts.copy()
        res = fn(self.lens, pts[..., 0], pts[..., 1])
        out[..., 0], out[..., 1] = res[0], res[1]
        return out

    def undistort_points(self, points2d):
        """rows (x, y[, w]) of the raw image -> the same rows in the ideal pin-hole image (further columns untouched).  8 Newton steps in
        float64 (lens.inverse: the device's expressions); a point the model cannot invert keeps its coordinates."""
        from . import lens
        return self._rows_xy(points2d, lens.undistort_uw)

    def distort_points(self, points2d):
        """rows (x, y[, w]) of the ideal pin-hole image -> the same rows in the raw image (the closed-form forward model)."""
        from . import lens
        return self._rows_xy(points2d, lens.distort_uw)

    def projectPoints_parallel(self, points3d):
        """(n,17,3) -> (n,17,2) in (y, x); host NumPy convenience (the device does this inside k_frame)."""
        n, j = points3d.shape[0], points3d.shape[1]
        hom = np.concatenate([points3d, np.ones((n, j, 1))], axis=2).reshape(-1, 4)
        h = (self.P @ hom.T).T
        return (h[:, :2] / h[:, 2:3])[:, ::-1].reshape(n, j, 2)

    def projectPoints_undist(self, points3d):
        """(n, 3) -> (n, 2) in (y, x), no distortion"""
        return self.projectPoints_parallel(np.asarray(points3d, dtype=np.float64)[None])[0]

    def projectPoints(self, points3d):
        """(n, 3) -> (n, 2) in (y, x) with the lens considered: where the points lie in the raw image"""
        yx = self.projectPoints_undist(points3d)
        if self.lens is None:
            return yx
        return self.distort_points(yx[:, ::-1])[:, ::-1]


def fundamental_matrices(K, RT):
    """(C,C,3,3) float32, F[a][b] with x_a^T F x_b = 0, evaluated in float32 torch CPU algebra in the reference's
    operation order (ivclabpose.py:166-177) so both stacks hand the same bits to the device."""
    C = len(K)
    Kt = [torch.tensor(K[i]) for i in range(C)]
    R = [torch.tensor(RT[i][:, :3]) for i in range(C)]
    T = [torch.tensor(RT[i][:, 3]) for i in range(C)]
    Kinv_t = [torch.inverse(k).t() for k in Kt]
    F = torch.zeros(C, C, 3, 3)
    for a in range(C):
        for b in range(C):
            e = Kt[b] @ R[b] @ R[a].t() @ (T[a] - R[a] @ R[b].t() @ T[b])
            ex = torch.tensor([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
            F[a, b] += Kinv_t[a] @ (R[a] @ R[b].t()) @ Kt[b].t() @ ex
            if F[a, b].sum() == 0:
                F[a, b] += 1e-12
    return F.numpy()


class ivclabpose(object):
    def __init__(self, person_detector=None, pose_detector=None, person_matcher=None, conf_threshold=0.4,
                 max_dets=16, max_tracks=32, device=0, autotune=False):
        """autotune (not in the reference): let the pose network pick the fastest of its executor configurations per crop count on this
        device (HRNetPose(autotune=True)); off by default because two batchings of the same crops may then differ in the last bf16 bits."""
        self.person_detector = person_detector if _cfg(person_detector, 'NAME') != '' else None
        self.pose_detector = pose_detector
        self.person_matcher = person_matcher
        self.conf_threshold = conf_threshold
        self.device = device
        self.cameras = None
        self.pose_model = None
        self.pts3d_filtered = None
        # optional keys of the detector's block (not in the reference's YAMLs; absent = the detector on every frame): DETECT_EVERY = K runs
        # the detector on every K-th frame and takes the boxes of the frames in between from the tracks (PersonBoxesFromTracks);
        # TRACK_BOX_GROW / TRACK_BOX_PAD = that box rule's growth and pad in pixels
        from . import _lib
        self.detect_every = int(_opt(person_detector, 'DETECT_EVERY') or 1)
        self.track_box_rule = dict(_lib.TRACK_BOX_RULE)
        for key, name in (('TRACK_BOX_GROW', 'grow'), ('TRACK_BOX_PAD', 'pad_px')):
            if _opt(person_detector, key) is not None:
                self.track_box_rule[name] = float(_opt(person_detector, key))
        self.frames_scheduled = 0
        if self.person_detector is None:
            print("Person Detector : Close.")
        elif _cfg(self.person_detector, 'NAME') in DETECTOR_NAMES:                  # ivclabpose.py:116-120
            import os
            d = self.person_detector
            v4 = _cfg(d, 'NAME') == 'YOLOv4'        # not in the reference: yolov4.YOLOv4 (YOLOv4 / YOLOv4-tiny and the three v3 networks), same keys
            if v4:
                from .yolov4 import YOLOv4 as YOLOv3
            else:
                from .yolov3 import YOLOv3
            cfg, weight, names = _cfg(d, 'CFG'), _cfg(d, 'WEIGHT'), _cfg(d, 'CLASS_NAMES')
            # the reference's cfg / weight / names files are not distributed with it: a missing cfg or names file means
            # the standard YOLOv3-416 COCO layout (person = class 0), missing weights mean a seeded random network.
            # ARCH (optional key, not in the reference): 'yolov3' | 'yolov3-tiny' | 'yolov3-spp', the standard network built when the cfg file is missing
            # (NAME 'YOLOv4': also 'yolov4' | 'yolov4-tiny', default 'yolov4')
            arch = _opt(d, 'ARCH') or ('yolov4' if v4 else 'yolov3')
            self.bbox_detector = YOLOv3(cfg if cfg and os.path.exists(cfg) else None,
                                        weight if weight and os.path.exists(weight) else None,
                                        names if names and os.path.exists(names) else None,
                                        score_thresh=_cfg(d, 'SCORE_THRESH'), nms_thresh=_cfg(d, 'NMS_THRESH'),
                                        use_cuda=True, device=device, max_det=max_dets,   # best max_dets boxes per view: the tracker's capacity
                                        arch=arch)
            print("Person Detector : ", _cfg(d, 'NAME'), '(weights: %s)' % self.bbox_detector.weights)
        else:
            raise NotImplementedError('person detector %r' % _cfg(self.person_detector, 'NAME'))
        if self.pose_detector is None:
            print("Pose Detector : Close.")
        elif _cfg(self.pose_detector, 'NAME') == 'HRPose':
            from .hrnet import HRNetPose
            # ivclabpose.py:107-111: gpu_args = every visible GPU.  One process drives ONE of them (`device`); several GPUs = several
            # ranks of a torch.distributed job, and HRNetPose.predict shards each call's crops over them (see HRNetPose.__init__).
            gpu_args = _Args(gpus=list(range(torch.cuda.device_count())), device=torch.device('cuda:%d' % device))
            # optional keys BOX_TRANSFORM ('stretch' | 'affine' | 'udp') / BOX_SCALE: the crop geometry; 'affine' = the published checkpoints' own
            # (_box2cs + get_affine_transform: aspect fix about the centre, x BOX_SCALE 1.25, zero border; decode and OKS-NMS through the
            # same effective box); 'udp' = the UDP checkpoints' (ViTPose, HRNet "+UDP": the same box on align-corners grids, decode always
            # pam_head_decode_udp; with POST_PROCESS or SOFT_ARGMAX_BETA a ValueError).  Absent: the raw box stretched to the input, as
            # before.  Another value is refused (ValueError).
            box_transform, box_scale = box_transform_options(self.pose_detector)
            self.pose_model = HRNetPose(_cfg(self.pose_detector, 'C'), _cfg(self.pose_detector, 'NUM_JOINTS'),
                                        _cfg(self.pose_detector, 'CHECKPOINT_FILE'),
                                        model_name=_cfg(self.pose_detector, 'MODEL_NAME'),
                                        resolution=tuple(_cfg(self.pose_detector, 'RESOLUTION')), hrpose_args=gpu_args,
                                        device=device, max_dets=max_dets,
                                        shard_crops=torch.distributed.is_available() and torch.distributed.is_initialized(),
                                        autotune=autotune, box_transform=box_transform, box_scale=box_scale)
            for key, attr, conv, when_absent in POSE_OPTIONS:
                value = _opt(self.pose_detector, key)
                if value is not None or when_absent:
                    setattr(self.pose_model, attr, conv(value))
            print("Pose Detector : ", _cfg(self.pose_detector, 'NAME'))
        if self.person_matcher is None:
            print("Person Matcher : Close.")
            self.tracker = None
        elif _cfg(self.person_matcher, 'NAME') == 'Iterative':
            m = self.person_matcher
            a = _Args(conf_threshold=conf_threshold)
            for dst, src in (('epi_threshold', 'EPI_THRESHOLD'), ('init_threshold', 'INIT_THRESHOLD'),
                             ('joint_threshold', 'JOINT_THRESHOLD'), ('num_joints', 'NUM_JOINTS'),
                             ('init_method', 'INIT_METHOD'), ('n_init', 'N_INIT'), ('max_age', 'MAX_AGE'),
                             ('w2d', 'W2D'), ('alpha2d', 'ALPHA2D'), ('w3d', 'W3D'), ('alpha3d', 'ALPHA3D'),
                             ('lambda_a', 'LAMBDA_A'), ('lambda_t', 'LAMBDA_T'), ('sigma', 'SIGMA'),
                             ('arm_sigma', 'ARM_SIGMA')):
                a[dst] = _cfg(m, src)
            # optional block ONE_EURO: the tracks' 3D output also through One-Euro filters on the device (pam_one_euro) -> pts3d_filtered
            oe = one_euro_from_matcher(m)
            self.tracker = IterativeTracker(a, max_dets=max_dets, max_tracks=max_tracks, device=device,
                                            one_euro=oe if oe is None else dict(oe))
            if self.pose_model is not None:
                self.tracker.set_input_guard(self.pose_model)      # keypoints of a forward whose gate timed out never reach the tracker state
            print("Person Matcher : ", _cfg(m, 'NAME'))

    # -- a18 ----------------------------------------------------------------------------------------------------------
    def GetCameraParameters(self, camera_parameter, im_width, im_height, F=None):
        P = np.asarray(camera_parameter['P']).astype(np.float32)
        K = np.asarray(camera_parameter['K']).astype(np.float32)
        RT = np.asarray(camera_parameter['RT']).astype(np.float32)
        if F is None:
            F = fundamental_matrices(K, RT)
        # optional key (not in the reference): 'distCoef' (C, 5), the lens of every camera as Panoptic's calibration files and OpenCV give
        # it.  The pose network then undistorts the tracker's copy of every decode on the device, the tracker draws its boxes in the raw
        # image; the host keypoints and the 9-tuple's pts stay in raw-image pixels.
        dist = camera_parameter.get('distCoef') if hasattr(camera_parameter, 'get') else None
        from . import _lib
        self.lens = _lib.lens_table(K, dist)
        dist = np.asarray(dist, dtype=np.float64) if self.lens is not None else None
        self.cameras = [Camera(j, P[j], K[j], RT[j], F[j], w=im_width, h=im_height, distCoef=None if dist is None else dist[j])
                        for j in range(len(P))]
        if self.tracker is not None:
            self.tracker.set_cameras(self.cameras)
        if self.pose_model is not None:
            self.pose_model.set_lens(self.lens)
        return self.cameras

    def PersonDetect(self, imglist, image_id):
        """ivclabpose.py:183-204: per image a list of person dicts, boxes clamped to the image, xywh."""
        if self.person_detector is None or _cfg(self.person_detector, 'NAME') not in DETECTOR_NAMES:
            return None
        return self._person_dicts(imglist, image_id, self.bbox_detector(imglist))

    def PersonDetectAhead(self, imglist, image_id):
        """Not in the reference: PersonDetect split in two so that a driver which already holds the NEXT frame's images (the loader decodes
        ahead) can run that frame's detector under the current frame's pose network -- issue here (a stream of its own, nothing waits),
        collect with ``PersonDetectResult``.  Same boxes as PersonDetect (same replay, same decode)."""
        if self.person_detector is None or _cfg(self.person_detector, 'NAME') not in DETECTOR_NAMES:
            return None
        if getattr(self, '_det_stream', None) is None:
            self._det_stream = torch.cuda.Stream(self.bbox_detector.device)
        return (imglist, image_id, self.bbox_detector.submit(imglist, stream=self._det_stream))

    def PersonDetectResult(self, ahead):
        if ahead is None:
            return None
        imglist, image_id, ticket = ahead
        return self._person_dicts(imglist, image_id, self.bbox_detector.collect(ticket))

    def box_source(self, ahead=0):
        """'detector' | 'tracks' for the frame `ahead` frames after the next one ``schedule_frame`` hands out (pipeline.box_source on
        DETECT_EVERY); always 'detector' without a detector block's DETECT_EVERY."""
        from .pipeline import box_source
        return box_source(self.frames_scheduled + ahead, self.detect_every, self.person_detector is not None)

    def schedule_frame(self):
        """The source of the next frame's boxes; counts the frame."""
        src = self.box_source()
        self.frames_scheduled += 1
        return src

    def PersonBoxesFromTracks(self, imglist, image_id):
        """Not in the reference: a person_bbox_list in PersonDetect's format (plus a ``track_id`` key) whose boxes are drawn round the
        tracks' predicted poses for frame image_id instead of coming from the detector (IterativeTracker.predict_boxes; rule:
        ``self.track_box_rule``).  Tentative and Confirmed tracks, in the tracker's list order; empty lists before the first frame."""
        if self.tracker is None or self.tracker.handle is None:
            return [[] for _ in imglist]
        h, w = imglist[0].shape[:2]
        rows = self.tracker.predict_boxes(image_id, (h, w), **self.track_box_rule)
        out = self._person_dicts(imglist, image_id, [r[:, :5] for r in rows])
        for persons, r in zip(out, rows):
            for p, row in zip(persons, r):
                p['track_id'] = int(row[5])
        return out

    def _person_dicts(self, imglist, image_id, results):
        person_bbox_list = []
        for idx, result in enumerate(results):
            h, w = imglist[idx].shape[:2]
            person_temps = []
            for ret in result:
                x1, y1 = max(0, float(ret[0])), max(0, float(ret[1]))
                x2, y2 = min(float(ret[2]), w), min(float(ret[3]), h)
                person_temps.append(dict(image_id=image_id, category_id=1, score=float(round(float(ret[4]), 4)),
                                         bbox=[x1, y1, x2 - x1, y2 - y1], data=imglist[idx], feature=[]))
            person_bbox_list.append(person_temps)
        return person_bbox_list

    def PersonPoseDetect(self, imagelist=None, person_bbox_list=None, batch_size=20, image_id=None):
        if self.pose_model is None:
            return None
        return self.pose_model.predict(person_bbox_list, batch_size, self.conf_threshold)

    # -- a2 + a17 ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _unpack(dump_results):
        """dump dicts -> per-view (n,17,3) float64 rows (y, x, score) (ivclabpose.py:233-245)."""
        out = []
        for items in dump_results:
            if len(items) == 0:
                out.append(np.zeros((0, NUM_JOINTS, 3)))
                continue
            k = np.array([it['keypoints'] for it in items], dtype=np.float64).reshape(len(items), NUM_JOINTS, 3)
            s = np.array([it['keypoints_score'] for it in items], dtype=np.float64)
            out.append(np.stack([k[:, :, 1], k[:, :, 0], s], axis=2))
        return out

    def PersonTrack_Project3DPose(self, frame_id, person_bbox_list=None, dump_results=None, build3D='SVD'):
        dev = getattr(dump_results, 'device_det', None)
        if dev is not None and dev.shape[1] == self.tracker.max_dets and dev.shape[0] == len(self.cameras) and dump_results.device_valid():
            # the dump is the one PersonPoseDetect returned, untouched: its keypoints are still on the device in the tracker's
            # layout -> no re-packing, no host -> device copy (the dicts stay the source of truth whenever the caller edits them)
            # (the frame kernel is queued first: the one host wait of this call, behind it, also covers the keypoints' copy predict() enqueued)
            asso_time, update_time, init_time = self.tracker.tracking_dev(frame_id, self.cameras, dump_results.device_n_det, dev, build3D,
                                                                          on_void=getattr(dump_results, 'redo_if_void', None))
            poses = dump_results.poses_host
        else:
            poses = self._unpack(dump_results)
            boxes = [np.array([it['bbox'] for it in items]) for items in dump_results]
            frames = [(b[0]['data'] if len(b) else []) for b in person_bbox_list]
            ideal = poses
            if any(c.lens is not None for c in self.cameras):
                # the dicts hold raw-image pixels (and pts below is built from them): the tracker gets an undistorted copy
                from . import lens
                ideal = [p if c.lens is None else lens.undistort_rows(c.lens, p) for c, p in zip(self.cameras, poses)]
            asso_time, update_time, init_time = self.tracker.tracking(frame_id, self.cameras, frames, boxes, ideal, build3D)
        camera_ids, pts, person_ids, pts3d, pts3d_joints_views, person3d_ids = [], [], [], [], [], []
        # ONE_EURO: the emitted tracks' filtered poses, aligned with the returned pts3d ((n, 3, 17)); None without the block
        filtered = [] if self.tracker.one_euro is not None else None
        for tr in self.tracker.tracks:
            if not tr.emitted:
                continue
            pts3d.append(tr.pose3d.T)
            if filtered is not None:
                filtered.append(tr.pose3d_filtered.T)
            pts3d_joints_views.append(tr.joints_views)
            person3d_ids.append(tr.track_id)
            person_ids.append([tr.track_id] * len(tr.order))
            cams = [cid for cid in tr.order if tr.time2d[cid] == frame_id]
            camera_ids.append(cams)
            pts.append([poses[cid][tr.matched_det[cid]] for cid in cams])
        self.pts3d_filtered = np.array(filtered) if filtered is not None else None
        return (np.array(camera_ids, dtype='object'), np.array(pts, dtype='object'), person_ids, np.array(pts3d),
                pts3d_joints_views, np.array(person3d_ids), asso_time, update_time, init_time)
