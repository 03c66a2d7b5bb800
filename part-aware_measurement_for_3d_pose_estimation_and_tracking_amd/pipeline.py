"""On-device per-frame pipeline: crop/resize/normalise (HIP) -> HRNet-W48 conv stack (hand-written MFMA kernels, hipGraph replay) ->
head + arg-max decode (HIP) -> [all-gather of per-view keypoints when views are sharded] -> fused tracker frame kernel (HIP).
Nothing returns to the host inside a frame; the output record is copied out asynchronously.

This is the device-resident form of testmodel.py's loop body (/root/reference/src/testmodel.py:59-69):
PersonPoseDetect + PersonTrack_Project3DPose."""
import contextlib

import numpy as np
import torch

from . import _lib, stages
from .distributed import CropGather, ViewGather
from .hrnet import HRNetPose

NUM_JOINTS = 17


def box_source(frame_no, detect_every=1, have_detector=True):
    """Where the person boxes of a frame come from: 'detector' on every detect_every-th frame, counted from the last reset (frame_no %
    detect_every == 0: the detector finds who enters), 'tracks' in between (boxes round the tracks' predicted poses, pam_track_boxes).
    Pure: the schedule is the same on every rank.  A schedule that asks for a detector nobody attached is an error, never a silent
    frame of track boxes."""
    detect_every = int(detect_every)
    if detect_every < 1:
        raise ValueError('detect_every must be >= 1')
    if int(frame_no) % detect_every == 0:
        if not have_detector:
            raise ValueError('frame %d is a detector frame and no detector is attached' % frame_no)
        return 'detector'
    return 'tracks'


class FramePipeline(object):
    def __init__(self, calib_cameras, matcher, conf_threshold, frame_hw, max_dets=8, max_tracks=16, device=0, world=1,
                 rank=0, group=None, use_graph=True, hrnet=True, seed=0, shard='views', overlap_tracker=False, net=None, exchange='torch',
                 pose_streams=1, autotune=True, prewarm=False, width=48, resolution=(384, 288), flip_test=False, shift_heatmap=True,
                 post_process=False, model_name='HRNet', crop_cap=None, detect_every=1, dark=False, blur_kernel=None, pose_nms=False,
                 oks_thre=0.9, in_vis_thre=0.2, lens=None, one_euro=None, overlay=None, box_transform='stretch', box_scale=_lib.BOX_SCALE):
        """shard: 'views' -- rank owns whole camera views (pose_step / track_step take view-local inputs); 'crops' -- the
        frame's crops are dealt out evenly over the ranks (pose_step_crops / track_step_crops take global view indices).
        overlap_tracker (either mode): exchange + tracker kernel + fetch of frame t run on their own stream, under the conv
        stack of frame t+1 (the tracker is one workgroup per scene; it rides on CUs the conv kernels leave idle).
        pose_streams = 2: the crop -> conv stack -> decode chains of consecutive frames alternate between two streams, each with its own
        replay instance (static input, activations, output) of the same weights, so frame t+1's HBM-bound stem / layer1 runs beside
        frame t's CU-bound last stages.  Frames still finish in order (the tracker stream takes them in order).
        autotune: the conv stack's replay of every crop count is the fastest of the executor's configurations on this device
        (HRNetPose(autotune=True)).
        prewarm: capture the replay of every crop-count bucket this rank can see (its views x max_dets, in steps of the network's
        graph_bucket) at construction -- `self.warmed` says what that cost -- and pad every frame's forward to its bucket, so that no
        step() ever captures (the reference's call shape has a fixed batch_size = 20, /root/reference/src/ivclabpose.py:208-212).
        width / resolution: the pose network FramePipeline builds when no `net` is given (HRNet-W48 at 384 x 288; 32 / (256, 192) = W32;
        model_name='PoseResNet' with width = the ResNet depth, model_name='ViTPose' with width = 'B' / 'L' and resolution (256, 192),
        as HRNetPose takes them).
        flip_test / shift_heatmap / post_process: that network's decode options (HRNetPose: the official test protocol; the flip test
        doubles every forward, prewarm captures the doubled counts).  A shared `net` keeps its own settings.
        dark / blur_kernel: that network's DARK decode (HRNetPose; the forwards keep their size).
        crop_cap: rows of the device-built crop table (pose_step_boxes): crop, forward and decode of such a frame run for this many rows
        whatever the boxes' count.  None = this rank's views x max_dets; under prewarm rounded up to the network's bucket.
        detect_every: the schedule of pose_step_auto (box_source): the detector on every detect_every-th frame since the last reset(),
        boxes round the tracks' predictions in between.
        pose_nms / oks_thre / in_vis_thre: behind the decode of every frame (pose_step, pose_step_boxes, pose_step_auto) each view's poses
        are rescored and its duplicates removed by greedy OKS-NMS on the device (pam_pose_nms, the rule: include/pam.h; at most 32 slots
        per view).  ``self.nms_n_det`` (device, one count per view of this rank) is then the n_det_local for track_step -- it replaces
        ``table_n_det`` -- and results() adds rec['pose_nms'] = dict(n_det, keep_from).  Box scores: the detector's, read in place from
        its list, on detector frames; 1.0 on track-box frames; pose_step takes a table.  The pipeline's own setting: a shared `net`
        keeps its own (HRNetPose.predict's).  Off: every step issues exactly the launches it issued without the option.
        lens: the rig's (C, 10) float64 lens table (_lib.lens_table; one row per camera, of ALL C views).  Behind the decode of every
        frame -- and behind pose_nms, whose OKS areas come from raw-image boxes -- this rank's keypoints are undistorted in place on the
        device (pam_undistort_keypoints; the model: include/pam.h), so view sharding exchanges ideal coordinates; ``undistort_local``
        does the same for rows a caller placed with write_local.  track_boxes then draws its boxes in the raw image (pam_set_lens).
        ``lens_info`` (device, 2 int32): [points that could not be inverted and were left as they were, points looked at] of the last
        launch.  None, or no non-zero coefficient: every step issues exactly the launches it issued without the option.
        one_euro: True (_lib.ONE_EURO_3D) or dict(freq, mincutoff, beta, dcutoff): behind the frame kernel of every track_step /
        track_step_crops, on the tracker's stream, the tracks' newest 3D poses go through One-Euro filters on the device (pam_one_euro;
        the rules: include/pam.h) and results() adds rec['pose3d_filtered'] ((n_tracks, 17, 3), the record's order) and
        rec['filter_meta'] = dict(n_fresh, ids, fresh, samples).  An output filter: the tracker state and the record are what they are
        without it; with view sharding every rank filters its own replica, nothing is exchanged.  None: the launches of before.
        overlay: dict(view3d=None | dict(size=(width, height), azimuth=, elevation=, up=), emitted_only=True) switches ``overlay_step``
        on: the tracks drawn into this rank's CUDA frames -- and into a free-viewpoint 3D canvas when view3d is given -- straight from
        the device-resident state (pam_overlay_tracks + pam_overlay_draw_counted; the rules: include/pam.h), the One-Euro poses when
        one_euro is on.  Needs shard='views'.  None: no step, no buffer, the launches of before.
        box_transform / box_scale: that network's crop geometry (HRNetPose): 'affine' crops every box of pose_step, pose_step_boxes,
        pose_step_auto and pose_step_crops through the pose checkpoints' centre/scale transform (include/pam.h); the crop launch leaves
        the frame's effective boxes in a device table beside the other per-frame buffers (``eff_table``, sized for the bucket cap, one per
        replay slot) and decode and pose_nms read that table in place of the boxes.  pam_crop_table and pam_track_boxes are unchanged and
        still deliver raw clamped boxes: on a track-box frame TRACK_BOX_GROW 1.25 and BOX_SCALE 1.25 MULTIPLY (a box 1.56 x the
        keypoints' extent); both defaults are left alone.  'udp': the same table and the same paths with the UDP protocol's align-corners
        crop and decode (pam_preprocess_crops_udp, pam_head_decode_udp; HRNetPose refuses it with post_process).  A shared `net` keeps
        its own setting.  'stretch': the launches of before."""
        box_transform, box_scale = _lib.check_box_transform(box_transform, box_scale)
        if overlay is not None and shard == 'crops':
            raise ValueError("overlay needs shard='views': a rank draws the frames of the views it owns")
        lens = _lib.check_lens(lens, len(calib_cameras))
        if lens is not None and shard == 'crops':
            raise ValueError("lens needs shard='views': crop sharding gathers rows whose view the device-side step cannot name")
        if lens is not None and max_dets > _lib.POSE_NMS_MAX:
            raise ValueError('lens takes at most %d slots per view (max_dets=%d)' % (_lib.POSE_NMS_MAX, max_dets))
        if pose_nms and shard == 'crops':
            raise ValueError("pose_nms needs shard='views': crop sharding builds its select index from the host box list, before the filter")
        if pose_nms and max_dets > _lib.POSE_NMS_MAX:
            raise ValueError('pose_nms takes at most %d slots per view (max_dets=%d)' % (_lib.POSE_NMS_MAX, max_dets))
        self.device = torch.device('cuda:%d' % device)
        torch.cuda.set_device(self.device)
        self.cams = calib_cameras
        self.C = len(calib_cameras)
        self.max_dets = max_dets
        self.frame_h, self.frame_w = frame_hw
        self.world, self.rank = world, rank
        self.params = _lib.make_params(matcher, conf_threshold)
        self.handle = _lib.Handle(self.C, self.params, max_dets=max_dets, max_tracks=max_tracks, n_scenes=1, device=device)
        self.handle.set_cameras(np.stack([c.P for c in calib_cameras]), np.stack([c.F for c in calib_cameras]),
                                np.stack([c.RK_INV for c in calib_cameras]), np.stack([c.position for c in calib_cameras]))
        # the side outputs that travel with the record (stages.py; results() adds them in this order): the One-Euro rows, the crop
        # table's info words (below), the filter's counts (below)
        self.one_euro = _lib.one_euro_config(one_euro)
        self._oe = stages.OneEuro(self.handle, self.one_euro) if self.one_euro is not None else None
        self.lens, self.lens_info = None, None
        if lens is not None:
            self.handle.set_lens(lens)
            self.lens = torch.from_numpy(lens).to(self.device)
            self.lens_info = torch.zeros(2, dtype=torch.int32, device=self.device)
        # net: an existing HRNetPose to share (weights, packed images, captured graphs) between several pipelines of one process
        self.net = net if net is not None else (HRNetPose(width, 17, None, model_name=model_name, resolution=tuple(resolution), device=device,
                                                          use_graph=use_graph, seed=seed,
                                                          max_dets=max_dets, autotune=autotune,
                                                          max_crops=len(calib_cameras) * max_dets, flip_test=flip_test,
                                                          shift_heatmap=shift_heatmap, post_process=post_process, dark=dark,
                                                          blur_kernel=blur_kernel, pose_nms=pose_nms, oks_thre=oks_thre,
                                                          in_vis_thre=in_vis_thre, box_transform=box_transform,
                                                          box_scale=box_scale) if hrnet else None)
        self.shard = shard
        # exchange: 'torch' = torch.distributed (RCCL when the backend is nccl, gloo in the CPU tests); 'abi' = pam_allgather_keypoints,
        # the library's own RCCL call on the decode stream (view sharding only)
        self.comm = None
        if exchange == 'abi':
            from .distributed import AbiComm
            self.comm = AbiComm(world, rank, device, group)
        self.gather = ViewGather(self.C, max_dets, world, rank, self.device, group, abi=(self.handle, self.comm) if self.comm else None)
        self.crop_gather = CropGather(self.C, max_dets, world, rank, self.device, group) if shard == 'crops' else None
        self.mine = self.gather.mine
        self._lens_views = torch.tensor(list(self.mine) or [0], dtype=torch.int32, device=self.device) if lens is not None else None
        # decode target: this rank's views only -- the leading records of the exchange's send buffer, (len(mine), max_dets + 1, 17, 3):
        # slot stride max_dets + 1, the extra row carries the view's detection count (ViewGather)
        self.det_local = self.gather.det_local
        self._rec_keep, oi, od = self.handle.pinned_record()           # one pinned buffer in the device record's layout: one copy per fetch
        self.out_i, self.out_d = torch.from_numpy(oi), torch.from_numpy(od)
        self.ev = None
        self.track_stream, self.track_overlaps = self._pick_track_stream() if overlap_tracker else (None, False)
        self.ev_pose, self.ev_track, self._track_pending = torch.cuda.Event(), torch.cuda.Event(), False
        assert pose_streams in (1, 2) and (pose_streams == 1 or overlap_tracker), 'two pose streams need the tracker on its own stream'
        self.pose_streams = [torch.cuda.Stream(self.device) for _ in range(pose_streams)] if pose_streams > 1 else None
        self._frame_no = 0
        # device-side gates (pam_sync.hip) need the forward to be the only flagged work on the device: two forwards in flight can block
        # each other's queues, and so can the replays of several ranks that share one device (more ranks than devices: one-device tests)
        # (which ranks share one is decided from the devices' identities: a launcher that shows each rank a single device has device_count() == 1)
        from .distributed import ranks_share_a_device
        self.shared_device = ranks_share_a_device(self.device, group) if world > 1 else False
        if self.net is not None and (self.pose_streams is not None or self.shared_device):
            self.net.disable_flag_sync()
        if self.net is not None:
            self.net.flag_race = 'throughput'        # the pipeline keeps the host a frame ahead of the device: time the flag race that way
            # Keypoints of a forward whose gate gave up must not reach the tracker state.  The host runs a frame ahead and cannot look, so
            # the frame kernel does: it skips every frame while the producer's void word is up (pam_set_input_guard; results() then raises
            # FrameVoid with the frame to resume from).  Sharded: the word travels with the exchange, so that every rank's replica skips
            # the same frames -- inside the view records (ViewGather.exchange), or as CropGather.void_any, which is the guard there.
            guard = self.crop_gather.void_any if (shard == 'crops' and world > 1) else self.net.void_word
            self.handle.set_input_guard(guard.data_ptr())
        self.bucketed, self.warmed = bool(prewarm), None
        if prewarm and self.net is not None:
            most = (self.C if shard == 'crops' else len(self.mine)) * max_dets
            if shard == 'crops' and world > 1:
                most = (most + world - 1) // world
            self.warmed = self.net.warm(most, slots=(0, 1) if pose_streams > 1 else (0,))
        self.detect_every, self._auto_no, self._det_ahead = int(detect_every), 0, None
        if self.detect_every < 1:
            raise ValueError('detect_every must be >= 1')
        self.crop_cap = int(crop_cap) if crop_cap is not None else max(1, len(self.mine) * max_dets)
        if self.crop_cap < 1:
            raise ValueError('crop_cap must be >= 1')
        if self.bucketed and self.net is not None:
            self.crop_cap = self.net.bucket(self.crop_cap)
        self._tables, self._tb, self.table_n_det = None, None, None
        # box_transform='affine' / 'udp': the effective boxes of a frame, written by its crop launch and read by its decode and filter; one table
        # per replay slot (two frames in flight), rows for the largest frame this rank can see, rounded up to the bucket as crop_cap is
        # (built here when the network has the option on, else at the first frame of a shared net whose owner switches it on later)
        self.eff_table = None
        if self.net is not None and self.net.box_transform != 'stretch':
            self._eff_rows(0, 0)
        self._ct = stages.CropTableInfo()
        self._ev_slot_read, self._table_no, self._table_slot = [None, None], 0, 0
        # the OKS-NMS behind the decode: [n_det | keep_from] int32 and the new scores, one set (the launch sits behind wait_track, so the
        # track step of the frame before has read its counts), and a pinned copy of the int32 part that travels with the record's fetch
        self.pose_nms, self.oks_thre, self.in_vis_thre = bool(pose_nms), float(oks_thre), float(in_vis_thre)
        self._nms = stages.PoseNmsOut(max(1, len(self.mine)), max_dets, self.device) if self.pose_nms else None
        self.nms_n_det, self.nms_keep_from, self.nms_pose_score = \
            (self._nms.n_det, self._nms.keep_from, self._nms.pose_score) if self.pose_nms else (None, None, None)
        self.overlay = None
        if overlay is not None:
            unknown = set(overlay) - {'view3d', 'emitted_only'}
            if unknown:
                raise ValueError('overlay: unknown key(s) %s (view3d, emitted_only)' % sorted(unknown))
            self.overlay = dict(emitted_only=bool(overlay.get('emitted_only', True)), view3d=None)
            self.ev_overlay = (torch.cuda.Event(), torch.cuda.Event())      # frames ready -> draw, draw done -> consumer
            if overlay.get('view3d') is not None:
                from .visualization import view3d_setup
                v3 = view3d_setup(calib_cameras, overlay['view3d'], self.device, what="overlay['view3d']")
                self.view3d_P, self.view3d_background, self.view3d_canvas = v3['P_dev'], v3['background'], None
                self.overlay['view3d'] = dict(size=v3['size'], P=v3['P'])

    def _pick_track_stream(self, tries=8, spin_us=400, avoid=None):
        """A stream for the exchange + tracker that REALLY runs beside the caller's (pose) stream.  HIP streams are multiplexed onto a few
        hardware queues (4 by default on ROCm 7.2) and a queue is in-order: the first stream the pool handed out sat on the pose stream's
        queue, so frame t's 80 us tracker kernel ran in FRONT of frame t + 1's crop kernel instead of under its conv stack (rocprofv3
        kernel trace, tools/frame_timeline.py: 110 us from the end of the head kernel to the next frame's first kernel, 10-20 us once
        the two streams are on different queues; +4.6 % frames/s).  Which queue a stream gets is decided at its first use and cannot be
        queried, so this measures it: two spin kernels (pam_clock_probe, one wave each), one per stream, take as long as ONE when the
        queues differ and as long as two when they are the same.  Returns (stream, overlaps); the first candidate that overlaps wins.
        The reference point is the stream that is current when the pipeline is built (frames are issued on the caller's current stream);
        with pose_streams = 2 the frames run on two pool streams of their own, which this does not test against.
        avoid: streams the new one must ALSO overlap with (the detector's stream must share a queue neither with the pose nor with the
        tracker stream)."""
        import ctypes as C
        import time
        pose = torch.cuda.current_stream(self.device)
        out = torch.zeros(4, dtype=torch.int64, device=self.device)
        lib = self.handle.lib
        others = [o for o in (avoid or []) if o is not None]

        def pair(x, y, us):
            torch.cuda.synchronize(self.device)
            t0 = time.perf_counter()
            for st, o in ((x, out), (y, out[2:])):
                if lib.pam_clock_probe(C.c_void_p(st.cuda_stream), C.c_void_p(o.data_ptr()), us) != 0:
                    raise _lib.PamError('pam_clock_probe failed')
            torch.cuda.synchronize(self.device)
            return time.perf_counter() - t0
        cands = []
        for _ in range(tries):
            s = torch.cuda.Stream(self.device)
            cands.append(s)
            pair(pose, s, 20)                            # first use: the stream gets its hardware queue here
            if all(min(pair(o, s, spin_us) for _ in range(3)) < 1.5e-6 * spin_us for o in [pose] + others):
                return s, True
        return cands[0], False

    # -- person detector of frame t + 1 under the pose network of frame t -----------------------------------------------------------------
    def attach_detector(self, detector, frames=None, n_crops=None, candidates=6):
        """detector: a pam.yolov3.YOLOv3.  The reference loop is detect -> pose -> track per frame (/root/reference/src/testmodel.py:59-63,
        ivclabpose.py:183-204); here frame t + 1's detection (k_resize_frames -> Darknet-53 -> k_yolo_detect, one hipGraph replay) is
        issued on a stream and hardware queue of its own as soon as frame t's crop kernel has read the detector's previous output, and
        runs under frame t's conv stack; frame t + 1's crop kernel waits (on the device) for it.
        frames + n_crops: choose the detector's stream by MEASUREMENT -- four hardware queues serve all streams and the pose replay's
        own branch chains sit on all of them, so which queue the detector shares decides how much of it hides: `candidates` fresh
        streams are each timed running the detector's replay beside the n_crops pose replay, the fastest pair wins (``det_pick``)."""
        import time
        self.detector = detector
        self.det_stream, self.det_overlaps = self._pick_track_stream(avoid=[self.track_stream])
        self.det_pick = None
        if frames is not None and n_crops and self.net is not None:
            cur = torch.cuda.current_stream(self.device)
            x = self.net.input_buffer(int(n_crops))
            self.net.features(x); detector.detect_dev(frames)
            torch.cuda.synchronize(self.device)

            def both(st, reps=6):
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                for _ in range(reps):
                    self.net.features(x)
                    with torch.cuda.stream(st):
                        detector.detect_dev(frames)
                torch.cuda.synchronize(self.device)
                return (time.perf_counter() - t0) / reps
            cands = [self.det_stream] + [torch.cuda.Stream(self.device) for _ in range(candidates - 1)]
            times = []
            for st in cands:
                both(st, 2)
                times.append(min(both(st) for _ in range(2)))
            k = int(np.argmin(times))
            self.det_stream = cands[k]
            self.det_pick = {'ms_pose_and_detector_side_by_side': [float(t * 1e3) for t in times], 'chosen': k}
        self.ev_det, self.ev_crop = [torch.cuda.Event(), torch.cuda.Event()], torch.cuda.Event()
        self._det_frames = 0

    def detect_ahead(self, frames):
        """Issue the detection of the NEXT frame (frames: its (views, H, W, 3) uint8 BGR device tensor) behind the crop kernel that was
        issued last on the current stream; returns (boxes, count) device tensors, valid once ``wait_detection`` of that frame has run."""
        cur = torch.cuda.current_stream(self.device)
        self.ev_crop.record(cur)
        with torch.cuda.stream(self.det_stream):
            self.det_stream.wait_event(self.ev_crop)
            out = self.detector.detect_dev(frames)
            self._det_frames += 1
            self.ev_det[self._det_frames & 1].record(self.det_stream)
        return out

    def wait_detection(self):
        """Order the current stream behind the latest detection issued by ``detect_ahead`` (call before the frame's crop kernel)."""
        torch.cuda.current_stream(self.device).wait_event(self.ev_det[self._det_frames & 1])

    def stream_ptr(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _pose(self, frame_ptrs, views, slot_of, boxes, det, time_events, after_crop=None, n_det=None, score=(None, (0, 0), None)):
        """crop -> conv stack -> head + arg-max for one frame on the current stream, replay slot = frame parity when two pose streams run.
        pose_nms: + the filter, from the counts n_det and the box scores score = (tensor or address, strides, view map)."""
        k = (self._frame_no & 1) if self.pose_streams is not None else 0
        n = int(views.numel())
        x = self.net.input_buffer(self.net.bucket(n) if self.bucketed else n, k)     # a bucket's spare rows repeat the last crop, undecoded
        eff = self._eff_rows(k, n) if self.net.box_transform != 'stretch' else None
        self.net.preprocess(frame_ptrs, self.frame_h, self.frame_w, views, boxes, x, eff=eff)
        if eff is not None:
            boxes = eff                                  # decode and filter go through the effective boxes (transform_preds)
        if after_crop is not None:
            after_crop()                                # the frames have been read: a feeder may mark its buffers reusable here
        if time_events is not None:
            time_events[0].record(torch.cuda.current_stream(self.device))
        f = self.net.features(x, k)
        if time_events is not None:
            time_events[1].record(torch.cuda.current_stream(self.device))
        self.wait_track()                               # the previous frame's exchange / tracker read the buffer decode writes
        self.net.head_decode(f, views, slot_of, boxes, det, n=n)
        nms = None
        if self.pose_nms:
            nms = (self.nms_n_det, self.nms_keep_from, self.nms_pose_score, dict(score=score[0], score_strides=score[1], views=score[2],
                                                                                 oks_thre=self.oks_thre, in_vis_thre=self.in_vis_thre))
            self._nms.live = True
        stages.after_decode(torch.cuda.current_stream(self.device).cuda_stream, det, n_det, (views, slot_of, boxes), nms=nms,
                            lens=(self.lens, self.lens_info, self._lens_views) if self.lens is not None else None, max_dets=self.max_dets)

    def _eff_rows(self, k, n):
        """The first n rows of replay slot k's effective-box table (box_transform='affine' / 'udp'); the tables hold the largest frame this rank
        can see -- crop_cap or every view x max_dets, rounded up to the bucket as crop_cap is -- and one grows for a longer caller's table."""
        if self.eff_table is None:
            rows = max(self.crop_cap, self.C * self.max_dets)
            rows = self.net.bucket(rows) if self.bucketed else rows
            self.eff_table = [torch.zeros((rows, 4), dtype=torch.float32, device=self.device)
                              for _ in range(len(self.pose_streams) if self.pose_streams is not None else 1)]
        if n > self.eff_table[k].shape[0]:
            self.eff_table[k] = torch.zeros((n, 4), dtype=torch.float32, device=self.device)
        return self.eff_table[k][:n]

    def undistort_local(self, n_det):
        """Lens distortion out of this rank's rows, in place in ``self.det_local`` (decode, write_local), behind whatever the current
        stream holds and in front of track_step: n_det = one int32 device count per view of this rank, what track_step is given.
        Local view i is camera mine[i] of the lens table.  Nothing is launched when the pipeline has no table."""
        if self.lens is None or not len(self.mine):
            return
        _lib.undistort_keypoints(torch.cuda.current_stream(self.device).cuda_stream, self.det_local, n_det, self.lens, self.lens_info,
                                 max_dets=self.max_dets, views=self._lens_views)

    def _no_crops(self, n, after_crop):
        """The one exit of a pose step that has nothing to run (no crop, no view of this rank, no network): a feeder's release and the
        next frame's detection are due on such frames too.  -> whether the step is over."""
        if n and self.net is not None:
            return False
        if after_crop is not None:
            after_crop()
        return True

    @contextlib.contextmanager
    def frame(self):
        """Everything of ONE frame (pose_step*, write_*, track_step*) goes inside.  With two pose streams the frame runs on the stream of
        its parity (ordered behind the caller's stream, which holds its inputs) with that parity's replay slot, so the forwards of
        consecutive frames overlap; frame t + 2 follows frame t on the same stream, which also orders the reuse of the slot."""
        if self.pose_streams is None:
            yield
            self._frame_no += 1
            return
        ps = self.pose_streams[self._frame_no & 1]
        ps.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(ps):
            yield
        self._frame_no += 1

    def pose_step(self, frame_ptrs, view_local, slot_of, boxes, time_events=None, after_crop=None, n_det=None, scores=None):
        """HRNet side for this rank's crops.  view_local: int32 (N,) index into self.mine; writes self.det_local.
        pose_nms: n_det (one int32 device count per view of this rank, what track_step would have been given) is required and
        ``self.nms_n_det`` is what track_step takes instead; scores: (len(mine), max_dets) float32 device table of box scores (None: 1.0)."""
        self._ct.info = None
        if self._nms is not None:
            self._nms.live = False
        if self.pose_nms and self.net is not None and n_det is None:
            raise ValueError('pose_step with pose_nms needs n_det: the filter starts from the per-view counts')
        if self.lens is not None and self.net is not None and n_det is None:
            raise ValueError('pose_step with a lens table needs n_det: the step undistorts the rows below the per-view counts')
        if self._no_crops(int(view_local.numel()), after_crop):
            if self.pose_nms and self.net is not None:  # nothing decoded, nothing kept
                self.wait_track()
                self._nms.nothing_kept()
            return
        self._pose(frame_ptrs, view_local, slot_of, boxes, self.det_local, time_events, after_crop, n_det=n_det,
                   score=(scores, (self.max_dets, 1), None))

    def write_local(self, rows):
        """Copy keypoint rows (len(mine), max_dets, 17, 3) into this rank's records, ordered behind the previous frame's readers."""
        self.wait_track()
        self.det_local[:, :self.max_dets].copy_(rows.reshape(-1, self.max_dets, NUM_JOINTS, 3)[:self.det_local.shape[0]])

    def track_step(self, frame_id, n_det_local, det_local=None, fetch=True):
        """Exchange (if sharded) + fused tracker kernel on the gathered records, read in place through the row map
        (pam_frame_dev_views); async fetch of the record.  det_local: None / ``self.det_local`` = the rows are already in the send
        buffer (decode, write_local); any other tensor is copied in first."""
        if det_local is not None and det_local.data_ptr() != self.det_local.data_ptr():
            self.write_local(det_local)

        def frame_kernel(st):
            recv = self.gather.exchange(n_det_local, self.net.void_word if self.net is not None else None)
            self.handle.frame_dev_views(st, frame_id, recv.data_ptr(), self.gather.rows.data_ptr())
        self._track(frame_id, fetch, frame_kernel)

    def _behind_tracker(self, issue, ev_in, ev_out, rejoin):
        """issue(torch stream) on the tracker's stream, behind the last tracker step.  ev_in: the event through which the tracker's stream
        first waits for what the current stream holds (None: it does not wait); ev_out is recorded behind the work.  rejoin: the current
        stream then waits for ev_out, and the hop is taken only while a step is pending there; otherwise ev_out is left for a later
        waiter (wait_track).  Without a tracker stream (or a pending step, under rejoin) the work is issued on the current stream.
        -> whether the hop was taken."""
        cur = torch.cuda.current_stream(self.device)
        if self.track_stream is None or (rejoin and not self._track_pending):
            issue(cur)
            return False
        if ev_in is not None:
            ev_in.record(cur)
        with torch.cuda.stream(self.track_stream):
            if ev_in is not None:
                self.track_stream.wait_event(ev_in)
            issue(self.track_stream)
            ev_out.record(self.track_stream)
        if rejoin:
            cur.wait_event(ev_out)
        return True

    def _track(self, frame_id, fetch, frame_kernel):
        """The body of track_step and track_step_crops: frame_kernel(stream pointer) -- the exchange and the frame kernel -- then the
        One-Euro launch, and with ``fetch`` the record's copy with the side outputs that travel with it (results()); on the tracker's
        stream, behind the pose stream, when there is one."""
        def issue(stream):
            st = stream.cuda_stream
            frame_kernel(st)
            if self._oe is not None:
                self._oe.step(st, frame_id, fetch)
            if fetch:
                self.handle.fetch(st, self.out_i.numpy(), self.out_d.numpy())
                self._ct.fetch()
                if self._nms is not None:
                    self._nms.fetch()
        if not self._behind_tracker(issue, self.ev_pose, self.ev_track, rejoin=False):
            return
        if self._ct.info is not None:                    # this frame's table set (its n_det) has been read: pose_step_boxes may refill it
            k = self._table_slot
            self._ev_slot_read[k] = self._ev_slot_read[k] or torch.cuda.Event()
            self._ev_slot_read[k].record(self.track_stream)
        self._track_pending = True

    def overlay_step(self, frames):
        """overlay=: the tracks as the last track_step left them, drawn into ``frames`` -- this rank's CUDA frames, one contiguous uint8
        (H, W, 3) BGR tensor per view of ``mine`` in order -- IN PLACE, and into the 3D canvas when view3d is configured: a NEW tensor every
        call (``view3d_canvas``: the background's copy with the tracks on top), so that a FrameWriter may still be reading the one
        before.  Issued on the tracker's stream behind the frame kernel and the One-Euro launch of that step, and behind whatever
        the current stream holds (the frames' producer); the current stream then waits for the draw, so the result can go straight to
        FrameWriter.submit.  Nothing is fetched: it works with track_step(fetch=False).  -> the list of frames (+ the canvas)."""
        if self.overlay is None:
            raise ValueError('overlay_step needs FramePipeline(overlay=...)')
        from .visualization import draw_tracks_device
        frames = list(frames)
        if len(frames) != len(self.mine):
            raise ValueError('overlay_step takes one frame per view of this rank (%d), got %d' % (len(self.mine), len(frames)))
        views, extra = [int(c) for c in self.mine], None
        if self.overlay['view3d'] is not None:
            self.view3d_canvas = torch.empty_like(self.view3d_background)      # (allocated on the consumer's stream, filled on the draw's)
            frames, views, extra = frames + [self.view3d_canvas], views + [-1], self.view3d_P
        pose = self._oe.dev[0] if self._oe is not None else None

        def issue(st):
            if extra is not None:
                self.view3d_canvas.copy_(self.view3d_background)
            draw_tracks_device(self.handle, frames, views=views, extra=extra, pose=pose, emitted_only=self.overlay['emitted_only'], stream=st)
        self._behind_tracker(issue, self.ev_overlay[0], self.ev_overlay[1], rejoin=True)
        return frames

    # -- person boxes that never visit the host ------------------------------------------------------------------------------
    def reset(self):
        """Forget every track (handle.reset()) and restart the schedule of pose_step_auto: the next frame is a detector frame."""
        self.handle.reset()
        self._auto_no, self._det_ahead = 0, None

    def _box_buffers(self):
        if self._tables is None:
            dev, cap, nv = self.device, self.crop_cap, max(1, len(self.mine))
            self._tables = [dict(view_of=torch.zeros(cap, dtype=torch.int32, device=dev), slot_of=torch.zeros(cap, dtype=torch.int32, device=dev),
                                 xywh=torch.zeros((cap, 4), dtype=torch.float32, device=dev),
                                 n_det=torch.zeros(nv, dtype=torch.int32, device=dev), info=torch.zeros(4, dtype=torch.int32, device=dev))
                            for _ in range(2)]
            self._tb = self.handle.track_box_buffers()
            self._mine_dev = torch.tensor(list(self.mine) or [0], dtype=torch.int32, device=dev)
            self.ev_boxes = torch.cuda.Event()

    def track_boxes(self, frame_id, **rule):
        """Person boxes of frame_id round the tracks' constant-velocity predictions (pam_track_boxes; rule: grow, pad_px, min_size_px,
        max_gap, defaults _lib.TRACK_BOX_RULE) -> (boxes (C, max_dets, 5), count (2C,), ids (C, max_dets)) device tensors for ALL C
        views, in the detector's layout; pipeline-owned, valid until the next call.
        Ordering: the kernel is issued behind the last tracker step that was issued -- on the track stream when there is one, with an
        event the current (pose) stream then waits on.  So the boxes always come from the state after the previous track_step, whatever
        overlap_tracker says: a frame whose boxes come from here cannot start its crops before the previous frame's k_frame has ended,
        which costs the overlap of k_frame under this frame's forward (the record's fetch still overlaps)."""
        self._box_buffers()
        self._behind_tracker(lambda st: self.handle.track_boxes(st.cuda_stream, frame_id, self.frame_w, self.frame_h, *self._tb, **rule),
                             None, self.ev_boxes, rejoin=True)
        return self._tb[:3]

    def pose_step_boxes(self, frame_ptrs, boxes, count, views=None, time_events=None, after_crop=None, use_scores=True):
        """pose_step on boxes that are on the device in the detector's layout (YOLOv3.detect_dev, track_boxes): boxes (G, max_det, 5)
        float32, count (>= G,) int32; views: int32 device tensor, for each of this rank's views the image of `boxes` that holds its list
        (None: image i is view mine[i]).  pam_crop_table turns them into a crop table of crop_cap rows (spare rows repeat the last real
        one), and crop, forward and decode run for crop_cap rows through the kernels pose_step uses.  ``self.table_n_det`` (device, one
        count per view of this rank) is the n_det_local for track_step -- ``self.nms_n_det`` under pose_nms, whose box scores are column 4
        of `boxes`, read in place (use_scores=False: 1.0)."""
        if self._nms is not None:
            self._nms.live = False
        if self.shard != 'views':
            raise ValueError("pose_step_boxes needs shard='views': crop sharding builds its select index from a host box list")
        if self._no_crops(len(self.mine), after_crop):
            return
        self._box_buffers()
        k = self._table_slot = self._table_no & 1       # two sets: the track step of the frame before may still be reading the other one
        self._table_no += 1
        T = self._tables[k]
        cur = torch.cuda.current_stream(self.device)
        if self._ev_slot_read[k] is not None:
            cur.wait_event(self._ev_slot_read[k])       # the track step of two frames ago has read this set's counts
        _lib.crop_table(cur.cuda_stream, boxes, count, self.frame_w, self.frame_h, self.max_dets, T['view_of'], T['slot_of'], T['xywh'],
                        T['n_det'], T['info'], views=views)
        self.table_n_det, self._ct.info = T['n_det'], T['info']
        score = (boxes.data_ptr() + 16, (5 * int(boxes.shape[1]), 5), views) if (self.pose_nms and use_scores) else (None, (0, 0), None)
        self._pose(frame_ptrs, T['view_of'], T['slot_of'], T['xywh'], self.det_local, time_events, after_crop, n_det=T['n_det'], score=score)

    def pose_step_auto(self, frame_id, frame_ptrs, frames, next_frames=None, time_events=None, after_crop=None, **rule):
        """pose_step_boxes with the boxes the schedule names (box_source(frames since reset(), detect_every)): the detector's -- the
        result of the detect_ahead this method issued during the frame before when `next_frames` was given, else detect_dev(frames) in
        line -- or track_boxes(frame_id).  frames: this rank's (views, H, W, 3) uint8 device tensor; next_frames: the next frame's, to
        run its detection under this frame's forward when the next frame is a detector frame.  -> 'detector' | 'tracks'."""
        det = getattr(self, 'detector', None)
        src = box_source(self._auto_no, self.detect_every, det is not None)
        views = None
        if src == 'detector':
            if self._det_ahead is not None:
                boxes, count = self._det_ahead
                self._det_ahead = None
                self.wait_detection()
            else:
                boxes, count = det.detect_dev(frames)
        else:
            boxes, count, _ = self.track_boxes(frame_id, **rule)
            self._box_buffers()
            views = self._mine_dev
        ahead = next_frames is not None and det is not None and hasattr(self, 'det_stream') and \
            box_source(self._auto_no + 1, self.detect_every, True) == 'detector'

        def crop_done():
            if after_crop is not None:
                after_crop()
            if ahead:
                self._det_ahead = self.detect_ahead(next_frames)
        self.pose_step_boxes(frame_ptrs, boxes, count, views=views, time_events=time_events, after_crop=crop_done,
                             use_scores=src == 'detector')
        self._auto_no += 1
        return src

    # -- crop-balanced sharding ----------------------------------------------------------------------------------------------
    def wait_track(self):
        """Order the caller's stream behind the previous frame's exchange / tracker (they read ``crop_gather.send`` / the view
        records): call before ANY write to that buffer -- decode, or a caller that fills it itself."""
        if self._track_pending:
            torch.cuda.current_stream(self.device).wait_event(self.ev_track)

    def write_send(self, rows):
        """Copy keypoint rows (C, max_dets, 17, 3) into the exchange buffer, ordered behind the previous frame's readers."""
        self.wait_track()
        self.crop_gather.send.copy_(rows)

    def pose_step_crops(self, frame_ptrs, view_of, slot_of, boxes, time_events=None, after_crop=None):
        """HRNet side for this rank's share of the frame's crops; view_of indexes ALL views (frame_ptrs has C entries).
        Decodes straight into the exchange buffer at (view, slot)."""
        if self._no_crops(int(view_of.numel()), after_crop):
            return
        self._pose(frame_ptrs, view_of, slot_of, boxes, self.crop_gather.send, time_events, after_crop)

    def track_step_crops(self, frame_id, n_det, select, fetch=True):
        """n_det (C,) int32 and select (CropGather.select_index) are the same on every rank (they follow from the frame's box
        list); the keypoint rows come from ``crop_gather.send`` of the rank that owns each crop."""
        def frame_kernel(st):
            det = self.crop_gather.gather(select, self.net.void_word if self.net is not None else None)
            self.handle.frame_dev(st, frame_id, n_det.data_ptr(), det.data_ptr())
        self._track(frame_id, fetch, frame_kernel)

    def results(self, strict=True):
        """Synchronise and decode the last fetched record.  strict: a non-zero status word (capacity overflow, infeasible
        assignment, clamped detection count -- include/pam.h) IN ANY FRAME since the handle was created or reset (the sticky half of
        the word) raises instead of passing silently into the caller's numbers."""
        if self.pose_streams is not None:
            for ps in self.pose_streams:
                ps.synchronize()
        if self.track_stream is not None:
            self.track_stream.synchronize()
        torch.cuda.current_stream(self.device).synchronize()
        rec = self.handle.decode(0, self.out_i.numpy(), self.out_d.numpy())
        if rec['status'] & _lib.ST_INPUT_VOID:
            # a gate of a captured forward timed out in frame rec['first_void']: the tracker (every rank's replica) skipped that frame and
            # all since; the network is on stream events by now (HRNetPose.check_void).  Lower the word and tell the caller where to resume.
            if self.net is not None:
                self.net.check_void()
                self.net.clear_void()
            raise _lib.FrameVoid(rec['first_void'], rec['frame_id'])
        if strict and (rec['status'] | rec['status_sticky']) != 0:
            raise _lib.PamError('tracker status 0x%x on frame %d, 0x%x over the run (1 track slots, 2 hypothesis slots, 4 infeasible '
                                'assignment, 8 clamped detection count)' % (rec['status'], rec['frame_id'], rec['status_sticky']))
        for side in (self._oe, self._ct, self._nms):     # pose3d_filtered / filter_meta, crop_table, pose_nms
            if side is not None and side.fetched:
                side.add_to(rec)
        return rec
