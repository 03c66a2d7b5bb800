"""HRNet-W48 / -W32, PoseResNet and ViTPose top-down 2D pose (a1): the ``HRNetPose(...).predict(...)`` seam of the reference
(/root/reference/src/ivclabpose.py:125-134,210; the backend itself is git-ignored there).

The conv stack is the hand-written HIP executor of hrnet_hip.py (MFMA kernels of csrc/, bf16 channels-last, BatchNorm folded), replayed
from a hipGraph per crop count (replay.ForwardReplay).  The PyTorch module of hrnet_model.py / poseresnet.py is the weight container the
executor packs (official state-dict key layout, so the published checkpoints load) and the fp32 checker; no forward runs through it.
Crop / resize / normalise and the head + arg-max decode are HIP kernels of libpam_hip.so (csrc/pam_crop.hip, csrc/pam_head.hip).
Parity with the authors' modified backend is UNPINNED (no source, weights or tests in the reference): decode follows
upstream simple-HRNet (hard arg-max, linear map through the box)."""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib, poseresnet, stages, vitpose
from .dump import DumpResults
from .replay import ForwardReplay
# Names that callers outside the package reach as hrnet.X, one line per home.  bench.py: PoseHighResolutionNet, init_random,
# fold_batchnorm, algorithmic_work; the scripts under tools/ and the tests: the rest of the model's names.
from .hrnet_model import (BN_EPS, BasicBlock, Bottleneck, HighResolutionModule, PoseHighResolutionNet, _folded_random_model,  # noqa: F401
                          algorithmic_work, count_flops, fold_batchnorm, init_random, load_folded_checkpoint)
# bench.py: measure_bf16_drift; the harness entry's smoke(): smoke_check; the other three for callers written against the old home.
from .selfcheck import drift_statistics, measure_bf16_drift, reference_decode, reference_preprocess, smoke_check  # noqa: F401


class HRNetPose(ForwardReplay):
    """Mirror of ``backend.HRPose.SimpleHRNet.HRNetPose``: ctor (c, nof_joints, checkpoint, model_name, resolution, ...),
    ``predict(person_bbox_list, batch_size, conf_threshold) -> dump_results`` (ivclabpose.py:131-132,210).
    c: the network width, 48 (HRNet-W48, the reference's configs) or 32 (HRNet-W32, usually at resolution (256, 192)); with
    model_name='PoseResNet' the ResNet depth, 50 / 101 / 152 (Simple Baselines: poseresnet.py, executor hrnet_hip.HipPoseResNet); with
    model_name='ViTPose' the variant 'B' / 'L' (or 768 / 1024) at resolution (256, 192) (vitpose.py, executor hrnet_hip.HipViTPose)."""
    WIDTHS = (32, 48)
    width = 48                  # the class default: config_for reads it (tests build objects with __new__)
    model_name = 'HRNet'        # or 'PoseResNet' (model_name 'PoseResNet' / 'poseresnet' / 'ResNet' / 'resnet'; c = depth 50 / 101 / 152),
                                # or 'ViTPose' (model_name 'ViTPose' / 'vitpose'; c = 'B' / 'L' / 768 / 1024, resolution (256, 192) only)
    depth = None
    variant = None              # ViTPose: 'B' | 'L'
    _hd_scratch = None          # head_decode's scratch, grown on demand

    def __init__(self, c, nof_joints, checkpoint_path, model_name='HRNet', resolution=(384, 288), hrpose_args=None,
                 device=0, dtype=torch.bfloat16, use_graph=True, seed=0, max_dets=16, backend='hip', graph_bucket=4,
                 shard_crops=False, group=None, autotune=False, max_crops=32, antialias=False, flip_test=False, shift_heatmap=True,
                 post_process=False, soft_beta=None, dark=False, blur_kernel=None, pose_nms=False, oks_thre=0.9, in_vis_thre=0.2,
                 box_transform='stretch', box_scale=_lib.BOX_SCALE):
        # the decode options first: a refused combination raises before anything touches a device
        self.box_transform, self.box_scale = _lib.check_box_transform(box_transform, box_scale)
        self.soft_beta, self.flip_test, self.shift_heatmap, self.post_process = soft_beta, flip_test, shift_heatmap, post_process
        self.dark, self.blur_kernel = dark, blur_kernel
        self.pose_nms, self.oks_thre, self.in_vis_thre = bool(pose_nms), float(oks_thre), float(in_vis_thre)
        if model_name in poseresnet.MODEL_NAMES:
            # simple-HRNet's second family: c is the ResNet depth (Bottleneck ResNets only; 18 / 34 are BasicBlock networks)
            if int(c) != c or int(c) not in poseresnet.DEPTHS:
                raise ValueError('HRNetPose: PoseResNet depth c=%r is not supported (PoseResNet-%s only)' % (
                    c, ' / -'.join(str(d) for d in sorted(poseresnet.DEPTHS))))
            self.model_name, self.depth, self.width = 'PoseResNet', int(c), None
        elif model_name in vitpose.MODEL_NAMES:
            # the plain vision transformer: c is the variant, 'B' / 'L' or its width 768 / 1024; one resolution (ValueError otherwise)
            self.model_name, self.depth, self.width, c = 'ViTPose', None, None, vitpose.variant_of(c)
            self.variant = c
            vitpose.check_resolution(resolution)
        elif model_name != 'HRNet':
            raise ValueError('HRNetPose: unknown model_name %r (HRNet, PoseResNet as %s, or ViTPose as %s)' % (
                model_name, ' / '.join(poseresnet.MODEL_NAMES), ' / '.join(vitpose.MODEL_NAMES)))
        assert int(nof_joints) == 17
        if model_name == 'HRNet':
            if int(c) != c or int(c) not in self.WIDTHS:
                raise ValueError('HRNetPose: width c=%r is not supported (HRNet-W%s only)' % (c, ' / -W'.join(str(w) for w in self.WIDTHS)))
            self.width = int(c)
        if not torch.cuda.is_available():
            raise RuntimeError('HRNetPose needs a GPU (the preprocessing / decode kernels are HIP only; no CPU fallback)')
        self.lib = _lib.load()
        # hrpose_args: the reference hands HRNetPose every visible GPU (gpu_args.gpus / .device, ivclabpose.py:107-111,131-132) and
        # lets the backend spread a batch over them inside one process.  Here the unit is one process per GPU.  shard_crops=True
        # (what ivclabpose passes when it runs under a torch.distributed job) makes predict() a COLLECTIVE over `group`: every rank
        # must call it with the SAME person_bbox_list; the call's crops are dealt out over the ranks, each runs its share on ITS
        # device (hrpose_args.device if given, else `device`) and ONE all-gather returns every rank the complete dump.  The default
        # is off: a merely initialised process group (a view-sharded host that calls predict() with per-rank inputs) changes nothing.
        import torch.distributed as dist
        self.group = group
        self.world, self.rank = (1, 0)
        if shard_crops and dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        dv = getattr(hrpose_args, 'device', None) if hrpose_args is not None else None
        if dv is None and isinstance(hrpose_args, dict):
            dv = hrpose_args.get('device')
        if dv is not None and torch.device(dv).type == 'cuda' and torch.device(dv).index is not None:
            device = torch.device(dv).index
        self.device = torch.device('cuda:%d' % device)
        self.resolution = tuple(resolution)
        self.dtype = dtype
        self.max_dets = max_dets
        resnet, vit = self.model_name == 'PoseResNet', self.model_name == 'ViTPose'
        family = vitpose if vit else (poseresnet if resnet else None)
        if checkpoint_path and os.path.exists(checkpoint_path):
            model = (family.load_folded_checkpoint if family else load_folded_checkpoint)(checkpoint_path, c, nof_joints)
            self.weights = checkpoint_path
        else:
            model = (family.folded_random_model if family else _folded_random_model)(c, nof_joints, seed)
            self.weights = 'random(seed=%d)' % seed
        holder = model.keypoint_head if vit else model                  # the module that owns the 1x1 head
        self.head = holder.final_layer.to(self.device).float()          # 1x1 head + decode stay float32
        self.head_w = self.head.weight.detach().reshape(int(nof_joints), -1).contiguous()     # [17][c] for k_head
        self.head_b = self.head.bias.detach().contiguous()
        holder.final_layer = nn.Identity()
        # the conv stack = the hand-written MFMA kernels of csrc/ (hrnet_hip.HipHRNet); there is no other backend in the product: the
        # PyTorch-ROCm form of the same folded module that the tests compare against lives in tests/torch_ref.py
        if backend != 'hip':
            raise ValueError("HRNetPose has one conv backend, 'hip' (got %r)" % (backend,))
        self.backend = backend
        from .hrnet_hip import HipHRNet, HipHRNetW32, HipPoseResNet, HipViTPose
        self.hip = (HipViTPose(model, self.device) if vit else HipPoseResNet(model, self.device) if resnet else
                    (HipHRNetW32 if self.width == 32 else HipHRNet)(model, self.device))
        self.in_channels = 8
        self.model = None
        # crop resize: False = plain bilinear (cv2.resize INTER_LINEAR semantics; the default: exact for boxes up to the network input, and what
        # every golden of this repository was made with); True = upstream simple-HRNet's PIL / torchvision Resize, which filters with a triangle
        # that widens with the down-scaling factor (HD Panoptic boxes taller than 384 pixels) -- csrc/pam_crop.hip
        self.antialias = bool(antialias)
        self._init_replay(use_graph, graph_bucket, max_crops)
        if self.world > 1:
            # the crop-sharded predict() is a collective that one rank cannot re-run alone: stream events.  (Ranks that SHARE a device
            # oversubscribe its hardware queues -- a gate can sit in front of its own producer: FramePipeline decides that from the
            # devices' identities, distributed.ranks_share_a_device, and calls disable_flag_sync; no collective hides in this constructor.)
            self._flag_sync_failed = True
        # autotune: the executor configuration follows the crop count (config_for); off = one configuration for every count (results of
        # different configurations differ in the last bf16 bits, and a test that compares an eager forward with a replay needs both in ONE)
        self.autotune = bool(autotune) and use_graph
        self.tuned = {}                                   # crop count -> {'choice': configuration name} of every replay captured so far
        self._kp_pinned = {}         # crop count -> two pinned host buffers for predict()'s keypoints
        self._meta_pinned = {}       # table size -> two pinned staging buffers for predict()'s per-call tables
        self.stream = torch.cuda.current_stream(self.device)

    # -- conv stack (the HIP executor; hipGraph replay per crop count: replay.ForwardReplay) -----------------------------
    def _forward(self, x, kind='heatmaps'):
        f = self.hip.features(x)                                        # (N, c, h, w) channels-last bf16
        return f if kind == 'features' else self._head(f)

    def heatmaps(self, x, slot=0):
        """x: (N,3,H,W) channels-last bf16 on the device -> (N,17,H/4,W/4) float32 (channels-last memory)."""
        return self._run(x, 'heatmaps', slot)

    def features(self, x, slot=0):
        """x as above -> (N,c,H/4,W/4) channels-last bf16: the input of ``head_decode`` (the product path: the heat-maps are
        never written).  slot: which replay instance (own static input / activations / output) -- two frames whose forwards are in
        flight at the same time (FramePipeline(pose_streams=2)) use different slots of the same weights."""
        return self._run(x, 'features', slot)

    def _head(self, f):
        n, c, h, w = f.shape
        hm = torch.empty((n, self.head_w.shape[0], h, w), dtype=torch.float32, device=f.device, memory_format=torch.channels_last)
        rc = self.lib.pam_head_heatmaps(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), n * h * w,
                                        C.c_void_p(f.data_ptr()), c, C.c_void_p(self.head_w.data_ptr()),
                                        C.c_void_p(self.head_b.data_ptr()), self.head_w.shape[0], C.c_void_p(hm.data_ptr()))
        if rc != 0:
            raise _lib.PamError('pam_head_heatmaps failed: %d' % rc)
        return hm

    def config_for(self, n):
        """Executor configuration of the n-crop forward (HipHRNet.CONFIGS).  With ``autotune`` a fixed rule from interleaved A/B runs over
        crop counts with the branch streams ordered by device-side flags (tools/ab_flags.py fused:flags_on=1 res48:flags_on=1,block2=1
        fsum:flags_on=1,fused_sums=1, end of round 5): up to 20 crops the fuse-layer sums carry their 1x1 products (k_fuse_sum, 18 launches
        fewer: 2-6 crops -3.0 ... -3.4 %, 8-16 crops -0.6 ... +0.7 %, 18 crops -1.3 %, 20 crops -1.7 %), above that they are separate launches
        (22 crops 0.0 %, 24 +0.5 %, 28 +1.6 %: the 1x1 launches hide beside the other branches' blocks and the sums are on the critical path).
        Up to 12 crops the 192- / 384-channel 3x3 layers also run with 32-channel slabs (HipHRNet.slab32: a launch of a few crops is as long
        as ONE workgroup; 2 crops -8 %, 4 -10 %, 6 -8 %, 9 -3 ... -6 %, 12 -2 %, 14 0 %, 16 +2 %).
        The 96-channel branch as streamed convolutions (round 4's choice for 8-12 crops under stream events) loses at every count now
        (+0.1 ... +5.6 %).  (Round 3 timed every configuration at the first replay of a crop count: 1.5 s per count, a choice decided by
        noise, and three dead captures per count that could never be destroyed, see _lib.new_graph.)
        HRNet-W32 has one configuration per executor setting (HipHRNetW32.CONFIGS): its class default at every crop count; so has PoseResNet
        (HipPoseResNet.CONFIGS)."""
        name = type(self.hip).config_name
        if self.autotune and self.width == 48:
            name = 'fused48_fused96_fsum_s32' if n <= self.s32_max_crops else ('fused48_fused96_fsum' if n <= self.fsum_max_crops else name)
        self.tuned[n] = {'choice': name}
        return name

    fsum_max_crops = int(os.environ.get('PAM_FSUM_MAX', '20'))      # tuning hooks of config_for's rule
    s32_max_crops = int(os.environ.get('PAM_S32_MAX', '12'))        # up to here the deep branches' 3x3 layers run with 32-channel slabs (-8 ... -10 % at 2-6 crops, -2 % at 12)

    def forward_crops(self, n):
        """Crops in the forward that serves n boxes: 2n under the flip test (n plain rows, then their n mirrors)."""
        return 2 * n if self.flip_test else n

    def input_buffer(self, n, slot=0):
        """The (N,3,H,W) channels-last bf16 tensor the preprocessing kernel writes for n boxes (N = forward_crops(n): under the flip test
        the mirrored crops follow the plain ones); the replay's own input when one exists, so no copy is needed."""
        n = self.forward_crops(n)
        g = self._graphs.get((n, 'features', slot)) or self._graphs.get((n, 'heatmaps', slot))
        if g is not None:
            return g[1]
        H, W = self.resolution
        return torch.empty((n, self.in_channels, H, W), dtype=self.dtype, device=self.device, memory_format=torch.channels_last)

    # -- HIP kernels around it -----------------------------------------------------------------------------------------
    def preprocess(self, frame_ptrs, frame_h, frame_w, view_of, boxes, out, eff=None):
        """frame_ptrs: int64 device tensor of per-view frame addresses; view_of int32 (N), boxes float32 (N,4) xywh.  out may hold more
        crops than N (a replay bucket): the extra ones repeat the last crop.  Under the flip test out (``input_buffer``) holds at least
        2N rows: N plain crops, their N mirrors, then repeats of the last mirror.
        box_transform='affine': the crops come from the boxes' effective boxes (pam_preprocess_crops_affine; the transform:
        include/pam.h), which the launch leaves in eff (N,4) float32 -- the table ``head_decode`` and the OKS-NMS take in place of
        ``boxes``; eff=None: a table of the call's own that nobody reads.  'udp': the same table through pam_preprocess_crops_udp (the
        align-corners grid).  'stretch' never touches eff."""
        H, W = self.resolution
        st = torch.cuda.current_stream(self.device).cuda_stream
        if self.uses_effective_box:
            n = int(view_of.numel())
            name = 'pam_preprocess_crops_' + self.box_transform    # _affine | _udp: one argument list
            if eff is None:
                eff = torch.empty((max(n, 1), 4), dtype=torch.float32, device=self.device)
            assert eff.is_contiguous() and eff.dtype == torch.float32 and eff.numel() >= 4 * n
            rc = getattr(self.lib, name)(C.c_void_p(st), n, int(out.shape[0]), 1 if self.flip_test else 0,
                                         C.c_void_p(frame_ptrs.data_ptr()), int(frame_h), int(frame_w),
                                         C.c_void_p(view_of.data_ptr()), C.c_void_p(boxes.data_ptr()), float(self.box_scale),
                                         H, W, int(out.shape[1]), C.c_void_p(out.data_ptr()), 1 if self.antialias else 0,
                                         C.c_void_p(eff.data_ptr()))
            if rc != 0:
                raise _lib.PamError('%s failed: %d' % (name, rc))
            return
        fn = self.lib.pam_preprocess_crops_flip if self.flip_test else self.lib.pam_preprocess_crops_ex
        rc = fn(C.c_void_p(st), int(view_of.numel()), int(out.shape[0]), C.c_void_p(frame_ptrs.data_ptr()),
                int(frame_h), int(frame_w), C.c_void_p(view_of.data_ptr()),
                C.c_void_p(boxes.data_ptr()), H, W, int(out.shape[1]), C.c_void_p(out.data_ptr()),
                1 if self.antialias else 0)
        if rc != 0:
            raise _lib.PamError('pam_preprocess_crops failed: %d' % rc)

    def decode(self, hm, view_of, slot_of, boxes, det, kp=None):
        """hm (N,17,h,w) float32 (channels-last or contiguous) -> det (C,max_dets,17,3) float64 rows (y,x,score)."""
        n, j, h, w = hm.shape
        nchw = hm.is_contiguous()
        assert nchw or hm.is_contiguous(memory_format=torch.channels_last)
        st = torch.cuda.current_stream(self.device).cuda_stream
        rc = self.lib.pam_decode_heatmaps(C.c_void_p(st), n, C.c_void_p(hm.data_ptr()), 1 if nchw else 0, h, w,
                                          C.c_void_p(view_of.data_ptr()), C.c_void_p(slot_of.data_ptr()),
                                          C.c_void_p(boxes.data_ptr()), det.shape[1], C.c_void_p(det.data_ptr()),
                                          C.c_void_p(kp.data_ptr()) if kp is not None else None)
        if rc != 0:
            raise _lib.PamError('pam_decode_heatmaps failed: %d' % rc)

    # Decode options, readable and writable as attributes (flip_test before the first capture: it doubles the forward).
    #   soft_beta      None: hard arg-max decode (the parity mode).  A float > 0: soft-arg-max with that inverse temperature
    #                  (sub-pixel keypoints = softmax(beta * heat-map)-weighted mean position; confidence = the maximum).
    #   flip_test      the official test protocol (TEST.FLIP_TEST): every forward carries each crop and its mirror, and the decode runs on
    #                  the average of the plain map and the mirrored-back, left/right-swapped map (pam_head_decode_flip).
    #   shift_heatmap  (TEST.SHIFT_HEATMAP; matters under flip_test only) the mirrored-back map moves one column to the right first.
    #   post_process   (TEST.POST_PROCESS) the arg-max moves a quarter of a cell towards the higher neighbour along each axis.
    #   dark           the DARK decode (Zhang et al., CVPR 2020; pam_head_decode_dark): the arg-max of the (merged) map moves by one Newton
    #                  step of the Gaussian-blurred map's logarithm.  Settable before or after capture: the forward keeps its size.
    #   blur_kernel    DARK's blur size, odd, 9 .. 17.  None: 17 for maps of 96 rows or more, otherwise 11 (the published DARK configs'
    #                  values for 384 x 288 and 256 x 192).
    # soft_beta with flip_test or post_process is refused (ValueError): the soft-arg-max has no merged-map form.  dark with post_process
    # or soft_beta is refused alike: each of the three is a sub-cell decode of its own.
    #   pose_nms       the protocol's last step (TEST.OKS_THRE / TEST.IN_VIS_THRE): behind the decode every pose is rescored (box score x
    #                  mean of its joint scores above in_vis_thre) and each view's duplicates are removed by greedy OKS-NMS at oks_thre, on
    #                  the device (pam_pose_nms; the rule: include/pam.h).  Plain attributes, settable at any time; composes with every
    #                  decode above (it runs after whichever ran).  Off: predict() issues exactly the launches it issued without it.
    _soft_beta, _flip_test, _post_process, _dark, _blur_kernel, shift_heatmap = None, False, False, False, None, True
    pose_nms, oks_thre, in_vis_thre = False, 0.9, 0.2
    #   box_transform  'stretch' (the default, what every golden of this repository was made with): the raw box resized to the input
    #                  whatever its shape.  'affine': the geometry the published HRNet / Simple Baselines / DARK checkpoints were trained
    #                  and evaluated with (_box2cs + get_affine_transform + warpAffine + transform_preds): the box widened to the input's
    #                  aspect about its centre, enlarged by box_scale, sampled with one scale and a zero border; the decode maps heat-map
    #                  cells back through the same effective box and pose_nms takes its areas from it (include/pam.h).  The dump's 'bbox'
    #                  stays the caller's box.  Constructor arguments (validated there: _lib.check_box_transform); the forwards keep their
    #                  size.  'stretch': every entry point makes exactly the calls it made without the option.
    #                  'udp': Unbiased Data Processing (Huang et al., CVPR 2020), the protocol of every public ViTPose checkpoint and of the
    #                  HRNet / Simple Baselines "+UDP" ones: the same effective box, but crop and heat-map are align-corners grids (pitch
    #                  We / (W - 1) and We / (hm_w - 1): pam_preprocess_crops_udp), and the decode is ALWAYS pam_head_decode_udp: with dark
    #                  the UDP form of DARK (post_dark_udp; blur_kernel as for dark), without it the plain arg-max through UDP's mapping.
    #                  post_process or soft_beta with 'udp' is refused (ValueError): the quarter-cell nudge compensates exactly the bias UDP
    #                  removes, and there is no UDP soft-arg-max.  shift_heatmap is honoured as given; the UDP configs run the flip test
    #                  with shift_heatmap=False.
    #   box_scale      _box2cs's enlargement, 1.25.  Boxes that already carry a margin (pam_track_boxes' TRACK_BOX_GROW 1.25) are
    #                  enlarged again: the two factors multiply.
    box_transform, box_scale = 'stretch', _lib.BOX_SCALE
    #   lens          (set_lens) the rig's lens table: behind the last decode of a predict() call -- and behind pose_nms, whose OKS areas
    #                  come from raw-image boxes -- the TRACKER's float64 copy of the keypoints is undistorted in place on the device
    #                  (pam_undistort_keypoints).  The host keypoints and the dump's dicts stay in raw-image pixels.  None: predict()
    #                  issues exactly the launches it issued without it.
    lens, lens_info = None, None

    @property
    def uses_effective_box(self):
        """True where crops, decode and OKS-NMS go through the effective box of include/pam.h ('affine', 'udp'), not the raw box."""
        return self.box_transform != 'stretch'

    def set_lens(self, table):
        """table: (cameras, 10) float64 host rows (_lib.lens_table), view v of a predict() call is camera v; None or all-zero
        coefficients switch the step off.  ``lens_info`` (device, 2 int32) then holds the last call's [points that could not be
        inverted and were left as they were, points looked at]."""
        table = None if table is None else _lib.check_lens(table, len(table))
        if table is None:
            self.lens, self.lens_info = None, None
            return
        self.lens = torch.from_numpy(table).to(self.device)
        self.lens_info = torch.zeros(2, dtype=torch.int32, device=self.device)

    def _decode_option(name):
        def get(self):
            return getattr(self, '_' + name)

        def put(self, value):
            value = (None if value is None else float(value)) if name == 'soft_beta' else bool(value)
            now = dict(soft_beta=self._soft_beta, flip_test=self._flip_test, post_process=self._post_process, dark=self._dark)
            now[name] = value
            if now['dark'] and (now['post_process'] or now['soft_beta'] is not None):
                raise ValueError('HRNetPose: dark cannot be combined with post_process or soft_beta (got dark=%r, post_process=%r, '
                                 'soft_beta=%r)' % (now['dark'], now['post_process'], now['soft_beta']))
            if now['soft_beta'] is not None and (now['flip_test'] or now['post_process']):
                raise ValueError('HRNetPose: soft_beta cannot be combined with flip_test or post_process (got soft_beta=%r, flip_test=%r, '
                                 'post_process=%r)' % (now['soft_beta'], now['flip_test'], now['post_process']))
            if self.box_transform == 'udp' and (now['post_process'] or now['soft_beta'] is not None):
                raise ValueError("HRNetPose: box_transform='udp' cannot be combined with post_process or soft_beta (got post_process=%r, "
                                 'soft_beta=%r)' % (now['post_process'], now['soft_beta']))
            if name == 'flip_test' and value != self._flip_test and getattr(self, '_graphs', None):
                raise RuntimeError('HRNetPose: flip_test changes the size of every forward; set it before the first capture')
            setattr(self, '_' + name, value)
        return property(get, put)
    soft_beta, flip_test, post_process = _decode_option('soft_beta'), _decode_option('flip_test'), _decode_option('post_process')
    dark = _decode_option('dark')
    del _decode_option

    @property
    def blur_kernel(self):
        return self._blur_kernel

    @blur_kernel.setter
    def blur_kernel(self, value):
        if value is not None and (int(value) != value or int(value) % 2 == 0 or not 9 <= int(value) <= 17):
            raise ValueError('HRNetPose: blur_kernel must be None or odd with 9 <= blur_kernel <= 17 (got %r)' % (value,))
        self._blur_kernel = None if value is None else int(value)

    def dark_blur_kernel(self, hm_h):
        """The blur size the DARK decode uses on a heat-map of hm_h rows: ``blur_kernel``, or by default 17 from 96 rows on, else 11."""
        return self._blur_kernel if self._blur_kernel is not None else (17 if hm_h >= 96 else 11)

    def decode_flags(self):
        """The flag word of pam_head_decode_flip for this object's options (0: the plain decode)."""
        return (1 | (2 if self.shift_heatmap else 0) if self.flip_test else 0) | (4 if self.post_process else 0)

    def head_decode(self, f, view_of, slot_of, boxes, det, kp=None, heat=None, n=None):
        """Final 1x1 convolution + arg-max decode (soft-arg-max when ``self.soft_beta`` is set) in one pass over the features f
        (N,c,h,w channels-last bf16): det rows as ``decode``; the heat-maps are written only when ``heat`` (N,17,h,w float32
        channels-last) is given.  n: decode only the first n crops of f.  Under the flip test f is the feature batch of a forward that
        ``preprocess`` filled (n plain crops, then their n mirrors: n defaults to half of f) and the decode runs on the merged maps; with
        ``post_process`` the arg-max carries the quarter-cell offset; with ``dark`` the DARK offset (pam_head_decode_dark, on the merged
        map under the flip test).  With every option off the launches are pam_head_decode's.  box_transform='udp': always
        pam_head_decode_udp (``boxes`` is the effective table), blur size dark_blur_kernel(h) with ``dark`` and 0 without."""
        nf, c, h, w = f.shape
        flags = self.decode_flags()
        n = (nf // 2 if flags & 1 else nf) if n is None else n
        assert f.is_contiguous(memory_format=torch.channels_last) and f.dtype == torch.bfloat16 and self.forward_crops(n) <= nf
        soft = self.soft_beta is not None
        need = int((self.lib.pam_head_decode_soft_scratch_bytes if soft else self.lib.pam_head_decode_scratch_bytes)(n, h, w))
        if self._hd_scratch is None or self._hd_scratch.numel() < need:
            self._hd_scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        head = (C.c_void_p(st), n, h, w, C.c_void_p(f.data_ptr()), c, C.c_void_p(self.head_w.data_ptr()),
                C.c_void_p(self.head_b.data_ptr()), self.head_w.shape[0])
        tail = (C.c_void_p(heat.data_ptr()) if heat is not None else None,
                C.c_void_p(view_of.data_ptr()), C.c_void_p(slot_of.data_ptr()), C.c_void_p(boxes.data_ptr()),
                det.shape[1], C.c_void_p(det.data_ptr()), C.c_void_p(kp.data_ptr()) if kp is not None else None,
                C.c_void_p(self._hd_scratch.data_ptr()))
        udp = self.box_transform == 'udp'
        if udp:                                           # (same scratch size as well: pam_head_decode_udp_scratch_bytes; never soft or quarter)
            rc = self.lib.pam_head_decode_udp(*(head[:2] + (n,) + head[2:] + (flags & 3, self.dark_blur_kernel(h) if self.dark else 0) + tail))
        elif soft:
            rc = self.lib.pam_head_decode_soft(*(head + (C.c_float(float(self.soft_beta)),) + tail))
        elif self.dark:                                   # (same scratch size as well: pam_head_decode_dark_scratch_bytes)
            rc = self.lib.pam_head_decode_dark(*(head[:2] + (n,) + head[2:] + (flags & 3, self.dark_blur_kernel(h)) + tail))
        elif flags:                                       # (same scratch size as the plain decode: pam_head_decode_flip_scratch_bytes)
            rc = self.lib.pam_head_decode_flip(*(head[:2] + (n,) + head[2:] + (flags,) + tail))
        else:
            rc = self.lib.pam_head_decode(*(head + tail))
        if rc != 0:
            raise _lib.PamError('pam_head_decode%s failed: %d' % ('_udp' if udp else '_soft' if soft else ('_dark' if self.dark else ('_flip' if flags else '')), rc))

    # -- the reference-shaped entry point ------------------------------------------------------------------------------
    def _call_tables(self, person_bbox_list, frame_ptr_of):
        """The small per-call tables of predict() as ONE int32 array, on the host alone (frame_ptr_of(v): the device address of view
        v's frame, asked for views that have persons) -> meta, (views, slots, boxes, cnt, S, o_ptr).  With n persons in V views:
        [view_of n | slot_of n | boxes 4n as float32 bits | per-view counts V | one pad word when V is odd | frame pointers V as int64 (0:
        a view without persons) | with pose_nms a (V, S) float32 box-score table, 1.0 where a person has no score]; S = max(max_dets,
        max(cnt)) is the slots per view of the call's buffer and o_ptr the (even) offset of the frame pointers."""
        V = len(person_bbox_list)
        views, slots, boxes, cnt, bscore = [], [], [], [0] * V, []
        for v, persons in enumerate(person_bbox_list):
            for p in persons:
                views.append(v); slots.append(cnt[v]); cnt[v] += 1; boxes.append(list(p['bbox']))     # copied: the dump is built lazily
                sc = p.get('score')
                bscore.append(1.0 if sc is None else float(sc))       # (absent or None: 1.0)
        n = len(views)
        S = max(self.max_dets, max(cnt))
        o_ptr = 6 * n + V + (V & 1)
        meta = np.empty(o_ptr + 2 * V + (V * S if self.pose_nms else 0), dtype=np.int32)
        meta[:n] = views; meta[n:2 * n] = slots
        meta[2 * n:6 * n].view(np.float32)[:] = np.asarray(boxes, dtype=np.float32).reshape(-1)
        meta[6 * n:6 * n + V] = cnt
        meta[o_ptr:o_ptr + 2 * V].view(np.int64)[:] = [frame_ptr_of(v) if cnt[v] else 0 for v in range(V)]
        if self.pose_nms:
            tab = np.ones((V, S), dtype=np.float32)
            tab[views, slots] = bscore
            meta[o_ptr + 2 * V:].view(np.float32)[:] = tab.reshape(-1)
        return meta, (views, slots, boxes, cnt, S, o_ptr)

    def _stage(self, meta):
        """meta on the device, through a pinned buffer of its own (two per size, alternating): the upload is asynchronous and the host
        goes on issuing.  Each buffer carries the event recorded behind its last upload: a host that runs more than two calls ahead of
        the GPU -- device frames, dumps dropped unread -- must not overwrite a table whose copy has not been issued to the device yet."""
        stage = self._meta_pinned.setdefault(meta.size, [])
        if len(stage) < 2:
            stage.append([torch.empty(meta.size, dtype=torch.int32).pin_memory(), None])
        stage.reverse()
        if stage[0][1] is not None:
            stage[0][1].synchronize()
        stage[0][0].numpy()[:] = meta
        m = stage[0][0].to(self.device, non_blocking=True)
        stage[0][1] = torch.cuda.Event()
        stage[0][1].record(torch.cuda.current_stream(self.device))
        return m

    def predict(self, person_bbox_list, batch_size=20, conf_threshold=0.4):
        """person_bbox_list[view] = list of dicts with 'bbox' [x, y, w, h] and 'data' (BGR uint8 HxWx3 ndarray or CUDA
        tensor) -> dump_results[view] = list of dicts {bbox, keypoints (51: x, y, score), keypoints_score (17), feature}.

        The returned list is a ``DumpResults``: besides the reference's dicts it keeps the decoded keypoints on the device in
        the tracker's input layout ((views, max_dets, 17, 3) float64 rows (y, x, score) + per-view counts), so that
        ``ivclabpose.PersonTrack_Project3DPose`` can hand them to the frame kernel without a host round trip when the caller
        passes the dump on unchanged."""
        V = len(person_bbox_list)
        if not self._arenas:
            self.max_crops = max(self.max_crops, int(batch_size))
        out = DumpResults([[] for _ in person_bbox_list])
        frames = {}
        for v, persons in enumerate(person_bbox_list):
            for p in persons:                              # the view's frame travels with its first person
                d = p['data']
                if not torch.is_tensor(d):
                    d = torch.from_numpy(np.ascontiguousarray(d))
                frames[v] = d.to(self.device, non_blocking=True).contiguous()
                break
        if not frames:
            return out
        any_frame = next(iter(frames.values()))
        fh, fw = any_frame.shape[0], any_frame.shape[1]
        meta, (views, slots, boxes, cnt, S, o_ptr) = self._call_tables(person_bbox_list, lambda v: frames[v].data_ptr())
        n = len(views)
        nms = bool(self.pose_nms)
        if nms and S > _lib.POSE_NMS_MAX:
            raise ValueError('HRNetPose.predict: pose_nms takes at most %d persons per view (got a buffer of %d slots)' % (_lib.POSE_NMS_MAX, S))
        lens = self.lens
        if lens is not None and (S > _lib.POSE_NMS_MAX or V != int(lens.shape[0])):
            raise ValueError('HRNetPose.predict: the lens table is for %d cameras and at most %d persons per view (got %d views, a buffer of '
                             '%d slots)' % (int(lens.shape[0]), _lib.POSE_NMS_MAX, V, S))
        m = self._stage(meta)
        view_of, slot_of = m[:n], m[n:2 * n]
        bx = m[2 * n:6 * n].view(torch.float32).reshape(n, 4)
        n_det = m[6 * n:6 * n + V]
        ptrs = m[o_ptr:o_ptr + 2 * V].view(torch.int64)
        det = torch.empty((V, S, 17, 3), dtype=torch.float64, device=self.device)
        kp = torch.empty((n, 17, 3), dtype=torch.float32, device=self.device)
        # box_transform='affine' / 'udp': the call's effective boxes, written by the crop launches (every row by pam_box_cs first when the crops
        # are sharded: a rank crops its share and filters all) and read by the decode and the filter in place of bx
        affine = self.uses_effective_box
        eff = torch.empty((n, 4), dtype=torch.float32, device=self.device) if affine else None
        dbx = eff if affine else bx
        lo, hi = 0, n
        if self.world > 1:                                # this rank's share of the call's crops (ordered by view, then person)
            from .distributed import crop_partition, check_same_call
            if os.environ.get('PAM_CHECK_SHARD', '0') == '1':    # debug: a rank with another crop list would hang or mis-assemble the gather
                check_same_call(n, V, self.device, self.group)
            lo, hi = crop_partition(n, self.world)[self.rank]
        host = self._pinned_kp(n)
        nms_dev = nms_host = None
        if nms:
            # the filter's outputs: [n_det_out V | keep_from V * S] int32 and pose_score (V, S) float64, with pinned host copies that
            # travel behind the keypoints' copy (they share its ring entry: a dump still pending on them is materialised first)
            nms_dev = (torch.empty(V + V * S, dtype=torch.int32, device=self.device), torch.empty((V, S), dtype=torch.float64, device=self.device),
                       m[o_ptr + 2 * V:].view(torch.float32))
            side = self._kp_last[2]
            if (V, S) not in side:
                side[(V, S)] = (torch.empty(V + V * S, dtype=torch.int32).pin_memory(), torch.empty((V, S), dtype=torch.float64).pin_memory())
            nms_host = side[(V, S)]

        def issue():
            """The device side of this call (crop -> conv stack -> head + arg-max per batch, the exchange, the copy of the keypoints to
            pinned host memory); DumpResults runs it again when a gate of one of its forwards gave up (clear_void first)."""
            kpl = kp
            if affine and self.world > 1:
                _lib.box_cs_dev(torch.cuda.current_stream(self.device).cuda_stream, bx, self.resolution[1], self.resolution[0],
                                self.box_scale, eff)
            for s in range(lo, hi, batch_size):
                e = min(hi, s + batch_size)
                k = e - s
                mp = min(batch_size, (k + self.graph_bucket - 1) // self.graph_bucket * self.graph_bucket) if batch_size >= self.graph_bucket else k
                x = self.input_buffer(mp)                    # mp > k: the crop kernel repeats the last crop into the bucket's spare rows
                self.preprocess(ptrs, fh, fw, view_of[s:e], bx[s:e], x, eff=eff[s:e] if affine else None)
                self.head_decode(self.features(x), view_of[s:e], slot_of[s:e], dbx[s:e], det, kp[s:e], n=k)
            if self.world > 1:
                from .distributed import gather_crop_keypoints
                kpl = gather_crop_keypoints(kp[lo:hi].contiguous(), n, self.world, self.rank, self.group)
                # the tracker's device-side input, rebuilt from the gathered rows: (view, slot) <- (y, x, score) as float64
                det[view_of.long(), slot_of.long()] = kpl[:, :, [1, 0, 2]].double()
            # behind the last decode of the call (the assembled buffer on every rank when the crops are sharded): the filter from the
            # ORIGINAL counts -- a redo after a void forward decodes and filters again -- with its outputs' copies right behind it, then
            # the lens step on the tracker's buffer only (kp, the host's rows, stays raw; a redo decodes again before it comes here, so
            # the in-place step never meets its own output)
            stages.after_decode(torch.cuda.current_stream(self.device).cuda_stream, det, n_det, (view_of, slot_of, dbx),
                                nms=(nms_dev[0][:V], nms_dev[0][V:], nms_dev[1], dict(score=nms_dev[2], score_strides=(S, 1), oks_thre=self.oks_thre,
                                                                                      in_vis_thre=self.in_vis_thre)) if nms else None,
                                nms_fetch=tuple(zip(nms_host, nms_dev)) if nms else (), lens=(lens, self.lens_info, None) if lens is not None else None)
            # The reference's contract is host lists -- but nothing needs them before the caller looks: the device -> host copy of the
            # keypoints is only ENQUEUED here (pinned buffer, this stream) and the per-person dicts are built at the first access of the
            # dump (DumpResults).  A loop that passes the dump straight on to PersonTrack_Project3DPose waits for the GPU once per frame
            # (behind the tracker kernel) instead of twice, and the tracker kernel is queued right behind the decode instead of after a
            # host round trip.
            host.copy_(kpl, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.device))
            return done
        out.attach_pending(det, nms_dev[0][:V] if nms else n_det, host, issue(), views, boxes, cnt)
        if nms:
            out._nms = (nms_host[0], nms_host[1], V, S)
        out._net, out._issue, out.device_eff = self, issue, eff
        import weakref
        self._kp_last[1] = weakref.ref(out)
        return out

    def _pinned_kp(self, n):
        """A pinned (n, 17, 3) float32 host buffer for the keypoints of one call; two per crop count, used alternately (a dump that is
        still pending when its buffer comes round again is materialised first).  An entry is [buffer, weak reference to the dump that
        uses it, side buffers]: the side buffers ((views, slots) -> pinned outputs of the call's pose_nms) belong to the same dump as the
        keypoints and are protected by the same rule; the dict stays empty while pose_nms is off."""
        ring = self._kp_pinned.setdefault(n, [])
        if len(ring) < 2:
            ring.append([torch.empty((n, 17, 3), dtype=torch.float32).pin_memory(), None, {}])
            ent = ring[-1]
        else:
            ent = ring[0]; ring.reverse()
            prev = ent[1]() if ent[1] is not None else None
            if prev is not None:
                prev._materialise()
        self._kp_last = ent
        return ent[0]
