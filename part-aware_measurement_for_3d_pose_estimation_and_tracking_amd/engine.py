"""How the conv stack issues a kernel: the activation memory of a forward (ActivationArena) and one launcher per C entry point of
include/pam.h (ConvEngine), shared by the pose executors of hrnet_hip.py and the person detector (yolov3.HipDarknet).  Activations are
NHWC bf16 torch tensors (channels-last); torch is used for memory and the stream only.  Every launch is hipGraph-capturable."""
import ctypes as C

import torch

from . import _lib
from .packing import down48_image, bf16_on, pointwise64_image, streamed_image


class ActivationArena(object):
    """Activations of the captured forwards of ONE replay slot: a bump allocator over one device buffer of two halves.  The executor
    calls ``epoch()`` at the start of the stem, of layer1's successor and of every HR module; an epoch allocates from the half the
    epoch before last used -- everything produced two epochs ago is dead by then (a module's tensors are read by that module and by the
    next one's first kernels only, and a full join of the branch streams lies between any two epochs).  Every capture of the slot (one
    per crop-count bucket) replays into the same buffer: they run one after the other, never at the same time.  Round 3 let every
    capture keep its own tensors: 197 GiB after a sweep over the 55 crop-count buckets of the Panoptic workload (tools/graph_memory.py).
    Without a device (``half_bytes`` None) the arena only measures: the largest epoch of a shape-only walk sizes the real one."""

    def __init__(self, device=None, half_bytes=None):
        self.half_bytes = half_bytes
        self.buf = torch.empty(2 * half_bytes, dtype=torch.uint8, device=device) if half_bytes else None
        self.half, self.off, self.peak = 1, 0, 0

    def epoch(self):
        self.half ^= 1
        self.off = 0

    def count(self, nbytes):
        self.off += (nbytes + 255) // 256 * 256
        self.peak = max(self.peak, self.off)

    def alloc(self, n, c, h, w):
        nbytes = 2 * n * c * h * w
        a = self.half * self.half_bytes + self.off
        self.count(nbytes)
        if self.off > self.half_bytes:
            raise _lib.PamError('activation arena too small: epoch needs > %d bytes' % self.half_bytes)
        return self.buf[a:a + nbytes].view(torch.bfloat16).as_strided((n, c, h, w), (h * w * c, 1, w * c, c))


class TileCfg(object):
    """The ``tile_cfg`` codes of pam_conv2d_nhwc_bf16_ex that conv() passes (include/pam.h; 0..8 name single kernels and tiles)."""
    AUTO = -1               # the library chooses; w_img is in the layout pam_conv3x3_layout() announces at call time
    CLASSIC = -2            # the classic kernels (k_conv3x3 / k_conv_igemm) and the classic image, automatic tiles
    STATED_STREAMED = -3    # automatic, the layout of w_img stated by the caller: streamed (k_conv3x3s, or PAM_E_ARG)
    STATED_CLASSIC = -4     # automatic, the layout of w_img stated by the caller: classic
    C96_48 = -5             # a 96 -> 96 layer streamed with slabs of 48 output channels (pam_conv3x3_layout_ex)
    C96_96 = -6             # ... with one slab of 96 output channels
    GEN_STREAMED = -7       # Darknet's activation codes (> 1) on the streamed kernel's general-activation form (pam_conv3x3_layout_gen)
    SLAB32 = -8             # 192- / 384-channel layers streamed with 32-channel slabs (pam_conv3x3_layout_small)


def ptr(t):
    """a tensor's device pointer as a C argument (None -> NULL)"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


class ConvEngine(object):
    """Kernel launchers shared by the pose networks (hrnet_hip.py) and the person detector (yolov3.HipDarknet), and what every executor
    built on them offers its caller (hrnet.HRNetPose): ``features``, named configurations, the activation arena's epochs."""
    count = None            # set to a dict to tally algorithmic bytes / flops of one forward (bench.py)
    prof = None             # set to a list: every launch appends dict(family, sig, bytes, flops, fn) -- fn re-issues exactly that launch
                            # (bench.py times each distinct one alone for the per-family roofline)
    arena = None            # an ActivationArena: outputs are carved from it instead of torch.empty (HRNetPose's captured replays)
    _keep = None

    def _new(self, n, c, h, w, device):
        """A fresh (n, c, h, w) channels-last bf16 activation: from the arena when one is set, else from the caching allocator (kept
        alive until the forward has been issued: another stream may still read what a freed block held)."""
        if self.arena is not None and device.type != 'meta':
            return self.arena.alloc(n, c, h, w)
        if self.arena is not None:
            self.arena.count(2 * n * c * h * w)
        y = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=device, memory_format=torch.channels_last)
        if self._keep is not None:
            self._keep.append(y)
        return y

    def _cur(self, x):
        """the current stream of x's device, as the C entry points take it"""
        return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)

    # -- the one launch path ----------------------------------------------------------------------------------------------------------------
    # A launcher allocates its outputs, then  `if self._tally(x, nbytes, flops): return y`  (a shape-only walk ends there), prepares what
    # needs device pointers, and hands the launch to _run.
    def _tally(self, x, nbytes, flops):
        """Adds one launch to ``count``; True on the meta device: nothing is launched."""
        if self.count is not None:
            self.count['bytes'] += nbytes; self.count['flops'] += flops; self.count['launches'] += 1
        return x.device.type == 'meta'

    def _run(self, x, name, call, nbytes, flops, family=None, sig=(), what=()):
        """Issues call() -- a zero-argument closure that reads the current stream when it runs, so that ``prof``'s ``fn`` re-issues
        exactly this launch later --, raises PamError('<name> failed (<rc>)<what[0] % what[1:]>') unless it returns 0, and appends the
        ``prof`` record when `family` (a string, or a callable asked after the launch) is given."""
        rc = call()
        if rc != 0:
            raise _lib.PamError('%s failed (%d)%s' % (name, rc, what[0] % tuple(what[1:]) if what else ''))
        if family is not None and self.prof is not None and x.device.type == 'cuda':
            if callable(family):
                family = family()
            self.prof.append(dict(family=family, sig=(family,) + tuple(sig), bytes=nbytes, flops=flops, fn=call))

    # -- what HRNetPose asks of an executor ---------------------------------------------------------------------------------------------
    CONFIGS = {}                # name -> the attributes that make the configuration (apply_config)
    config_name = None
    multi_stream = False
    # device-side ordering of branch streams (HipHRNet; an executor that is one chain sets flag_sync = False and never uses the rest)
    flag_sync = True            # policy: captured replays use flags (HRNetPose._run); False / PAM_FLAG_SYNC=0: stream events everywhere
    flags_on = False            # state: this forward is being issued with flags
    flag_host_err = None        # pinned int32 word that receives 1 when a gate of ANY replay times out (HRNetPose reads it before every replay)
    flag_max_us = 2000000       # a gate gives up after 2 s (a systematic deadlock, found by the check after the first replay) and raises the error word
    flag_dev_void = None        # device int32 word that receives 1 at any time-out: what the frame kernel's input guard reads (HRNetPose.void_word)
    _flag_limit = None          # the bound as a device word the gates read when they start (set_flag_limit changes it for captured gates too)
    _flags = None

    def apply_config(self, name):
        for k, v in self.CONFIGS[name].items():
            setattr(self, k, v)
        self.config_name = name

    def flag_limit(self):
        if self._flag_limit is None:
            self._flag_limit = torch.tensor([int(self.flag_max_us)], dtype=torch.int32, device=self.device)
        return self._flag_limit

    def _epoch(self):
        if self.arena is not None:
            self.arena.epoch()

    def features(self, x8):
        """x8: (N, 8, H, W) channels-last bf16 (RGB + 5 zero channels) -> the executor's (N, C, H/4, W/4) channels-last bf16 feature map."""
        self._keep = []
        return self._features(x8)

    # -- convolutions -----------------------------------------------------------------------------------------------------------------------
    pw64 = True                 # 64 -> 64 pointwise layers over >= 64 k pixels on the streaming kernel k_pw1 (ReLU or leaky)
    slab32 = False              # round 5: the 192- / 384-channel 3x3 layers with 32-channel slabs (pam_conv3x3_layout_small): for forwards of a few crops
    gen_streamed = True         # Darknet 3x3 layers with Cin 128 / 256 / 512 on k_conv3x3s<.., GEN> (False: the classic k_conv3x3)
    tile_cfg = TileCfg.AUTO
    c96_slab = 0                # 96 -> 96 3x3 layers: 0 = k_conv3x3, 48 / 96 = the streamed kernel with slabs of that many output channels
    ACT = {None: 0, False: 0, True: 1, 'linear': 0, 'relu': 1, 'leaky': 2, 'mish': 3}

    @staticmethod
    def _cached(op, key, build):
        img = op._images.get(key)
        if img is None:
            img = op._images[key] = build()
        return img

    def conv(self, op, x, res=None, relu=False, res_after_act=False, relu_from=0):
        """relu: False/True, or 'linear' | 'relu' | 'leaky' (slope 0.1); res_after_act: out = act(conv + b) + res (Darknet shortcut).
        x may be a channel slice of a wider channels-last tensor; relu_from: the activation applies to channels >= relu_from."""
        n, cin, h, w = x.shape
        T = TileCfg
        if (self.down48 and op.stride == 2 and op.kh == 3 and op.kw == 3 and op.pad == 1 and op.cin == 48 and op.cout % 48 == 0 and
                self.ACT[relu] <= 1 and not res_after_act and relu_from % 8 == 0):
            return self.conv_down48(op, x, res=res, relu=bool(self.ACT[relu]), relu_from=relu_from)
        if (self.down_s and op.stride == 2 and op.kh == 3 and op.kw == 3 and op.pad == 1 and op.cin in (96, 192) and res is None and
                self.ACT[relu] <= 1 and relu_from % 16 == 0 and self.tile_cfg == T.AUTO and
                (x.device.type == 'meta' or self.lib.pam_conv3x3s2_slab(h, w, cin, op.cout) > 0)):
            return self.conv_down_s(op, x, relu=bool(self.ACT[relu]), relu_from=relu_from)
        if (self.pw64 and op.kh == 1 and op.kw == 1 and op.stride == 1 and cin == 64 and op.cout == 64 and res is None and relu_from == 0 and
                self.ACT[relu] in (1, 2) and x.device.type != 'meta' and x.is_contiguous(memory_format=torch.channels_last) and n * h * w >= 65536):
            # a 64 -> 64 pointwise layer over many pixels (Darknet's 64 -> 32, zero-padded, at 208 x 208) is a pure stream: k_pw1
            img = self._cached(op, 'pw64', lambda: bf16_on(pointwise64_image(op.w[:, :64].float().cpu()), op._device))
            y = self._new(n, 64, h, w, x.device)
            nbytes, flops = 2 * (x.numel() + y.numel() + 64 * 64) + 4 * 64, 2 * y.numel() * 64
            self._tally(x, nbytes, flops)                          # never the meta device here (the condition above excludes it)
            self._run(x, 'pam_pointwise64_act_nhwc_bf16', lambda: self.lib.pam_pointwise64_act_nhwc_bf16(
                self._cur(x), ptr(x), ptr(img), ptr(op.bias), ptr(y), n * h * w, self.ACT[relu]), nbytes, flops)
            return y
        in_cs = cin if x.device.type == 'meta' else x.stride(3)          # channels between neighbouring pixels
        assert cin == op.cin and (x.device.type == 'meta' or (x.stride(1) == 1 and x.stride(2) == w * in_cs and x.stride(0) == h * w * in_cs)), (x.shape, op.cin)
        ho = (h + 2 * op.pad - op.kh) // op.stride + 1
        wo = (w + 2 * op.pad - op.kw) // op.stride + 1
        y = self._new(n, op.cout, ho, wo, x.device)
        # unique bytes this conv must move: input + weights + bias [+ residual] + output
        nbytes = 2 * (x.numel() + y.numel() + op.cout * op.kh * op.kw * op.cin + (y.numel() if res is not None else 0)) + 4 * op.cout
        flops = 2 * y.numel() * op.kh * op.kw * op.cin
        if self._tally(x, nbytes, flops):
            return y
        act = self.ACT[relu] | (4 if (res_after_act and res is not None) else 0)
        # the streamed kernels (k_conv3x3s / k_conv_gs) take the activation codes 0 / 1 only: leaky / shortcut-after-activation layers
        # (the detector's) ask for the classic kernels and the classic weight image
        tile_cfg = T.CLASSIC if (self.tile_cfg == T.AUTO and act > 1) else self.tile_cfg
        wimg = None
        rows3x3 = (op.kh == 3 and op.kw == 3 and op.stride == 1 and op.pad == 1 and in_cs == cin and relu_from == 0 and
                   op._w_ohwi is not None)                                # a whole-tensor 3x3 stride-1 layer that has rows-in-LDS images
        if tile_cfg == T.CLASSIC and self.gen_streamed and rows3x3 and self.lib.pam_conv3x3_layout_gen(h, w, cin, op.cout) > 0:
            # round 5: Darknet's 3x3 layers (leaky, shortcut after the activation) on the streamed kernel's general-activation instantiations
            bn = self.lib.pam_conv3x3_layout_gen(h, w, cin, op.cout)
            wimg = self._cached(op, ('gen', bn), lambda: streamed_image(op._w_ohwi, bn, op._device))
            tile_cfg = T.GEN_STREAMED
        if (wimg is None and self.slab32 and tile_cfg == T.AUTO and rows3x3 and cin in (192, 384) and
                self.lib.pam_conv3x3_layout_small(h, w, cin, op.cout) > 0):
            # forwards of a few crops: the deep branches' layers with 32-channel slabs (twice the workgroups, each half as long; bit-identical)
            wimg = self._cached(op, ('s32', 32), lambda: streamed_image(op._w_ohwi, 32, op._device))
            tile_cfg = T.SLAB32
        if wimg is None:
            wimg = op.image(h, w, classic=(tile_cfg != T.AUTO), c96_slab=self.c96_slab) if (in_cs == cin and relu_from == 0) else None
        if tile_cfg == T.AUTO and wimg is not None and op._stem is None:
            # automatic choice, but the layout of THIS image is stated (a 96 -> 96 layer: with the executor's slab width, c96_slab)
            if getattr(op, 'last_streamed', False):
                tile_cfg = {48: T.C96_48, 96: T.C96_96}.get(getattr(op, 'last_c96', 0), T.STATED_STREAMED)
            else:
                tile_cfg = T.STATED_CLASSIC

        def family():
            kind = self.lib.pam_conv_last_kernel()
            if kind == 4:
                return 'k_conv_stem %d->%d' % (3, op.cout)
            if kind in (1, 2):
                return '%s C=%d %dx%d' % ('k_conv3x3s' if kind == 2 else 'k_conv3x3', op.cin, h, w)
            return '%s %dx%d stride %d' % ('k_conv_gs' if kind == 3 else 'k_conv_igemm', op.kh, op.kw, op.stride)
        # The library refuses a call one of its kernels cannot address (csrc/pam_conv_plan.hpp).  A convolution is
        # independent per image, so a larger call is issued as slices of N, each below those frontiers, one after the other on the same
        # stream; the usual call is one slice.  conv_slice states the plan's rules once for the host: the input below 2^31 bytes -- 2^32
        # where the implicit GEMM forms no padding offset (pad 0, K a multiple of the plan's KC = 64) and no k_conv_gs tile is stated --,
        # the residual below 2^32, the output of the stated streamed forms (-7 / -8) below 2^31, pixel counts in an int.
        no_pad_offset = op.pad == 0 and (op.kh * op.kw * op.cin) % 64 == 0 and not 8 <= tile_cfg <= 12
        step = self.conv_slice(n, 2 * h * w * in_cs, 2 * ho * wo * op.cout if res is not None else 0, max(h * w, ho * wo),
                               in_frontier=2 ** 32 if no_pad_offset else 2 ** 31,
                               out_bytes=2 * ho * wo * op.cout if tile_cfg in (T.GEN_STREAMED, T.SLAB32) else 0)
        for i in range(0, n, step):
            xs, ys, rs = x[i:i + step], y[i:i + step], (None if res is None else res[i:i + step])
            self._run(x, 'pam_conv2d_nhwc_bf16', lambda xs=xs, ys=ys, rs=rs: self.lib.pam_conv2d_nhwc_bf16_ex(
                self._cur(xs), ptr(xs), ptr(op.w), ptr(wimg), ptr(op.bias), ptr(rs), ptr(ys),
                xs.shape[0], h, w, op.cin, op.cout, op.kh, op.kw, op.stride, op.pad, act, tile_cfg, in_cs, relu_from),
                nbytes * xs.shape[0] // n, flops * xs.shape[0] // n, family,
                (xs.shape[0], h, w, op.cin, op.cout, res is not None, in_cs, relu_from),
                what=(' for %s', (xs.shape, op.cout, op.kh, op.stride)))
        return y

    @staticmethod
    def conv_slice(n, in_bytes, res_bytes, pixels, in_frontier=2 ** 31, out_bytes=0):
        """Images per launch for n images of in_bytes (residual: res_bytes, 0 = none; out_bytes: only where the form bounds its output)
        and `pixels` pixels each: the largest count whose input stays below in_frontier bytes, whose residual stays below 2^32, whose
        bounded output stays below 2^31 and whose pixels stay below 2^31, as even slices."""
        cap = min((in_frontier - 1) // max(in_bytes, 1), (2 ** 32 - 1) // max(res_bytes, 1), (2 ** 31 - 1) // max(out_bytes, 1),
                  (2 ** 31 - 1) // max(pixels, 1))
        if cap >= n:
            return n
        if cap < 1:
            raise _lib.PamError('one image of this convolution exceeds the 32-bit addressing of the conv kernels')
        parts = (n + cap - 1) // cap
        return (n + parts - 1) // parts

    down_s = True               # 3x3 stride-2 layers with 96 / 192 input channels on k_down_s (csrc/pam_down.hip); False: the generic kernels

    def conv_down_s(self, op, x, relu=False, relu_from=0):
        """3x3 stride-2 convolution of a 96- / 192-channel input (channel slices allowed) through the streamed stride-2 kernel."""
        n, cin, h, w = x.shape
        in_cs = cin if x.device.type == 'meta' else x.stride(3)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = self._new(n, op.cout, ho, wo, x.device)
        nbytes = 2 * (x.numel() + y.numel() + op.cout * 9 * cin) + 4 * op.cout
        flops = 2 * y.numel() * 9 * cin
        if self._tally(x, nbytes, flops):
            return y
        assert x.stride(1) == 1 and x.stride(2) == w * in_cs and x.stride(0) == h * w * in_cs, (x.shape, x.stride())
        bn = self.lib.pam_conv3x3s2_slab(h, w, cin, op.cout)
        # op.w: [cout][k = (ky, kx, cin)]
        img = self._cached(op, ('s2', bn), lambda: streamed_image(op.w[:, :9 * cin].float().cpu().reshape(op.cout, 3, 3, cin), bn, op._device))
        self._run(x, 'pam_conv3x3s2_nhwc_bf16', lambda: self.lib.pam_conv3x3s2_nhwc_bf16(
            self._cur(x), ptr(x), in_cs, ptr(img), ptr(op.bias), ptr(y), n, h, w, cin, op.cout, 1 if relu else 0, int(relu_from)),
            nbytes, flops, 'k_down_s 3x3 stride 2 C=%d %dx%d' % (cin, h, w), (n, h, w, op.cout, in_cs, relu_from),
            what=(' for %s -> %d', tuple(x.shape), op.cout))
        return y

    down48 = True               # 3x3 stride-2 layers with 48 input channels on k_down48 (csrc/pam_down.hip); False: the generic kernels
    d48_tile = None             # (rows, cols, slab groups) instead of the library's choice (tuning)

    def conv_down48(self, op, x, res=None, relu=False, relu_from=0):
        """3x3 stride-2 convolution of a 48-channel input (a channel slice of a wider tensor is fine) through k_down48."""
        n, cin, h, w = x.shape
        assert cin == 48 and op.cin == 48 and op.stride == 2 and op.kh == 3 and op.pad == 1
        in_cs = cin if x.device.type == 'meta' else x.stride(3)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = self._new(n, op.cout, ho, wo, x.device)
        nbytes = 2 * (x.numel() + y.numel() + op.cout * 9 * 48 + (y.numel() if res is not None else 0)) + 4 * op.cout
        flops = 2 * y.numel() * 9 * 48
        if self._tally(x, nbytes, flops):
            return y
        assert x.stride(1) == 1 and x.stride(2) == w * in_cs and x.stride(0) == h * w * in_cs, (x.shape, x.stride())
        img = down48_image(op)
        t = self.d48_tile or (0, 0, 0)
        self._run(x, 'pam_conv3x3s2_c48_nhwc_bf16', lambda: self.lib.pam_conv3x3s2_c48_nhwc_bf16(
            self._cur(x), ptr(x), in_cs, ptr(img), ptr(op.bias), ptr(res), op.cout if res is not None else 0,
            ptr(y), op.cout, n, h, w, op.cout, 1 if relu else 0, int(relu_from), int(t[0]), int(t[1]), int(t[2])),
            nbytes, flops, 'k_down48 3x3 stride 2 C=48 %dx%d' % (h, w), (n, h, w, op.cout, res is not None, in_cs, relu_from),
            what=(' for %s -> %d', tuple(x.shape), op.cout))
        return y

    # -- fused blocks -----------------------------------------------------------------------------------------------------------------------
    _bb2_tiles = {}             # (C, N, H, W) -> the library's tile choice (pam_basic_block2_tile searches ~H x W candidates)
    b48_tile = None             # the same for the 48-channel block
    b96_tile = None             # (rows, cols) of the 96-channel fused block's items instead of the library's choice (tuning)

    def basic_block2(self, op, x, tile=None):
        """One BasicBlock (PackedBlock with ``wpack``: C = 32, 48 or 96) on x through the resident-weights kernel; tile = (rows, cols) or None."""
        n, c, h, w = x.shape
        assert c == op.c, (x.shape, op.c)
        y = self._new(n, c, h, w, x.device)
        nbytes, flops = 2 * (2 * x.numel() + 2 * 9 * c * c) + 8 * c, 2 * 2 * x.numel() * 9 * c
        if self._tally(x, nbytes, flops):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last)
        if tile is None and c == 96 and self.b96_tile:
            tile = tuple(self.b96_tile)
        if tile is None and c == 48 and self.b48_tile:
            tile = tuple(self.b48_tile)
        if tile is None:
            tile = self._bb2_tiles.get((c, n, h, w))
            if tile is None:
                t2 = (C.c_int32 * 2)()
                if self.lib.pam_basic_block2_tile(c, n, h, w, t2) != 0:
                    raise _lib.PamError('no resident-weights block tile for %s' % (tuple(x.shape),))
                tile = self._bb2_tiles[(c, n, h, w)] = (int(t2[0]), int(t2[1]))
        self._run(x, 'pam_basic_block2_nhwc_bf16', lambda: self.lib.pam_basic_block2_nhwc_bf16(
            self._cur(x), ptr(x), ptr(op.wpack), ptr(y), n, h, w, c, tile[0], tile[1]),
            nbytes, flops, 'k_bblock2 C=%d' % c, (n, h, w, c) + tuple(tile), what=(' for %s tile %s', tuple(x.shape), tile))
        return y

    def pointwise64(self, op, x):
        """ReLU(conv1x1 64 -> 64 (x)) as a pure stream (k_pw1)."""
        n, c, h, w = x.shape
        assert c == 64
        y = self._new(n, c, h, w, x.device)
        nbytes, flops = 2 * (2 * x.numel() + 64 * 64) + 4 * 64, 2 * n * h * w * 64 * 64
        if self._tally(x, nbytes, flops):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last)
        self._run(x, 'pam_pointwise64_relu_nhwc_bf16', lambda: self.lib.pam_pointwise64_relu_nhwc_bf16(
            self._cur(x), ptr(x), ptr(op.w), ptr(op.b), ptr(y), n * h * w), nbytes, flops, 'k_pw1 64->64 pointwise', (n, h, w))
        return y

    def stem_fused(self, op, x8):
        """(x0, y1) = stem + the first Bottleneck's conv1 in one launch (k_stem_fused): bit-identical to conv(conv1), conv(conv2), pointwise64."""
        n, c, h, w = x8.shape
        assert c == 8
        h2, w2 = ((h - 1) // 2 + 1 - 1) // 2 + 1, ((w - 1) // 2 + 1 - 1) // 2 + 1
        x0 = self._new(n, 64, h2, w2, x8.device)
        y1 = self._new(n, 64, h2, w2, x8.device)
        h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        nbytes = 2 * (x8.numel() + x0.numel() + y1.numel() + 64 * 72 + 64 * 576 + 64 * 64) + 4 * 192
        flops = 2 * n * (h1 * w1 * 64 * 72 + h2 * w2 * 64 * (576 + 64))
        if self._tally(x8, nbytes, flops):
            return x0, y1
        assert x8.is_contiguous(memory_format=torch.channels_last)
        self._run(x8, 'pam_stem_fused_nhwc_bf16', lambda: self.lib.pam_stem_fused_nhwc_bf16(
            self._cur(x8), ptr(x8), ptr(op.c1._stem), ptr(op.c1.bias), ptr(op.w2), ptr(op.b2), ptr(op.pw.w), ptr(op.pw.b),
            ptr(x0), ptr(y1), n, h, w), nbytes, flops, 'k_stem_fused stem + conv1 of layer1', (n, h, w), what=(' for %s', tuple(x8.shape)))
        return x0, y1

    def bottleneck_fused(self, op, y1, res=None, x0=None):
        """(X, y1' or None) = conv3x3 + pointwise tail of a layer1 Bottleneck in one launch (k_bneck): bit-identical to conv(c2) + bottleneck_tail.
        res: the block input (blocks 1-3); x0: the first block's 64-channel input (its downsample convolution is part of the tail)."""
        n, c, h, w = y1.shape
        t = op.tail
        assert c == 64 and (res is None) != (x0 is None) and (x0 is None) == (t.S == 1)
        assert res is None or tuple(res.shape) == (n, 256, h, w)
        X = self._new(n, 256, h, w, y1.device)
        Y = self._new(n, 64, h, w, y1.device) if t.w1 is not None else None
        M = n * h * w
        side = res if res is not None else x0
        nbytes = 2 * (y1.numel() + side.numel() + X.numel() + (Y.numel() if Y is not None else 0) + 64 * 576 + t.S * 256 * 64 +
                      (64 * 256 if t.w1 is not None else 0)) + 4 * (64 + 256 + (64 if t.w1 is not None else 0))
        flops = 2 * M * (64 * 576 + t.S * 64 * 256 + (256 * 64 if t.w1 is not None else 0))
        if self._tally(y1, nbytes, flops):
            return X, Y
        for q in (y1, side):
            assert q.is_contiguous(memory_format=torch.channels_last)
        self._run(y1, 'pam_bottleneck_fused_nhwc_bf16', lambda: self.lib.pam_bottleneck_fused_nhwc_bf16(
            self._cur(y1), ptr(y1), ptr(x0), ptr(res), ptr(op.w2), ptr(op.b2), ptr(t.w3), ptr(t.b3), ptr(t.w1),
            ptr(t.b1), ptr(X), ptr(Y), n, h, w),
            nbytes, flops, 'k_bneck 3x3 + bottleneck tail', (n, h, w, t.S, t.w1 is not None), what=(' for %s', tuple(y1.shape)))
        return X, Y

    def bottleneck_tail(self, op, y2, x0=None, res=None, tile_cfg=0):
        """X = ReLU(conv3(y2) [+ downsample(x0)] [+ res]); y1 = ReLU(conv1_next(X)) in one launch -> (X, y1 or None)."""
        n, c, h, w = y2.shape
        assert c == 64 and (x0 is None) == (op.S == 1), (y2.shape, op.S)
        X = self._new(n, 256, h, w, y2.device)
        Y = self._new(n, 64, h, w, y2.device) if op.w1 is not None else None
        M = n * h * w
        nbytes = 2 * (y2.numel() + (x0.numel() if x0 is not None else 0) + (res.numel() if res is not None else 0) + X.numel() +
                      (Y.numel() if Y is not None else 0) + op.S * 256 * 64 + (64 * 256 if op.w1 is not None else 0)) + 4 * (256 + (64 if op.w1 is not None else 0))
        flops = 2 * M * (op.S * 64 * 256 + (256 * 64 if op.w1 is not None else 0))
        if self._tally(y2, nbytes, flops):
            return X, Y
        for t in (y2, x0, res):
            assert t is None or t.is_contiguous(memory_format=torch.channels_last)
        self._run(y2, 'pam_bottleneck_tail_nhwc_bf16', lambda: self.lib.pam_bottleneck_tail_nhwc_bf16(
            self._cur(y2), ptr(y2), ptr(x0), ptr(res), ptr(op.w3), ptr(op.b3), ptr(op.w1), ptr(op.b1),
            ptr(X), ptr(Y), M, tile_cfg),
            nbytes, flops, 'k_pw2 bottleneck tail', (n, h, w, op.S, res is not None, op.w1 is not None), what=(' for %s', tuple(y2.shape)))
        return X, Y

    # -- sums, routes and pools -----------------------------------------------------------------------------------------------------------
    def upsample_add(self, base, terms, shifts, relu):
        n, c, h, w = base.shape
        y = self._new(n, c, h, w, base.device)
        nbytes = 2 * (2 * base.numel() + sum(t.numel() for t in terms))
        if self._tally(base, nbytes, 0):
            return y
        ptrs = (C.c_void_p * 3)(*[ptr(t) for t in terms] + [None] * (3 - len(terms)))
        sh = (C.c_int32 * 3)(*(list(shifts) + [0] * (3 - len(shifts))))
        cs = (C.c_int32 * 3)(*([t.stride(3) for t in terms] + [0] * (3 - len(terms))))       # terms may be channel slices
        self._run(base, 'pam_upsample_add_nhwc_bf16', lambda: self.lib.pam_upsample_add_nhwc_bf16_ex(
            self._cur(base), ptr(base), len(terms), ptrs, sh, cs, ptr(y), n, h, w, c, 1 if relu else 0),
            nbytes, 0, 'k_upsample_add', (n, h, w, c, len(terms)))
        return y

    def fuse_sum(self, op, base, plain, srcs, relu=True, tile=(0, 0), max_wg=0):
        """One output of an HR module's fuse layer in one launch (k_fuse_sum): relu(base + sum plain + sum up(conv1x1(src))).
        op: PackedUp; plain: tensors of base's shape (channel slices allowed); srcs: the coarser branches' tensors in op's order."""
        n, c, h, w = base.shape
        assert c == op.c and len(srcs) == len(op.shifts) and len(plain) <= 2
        y = self._new(n, c, h, w, base.device)
        nbytes = 2 * (2 * base.numel() + sum(t.numel() for t in plain) + sum(t.numel() for t in srcs) + sum(c * cs for cs in op.chans)) + 4 * c * len(srcs)
        flops = sum(2 * t.shape[0] * t.shape[2] * t.shape[3] * t.shape[1] * c for t in srcs)
        if self._tally(base, nbytes, flops):
            return y
        for t, sh, cs in zip(srcs, op.shifts, op.chans):
            assert tuple(t.shape) == (n, cs, h >> sh, w >> sh) and t.is_contiguous(memory_format=torch.channels_last), (t.shape, base.shape, sh)
        pp = (C.c_void_p * 2)(*[ptr(t) for t in plain] + [None] * (2 - len(plain)))
        pcs = (C.c_int32 * 2)(*([t.stride(3) for t in plain] + [0] * (2 - len(plain))))
        sp = (C.c_void_p * len(srcs))(*[ptr(t) for t in srcs])
        self._run(base, 'pam_fuse_sum_nhwc_bf16', lambda: self.lib.pam_fuse_sum_nhwc_bf16(
            self._cur(base), ptr(base), len(plain), pp, pcs, len(srcs), sp, op.c_sh, op.c_ch, op.c_w, op.c_b, ptr(y),
            n, h, w, c, 1 if relu else 0, int(tile[0]), int(tile[1]), int(max_wg)),
            nbytes, flops, 'k_fuse_sum', (n, h, w, c, len(plain), len(srcs)), what=(' for %s', tuple(base.shape)))
        return y

    def upsample_concat(self, a, b):
        """Darknet upsample(x2) + route: concat(nearest_up2(a), b) along channels."""
        n, ca, h2, w2 = a.shape
        _, cb, h, w = b.shape
        assert h == 2 * h2 and w == 2 * w2 and b.shape[0] == n, (a.shape, b.shape)
        y = self._new(n, ca + cb, h, w, a.device)
        nbytes = 2 * (a.numel() + b.numel() + y.numel())
        if self._tally(a, nbytes, 0):
            return y
        self._run(a, 'pam_upsample_concat_nhwc_bf16', lambda: self.lib.pam_upsample_concat_nhwc_bf16(
            self._cur(a), ptr(a), ptr(b), ptr(y), n, h, w, ca, cb), nbytes, 0)
        return y

    def route(self, srcs, c_out):
        """Darknet's general [route], one launch (k_route): srcs = [(tensor, first channel, channels, nearest-x2 flag)], 1 .. 4 of them;
        the slices side by side, then zeros up to c_out channels.  An x2 source is the half-size map."""
        t0, _, _, up0 = srcs[0]
        n, h, w = t0.shape[0], t0.shape[2] * (2 if up0 else 1), t0.shape[3] * (2 if up0 else 1)
        y = self._new(n, c_out, h, w, t0.device)
        nbytes = 2 * (n * h * w * sum(s[2] for s in srcs) + y.numel())
        if self._tally(t0, nbytes, 0):
            return y
        k = len(srcs)
        for t, off, cnt, up in srcs:
            assert t.is_contiguous(memory_format=torch.channels_last) and tuple(t.shape[2:]) == ((h // 2, w // 2) if up else (h, w)), (t.shape, (h, w), up)
        sp = (C.c_void_p * k)(*[ptr(s[0]) for s in srcs])
        cs = (C.c_int32 * k)(*[s[0].shape[1] for s in srcs])
        off = (C.c_int32 * k)(*[int(s[1]) for s in srcs]); cnt = (C.c_int32 * k)(*[int(s[2]) for s in srcs])
        up = (C.c_int32 * k)(*[1 if s[3] else 0 for s in srcs])
        self._run(t0, 'pam_route_concat_nhwc_bf16', lambda: self.lib.pam_route_concat_nhwc_bf16(
            self._cur(t0), k, sp, cs, off, cnt, up, ptr(y), n, h, w, c_out), nbytes, 0, 'k_route', (n, h, w, c_out, k),
            what=(' for %s -> %d channels', [tuple(s[0].shape) + tuple(s[1:]) for s in srcs], c_out))
        return y

    def maxpool(self, x, size, stride):
        """Darknet [maxpool]: pad = size - 1, out = (in + pad - size) / stride + 1, windows start at -pad / 2, taps outside the image
        do not take part (size 2 or 3, stride 1 or 2)."""
        n, c, h, w = x.shape
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        y = self._new(n, c, ho, wo, x.device)
        nbytes = 2 * (x.numel() + y.numel())
        if self._tally(x, nbytes, 0):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last), (x.shape, x.stride())
        self._run(x, 'pam_maxpool_nhwc_bf16', lambda: self.lib.pam_maxpool_nhwc_bf16(
            self._cur(x), ptr(x), ptr(y), n, h, w, c, int(size), int(stride)), nbytes, 0,
            what=(' for %s size %d stride %d', tuple(x.shape), size, stride))
        return y

    def spp(self, x, sizes):
        """YOLOv3-SPP's block, one launch: concat(pool_c(x), pool_b(x), pool_a(x), x) along channels for sizes = (a, b, c), every pool
        Darknet's stride-1 [maxpool] (odd sizes 3 .. 13, ascending; maps up to _lib.SPP_MAX_HW a side)."""
        n, c, h, w = x.shape
        a, b, cc = [int(s) for s in sizes]
        y = self._new(n, 4 * c, h, w, x.device)
        nbytes = 2 * (x.numel() + y.numel())
        if self._tally(x, nbytes, 0):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last), (x.shape, x.stride())
        self._run(x, 'pam_spp_concat_nhwc_bf16', lambda: self.lib.pam_spp_concat_nhwc_bf16(
            self._cur(x), ptr(x), ptr(y), n, h, w, c, a, b, cc), nbytes, 0, 'k_spp', (n, h, w, c, a, b, cc),
            what=(' for %s sizes %s', tuple(x.shape), (a, b, cc)))
        return y
