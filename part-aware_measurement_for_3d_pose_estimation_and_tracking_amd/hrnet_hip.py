"""HRNet-W48 / -W32, PoseResNet and ViTPose on the hand-written MFMA kernels of csrc/ (no MIOpen in the loop): the executors.

The folded (conv + bias) PyTorch module of hrnet.py / poseresnet.py is walked once into packed weights (packing.py); a forward then
issues the launches of engine.ConvEngine -- bias, residual add and ReLU fused into the convolutions' epilogues -- in the executor's
schedule: HipHRNet runs the branches of an HR module on side streams and orders them by stream events or device-side flags,
HipPoseResNet and HipViTPose (token kernels of csrc/pam_vit.hip, then PoseResNet's deconvolutions) are one dependent chain each.  The
whole forward is hipGraph-capturable."""
import ctypes as C

import torch

from . import _lib
from .engine import ActivationArena, ConvEngine, TileCfg, ptr  # noqa: F401
# the packers lived in this module before packing.py: tests and tools reach them as hrnet_hip.X
from .packing import (PackedBlock, PackedBneck, PackedConv, PackedDeconv, PackedLinear, PackedPointwise64, PackedResNetStem,  # noqa: F401
                      PackedStem, PackedTail, PackedUp, conv64_image, down48_image, streamed_image)


class HipHRNet(ConvEngine):
    merge_fuse = True           # merged first-level fuse convolutions (False: one launch per convolution)
    merge_up = True

    def __init__(self, folded_model, device):
        self.lib = _lib.load()
        self.device = device
        self._pack(folded_model, device)
        self.tile_cfg = TileCfg.AUTO
        # concurrency: the 2-4 branches of an HR module run on side streams (the coarse branches do not fill the chip)
        # equal priorities: a high-priority stream for the deep branches (whose short kernels wait for CUs behind the fused blocks' long items)
        # doubles the forward -- round 4: 4.2-4.6 ms vs 2.31 ms with side streams 2 / 2 + 3 at priority -1; all three: 2.65 ms
        self.side = [torch.cuda.Stream(device) for _ in range(3)]
        self.multi_stream = True
        self.count = None            # set to a dict to tally algorithmic bytes / flops of one forward (bench.py)

    def _pack(self, folded_model, device):
        m = folded_model
        P = lambda c, **kw: PackedConv(c, device, **kw)
        self.conv1 = P(m.conv1, pad_cin_to=8)
        self.conv2 = P(m.conv2)
        self.layer1 = [dict(c1=P(b.conv1), c2=P(b.conv2), c3=P(b.conv3),
                            down=P(b.downsample[0]) if b.downsample is not None else None) for b in m.layer1]
        # the same blocks for the fused pointwise tail: tail b = conv3_b [+ downsample_0] + residual + ReLU, then conv1_{b+1} + ReLU
        l1 = list(m.layer1)
        self.pw0 = PackedPointwise64(l1[0].conv1, device)
        self.stem = PackedStem(self.conv1, m.conv2, self.pw0, device)
        self.tails = [PackedTail(b.conv3, b.downsample[0] if b.downsample is not None else None,
                                 l1[i + 1].conv1 if i + 1 < len(l1) else None, device) for i, b in enumerate(l1)]
        self.bnecks = [PackedBneck(b.conv2, self.tails[i], device) for i, b in enumerate(l1)]
        self.t1 = [P(m.transition1[0][0]), P(m.transition1[1][0][0])]
        self.t2 = P(m.transition2[2][0][0])
        self.t3 = P(m.transition3[3][0][0])
        self.stage2 = [self._module(x) for x in m.stage2]
        self.stage3 = [self._module(x) for x in m.stage3]
        self.stage4 = [self._module(x) for x in m.stage4]

    def _module(self, hm):
        P = lambda c: PackedConv(c, self.device)
        branches = [[(P(b.conv1), P(b.conv2)) for b in br] for br in hm.branches]
        # the same blocks packed for the fused kernels (32-, 48- and 96-channel branches: one launch per block)
        fused = [[PackedBlock(b.conv1, b.conv2, self.device) for b in br] if br[0].conv1.out_channels in (32, 48, 96) else None
                 for br in hm.branches]
        fuse = []
        for i, row in enumerate(hm.fuse_layers):
            r = []
            for j, f in enumerate(row):
                if f is None:
                    r.append(None)
                elif j > i:
                    r.append(('up', P(f[0]), j - i))
                else:
                    r.append(('down', [P(step[0]) for step in f]))
            fuse.append(r)
        # the first strided conv of every down chain that starts from branch j reads the same tensor: ONE merged launch per source
        # branch (final convs of 1-conv chains first = no ReLU, then the intermediates = ReLU), the chains continue from channel slices
        merged = {}
        for j in range(len(hm.branches)):
            heads = [(i, hm.fuse_layers[i][j]) for i in range(len(hm.fuse_layers)) if i > j and hm.fuse_layers[i][j] is not None]
            if len(heads) >= 2:
                heads.sort(key=lambda t: (len(t[1]) > 1, t[0]))
                op = PackedConv.merged([f[0][0] for _, f in heads], self.device)
                parts, off = [], 0
                for i, f in heads:
                    parts.append((i, off, f[0][0].out_channels, len(f) == 1)); off += f[0][0].out_channels
                relu_from = sum(c for _, _, c, final in parts if final)
                if relu_from % 16 == 0:
                    merged[j] = dict(op=op, parts=parts, relu_from=relu_from)
        # likewise the 1x1 up-convolutions from branch j to every finer output i < j (all linear): one launch, the sums read slices
        merged_up = {}
        for j in range(len(hm.branches)):
            ups = [(i, hm.fuse_layers[i][j]) for i in range(len(hm.fuse_layers)) if i < j and hm.fuse_layers[i][j] is not None]
            if len(ups) >= 2:
                op = PackedConv.merged([f[0] for _, f in ups], self.device)
                parts, off = [], 0
                for i, f in ups:
                    parts.append((i, off, f[0].out_channels, j - i)); off += f[0].out_channels
                merged_up[j] = dict(op=op, parts=parts)
        # and the same 1x1 convolutions grouped by OUTPUT for the fused sum (k_fuse_sum: the products never reach HBM)
        fsum = []
        for i, row in enumerate(hm.fuse_layers):
            ups = [(j, row[j][0]) for j in range(len(row)) if j > i and row[j] is not None]
            fsum.append(dict(op=PackedUp([f for _, f in ups], [j - i for j, _ in ups], self.device), srcs=[j for j, _ in ups]) if ups else None)
        return dict(branches=branches, fused=fused, fuse=fuse, merged=merged, merged_up=merged_up, fsum=fsum)

    # -- network ------------------------------------------------------------------------------------------------------
    # Stream plan (stream 0 = the caller's stream; hipGraph-capturable -- pairwise event dependencies between the branch streams
    # crashed capture on ROCm 7.2, so all cross-stream ordering is a join/fork through stream 0):
    #   * stream b runs branch b of every HR module AND the fuse chains that start from branch b's output (strided-conv chains
    #     down, 1x1 convs up);
    #   * ONE join per module (a cross-stream join costs ~10 us of idle chip), then the sum of output i (one k_upsample_add over
    #     all its terms) runs on stream i, where branch i of the next module continues without further sync;
    #   * a join before every stage (the new branch's transition conv reads another stream's sum) and at the end.
    # Every tensor of a forward is kept alive until the forward has been issued (self._keep), so the caching allocator can never
    # hand a block that another stream still reads to a new tensor.
    order = (0, 1, 2, 3)        # issue order of the branches inside a module (six orders measured within 1 %)

    def _stream(self, b):
        """stream of branch b: the caller's for branch 0, side stream b - 1 otherwise"""
        return None if (b == 0 or not self.multi_stream) else self.side[b - 1]

    def _barrier(self):
        """Join and re-fork all branch streams through the caller's stream."""
        if self.multi_stream:
            cur = torch.cuda.current_stream(self.device)
            for st in self.side:
                cur.wait_stream(st)
            for st in self.side:
                st.wait_stream(cur)

    # Executor configurations the replay autotuner chooses between per crop count (HRNetPose(autotune=True)).  Round 4, interleaved A/B on
    # one device (tools/ab_crops.sh; vs round 3's grouped ring-kernel blocks, which are gone): 12 crops resident48_streamed96 -9.2 %,
    # fused48_fused96 -8.2 %; 20 crops -3.3 / -7.3 %; 40 crops -4.1 / -8.9 %; 60 crops -5.7 / -11.2 %; 112 crops -1.7 / -7.6 %; 217 crops
    # +0.3 / -6.9 %.
    CONFIGS = {
        'fused48_fused96': dict(block2=3, c96_slab=48, fused_sums=False, slab32=False),          # both fine branches: ONE fused-BasicBlock launch per block (csrc/pam_block2.hip)
        'resident48_streamed96': dict(block2=1, c96_slab=48, fused_sums=False, slab32=False),    # 48-channel branch fused, 96-channel branch as two streamed convolutions per block
        # round 5: up to 6 crops the fuse layers' 1x1 products run inside the sum launches (k_fuse_sum: 203 launches): a forward that small
        # is a chain of launch latencies (interleaved A/B: 2 crops -1.7 %, 4 -1.9 %, 6 -1.9 %, 8 -0.2 %, 12 +0.9 %, 20 +0.3 ... +1.5 %)
        'fused48_fused96_fsum': dict(block2=3, c96_slab=48, fused_sums=True, slab32=False),
        # round 5: up to 12 crops a launch of the deep branches is as long as ONE workgroup -> their 3x3 layers with 32-channel slabs (twice the
        # workgroups, each half the MFMAs and weight bytes; bit-identical): 2 crops -8 %, 4 -10 %, 6 -8 %, 9 -3 ... -6 %, 12 -2 %, 14 0 %, 16 +2 %
        'fused48_fused96_fsum_s32': dict(block2=3, c96_slab=48, fused_sums=True, slab32=True),
    }

    config_name = 'fused48_fused96'
    block2 = 3                  # bit 0: the finest branch (48 channels; 32 in HipHRNetW32) as one resident-weights fused BasicBlock launch per
                                # block (k_bblock2_48 / k_bblock2_32), bit 1: the
                                # 96-channel branch on the streamed-weights fused block (k_bblock2_96) -- csrc/pam_block2.hip
    c96_slab = 48               # 96 -> 96 layers that are NOT fused: k_conv3x3s with 48-channel slabs (0 = k_conv3x3)
    stamp = None                # diagnostics (tools/fwd_stamps.py): callable(tag) issued on the current stream at points of the schedule
    fs_cap = (0, 0, 0, 0)       # max_workgroups of output i's fused sum (0 = none).  A hint since DESIGN section 10s: only the persistent kernel,
                                # which the library still takes for a few sizes, caps its grid by it; the register-weights kernel ignores it
    fused_sums = False          # round 5: True = the fuse layers' 1x1 up-convolutions inside the sum launch (k_fuse_sum: 203 launches instead of 221,
                                # bit-identical); False = one merged 1x1 launch per source branch + k_upsample_add.  The 1x1 launches ran
                                # beside the other branches' blocks and were hidden, while the sums sit behind the module's join on the
                                # critical path.  Until DESIGN section 10s the sum was a persistent one-workgroup-per-CU kernel with the
                                # weights in LDS (20.9 vs k_upsample_add's 7.9 us for output 0 of a stage-4 module) and the fused form was
                                # within -1.5 ... +0.3 % of the un-fused one at 20 crops; now small independent workgroups keep the
                                # weights in registers (15.3 us for that output, 7.5 us for stage 2's; section 10s has the forward's A/B).
                                # Off by default; config_for turns it on by crop count.
    knock_conv2 = 0             # diagnostics: 1 = the second convolution of every un-fused BasicBlock is not issued
    knock_up = 0                # diagnostics: 1 = the coarsest branch's merged 1x1 up-convolution is not issued (its output stays uninitialised)
    knock_out = 0               # diagnostics: bit b = skip the BasicBlocks of branch b (what a free branch would be worth: tools/ab_flags.py)

    def _st(self, tag):
        if self.stamp is not None:
            self.stamp(tag)

    # -- device-side ordering of the branch streams (round 5, csrc/pam_sync.hip) ----------------------------------------------------------
    # A module ends with a full exchange (every sum reads every branch).  As stream events in a captured hipGraph that join costs 15-21 us
    # of idle chip per module (two cross-queue hops through the caller's stream); with flags the branch streams are independent chains that
    # meet through a counter in device memory: a branch's chain ends with a signal launch, a one-wave gate launch in front of every sum polls
    # the module's counter.  HRNetPose switches this on around a capture (flags_on) and checks the error word after the first replay: a
    # gate that timed out (two chains mapped onto one in-order hardware queue, a profiler serialising kernels) means a re-capture with stream events.
    # The policy switch, the state and the words HRNetPose hands over (flag_sync, flags_on, flag_host_err, ...) are ConvEngine's.

    def set_flag_limit(self, us):
        """Bound (microseconds) of every gate that STARTS after the current stream's work so far, captured ones included (tests force a
        time-out in replay k this way; 0 = give up at the first poll that finds a branch missing)."""
        self.flag_max_us = int(us)
        self.flag_limit().fill_(int(us))

    def _flag_begin(self):
        """counters + error word of ONE forward (word 0 = error); zeroed on the caller's stream in front of the fork -- inside a capture the
        fill is a node of the graph, i.e. it runs at every replay"""
        self._flags = torch.zeros(128, dtype=torch.int32, device=self.device)
        self._flag_next = 1
        if self._keep is not None:
            self._keep.append(self._flags)

    def _flag_new(self):
        i = self._flag_next
        self._flag_next += 1
        assert i < 128
        return i

    def _sig(self, i):
        rc = self.lib.pam_flag_signal(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.c_void_p(self._flags.data_ptr() + 4 * i))
        if rc != 0:
            raise _lib.PamError('pam_flag_signal failed (%d)' % rc)

    flag_per_output = False     # round 6 experiment: one counter per OUTPUT of a module (a sum waits for the blocks and chains it reads)
                                # instead of one per module (every sum waits for every branch's whole tail)

    def _sig_mask(self, base, mask):
        if not mask:
            return
        rc = self.lib.pam_flag_signal_mask(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.c_void_p(self._flags.data_ptr() + 4 * base),
                                           C.c_uint32(int(mask)))
        if rc != 0:
            raise _lib.PamError('pam_flag_signal_mask failed (%d)' % rc)

    def _gate(self, i, target, arrive=False):
        rc = self.lib.pam_flag_gate(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.c_void_p(self._flags.data_ptr() + 4 * i),
                                    int(target), C.c_void_p(self._flags.data_ptr()), C.c_void_p(self.flag_limit().data_ptr()), 1 if arrive else 0,
                                    C.c_void_p(self.flag_host_err.data_ptr()) if self.flag_host_err is not None else None,
                                    C.c_void_p(self.flag_dev_void.data_ptr()) if self.flag_dev_void is not None else None)
        if rc != 0:
            raise _lib.PamError('pam_flag_gate failed (%d)' % rc)

    def _branch_blocks(self, mod, b, blocks, x):
        """The BasicBlocks of branch b on the current stream."""
        fused = mod['fused'][b]
        if self.knock_out & (1 << b):
            return x
        if blocks and fused is not None and (self.block2 & (2 if fused[0].c == 96 else 1)):
            for op in fused:
                x = self.basic_block2(op, x)
            return x
        for c1, c2 in blocks:
            y = self.conv(c1, x, relu=True)
            if self.knock_conv2:                                      # diagnostics: half the launches AND half the work of the un-fused branches
                x = y
                continue
            x = self.conv(c2, y, res=x, relu=True)
        return x

    def _hr_module(self, mod, xs):
        """xs[b]: tensor, or ('lazy', transition op, source tensor) for a branch this stage creates.
        Stream b runs branch b's blocks and the fuse chains that hang off its output; ONE join; sum i on stream i."""
        self._epoch()
        xs = list(xs)
        fuse = mod['fuse']
        terms = [dict() for _ in fuse]
        flags = self.flags_on and self.multi_stream
        per_out = bool(flags and self.flag_per_output)
        ctail = self._flag_new() if (flags and not per_out) else None
        cbase, contrib = None, None
        if per_out:
            cbase = self._flag_next
            for _ in fuse:
                self._flag_new()
            nb = len(mod['branches'])
            contrib = [[b for b in range(nb) if b != i and b < len(row) and row[b] is not None] for i, row in enumerate(fuse)]
        for b in [q for q in self.order if q < len(mod['branches'])]:
            with torch.cuda.stream(self._stream(b)):
                x = xs[b]
                if isinstance(x, tuple):                              # transition conv runs on the new branch's own stream
                    if flags and len(x) > 3 and x[3] is not None:
                        self._gate(x[3], 1)                           # ... behind the sum it reads, which another stream issued
                    x = self.conv(x[1], x[2], relu=True)
                self._st('b%d start' % b)
                x = self._branch_blocks(mod, b, mod['branches'][b], x)
                self._st('b%d blocks' % b)
                xs[b] = x
                mg = mod['merged'].get(b) if self.merge_fuse else None
                heads = {}
                if mg is not None:                                    # first conv of all down chains from this branch in one launch
                    y = self.conv(mg['op'], x, relu=True, relu_from=mg['relu_from'])
                    heads = {i: y[:, off:off + c] for i, off, c, _ in mg['parts']}
                fmask = 15 if self.fused_sums is True else int(self.fused_sums)   # bit i: output i's sum carries its 1x1 products (k_fuse_sum)
                if per_out:                                           # the fused sums of finer outputs read this branch's blocks' output itself
                    self._sig_mask(cbase, sum(1 << i for i, row in enumerate(fuse) if i < b and b < len(row) and row[b] is not None
                                              and row[b][0] == 'up' and (fmask >> i) & 1 and mod['fsum'][i] is not None))
                mu = mod['merged_up'].get(b) if (self.merge_fuse and self.merge_up and not fmask) else None
                if mu is not None:                                    # all 1x1 up-convolutions from this branch in one launch
                    if self.knock_up and b == len(mod['branches']) - 1:   # diagnostics: what the last finisher's tail is worth
                        y = self._new(x.shape[0], mu['op'].cout, x.shape[2], x.shape[3], x.device)
                    else:
                        y = self.conv(mu['op'], x)
                    for i, off, c, sh in mu['parts']:
                        terms[i][b] = (y[:, off:off + c], sh)
                    if per_out:
                        self._sig_mask(cbase, sum(1 << i for i, _, _, _ in mu['parts']))
                for i, row in enumerate(fuse):
                    f = row[b] if b < len(row) else None
                    if f is None or (f[0] == 'up' and (mu is not None or (fmask >> i) & 1)):
                        continue
                    if f[0] == 'up':
                        terms[i][b] = (self.conv(f[1], x), f[2])
                    else:
                        t, ops = (heads[i], f[1][1:]) if i in heads else (x, f[1])
                        k0 = len(f[1]) - len(ops)
                        for k, op in enumerate(ops):
                            t = self.conv(op, t, relu=(k0 + k < len(f[1]) - 1))
                        terms[i][b] = (t, 0)
                    if per_out:
                        self._sig_mask(cbase, 1 << i)
                self._st('b%d tail' % b)
                if flags and not per_out and b >= len(fuse):
                    self._sig(ctail)                                  # a branch without an output of its own only arrives (the last module of stage 4)
        if not flags:
            self._barrier()
        self._st('join')
        # out_i = relu(x_i + sum_{j>i} up(conv1x1(x_j)) + sum_{j<i} strided-conv-chain(x_j)), terms in branch order
        out = [None] * len(fuse)
        for i in [q for q in self.order if q < len(fuse)]:
            with torch.cuda.stream(self._stream(i)):
                if per_out:
                    self._gate(cbase + i, 1 + len(contrib[i]), arrive=True)   # this output's own producers only
                elif flags:
                    self._gate(ctail, len(mod['branches']), arrive=True)   # this stream's chain is done; wait for every other branch's
                tl = [terms[i][j] for j in sorted(terms[i])]
                fs = mod['fsum'][i] if ((15 if self.fused_sums is True else int(self.fused_sums)) >> i) & 1 else None
                if fs is not None:                                    # plain (down-chain) terms + the coarser branches through their 1x1 products
                    out[i] = self.fuse_sum(fs['op'], xs[i], [t for t, _ in tl], [xs[j] for j in fs['srcs']], relu=True, max_wg=self.fs_cap[i])
                else:
                    out[i] = self.upsample_add(xs[i], [t for t, _ in tl], [sh for _, sh in tl], relu=True) if tl else torch.relu(xs[i])
                self._st('sum%d' % i)
        return out

    fuse_tail = True            # layer1: conv3 + residual + next conv1 of every Bottleneck in one launch (csrc/pam_pw.hip)
    tail_cfg = 0                # its wave-tile size (0 = automatic)
    fuse_bneck0 = True          # the first block too (its downsample fragments live in registers: they do not fit LDS beside the rest): -0.7 % at 20 crops, -1.2 % at 8
    fuse_bneck = True           # blocks 1-3 of layer1: 3x3 + pointwise tail in one launch (csrc/pam_bneck.hip; needs fuse_tail): -3.0 % at 20 crops, -2.1 % at 8, -1.6 % at 40
    fuse_stem = True            # conv1 + conv2 + layer1[0].conv1 in one launch (csrc/pam_stem.hip; needs fuse_tail): -2.2 % at 20 crops, -1.5 % at 8, -2.5 % at 40
    stop_after = None           # diagnostics (tools/stage_times.py): 'stem' | 'layer1' | 'stage2' | 'stage3' -> the forward ends there

    def _end(self, xs):
        if self.multi_stream:                                                                # final join only (no re-fork: capture must end with no forked stream)
            cur = torch.cuda.current_stream(self.device)
            for st in self.side:
                cur.wait_stream(st)
        return xs[0]

    def _features(self, x8):
        """x8: (N, 8, H, W) channels-last bf16 (RGB + 5 zero channels) -> (N, 48 | 32, H/4, W/4) channels-last bf16."""
        if self.flags_on and self.multi_stream and x8.device.type != 'meta':
            self._flag_begin()
        x = self._head(x8)
        if self.stop_after in ('stem', 'layer1'):
            return x
        return self._body(x)

    def _head(self, x8):
        """stem + layer1: one dependent chain on the caller's stream -> the (N, 256, H/4, W/4) tensor the branches start from"""
        self._epoch()
        n8, _, h8, w8 = x8.shape
        # The head's kernels, fused or not, index with 32 bits and refuse a tensor of 2^31 bytes (the 256-channel tensor at a quarter of
        # the resolution, the stem's 64 channels at half of it, the 8-channel input): > 606 crops of 384 x 288 run as even slices of
        # at most that many crops, one after the other on this stream, each through the same launches as a smaller batch.
        h4, w4 = (h8 + 3) // 4, (w8 + 3) // 4
        step, out = self.conv_slice(n8, max(h4 * w4 * 512, h8 * w8 * 16), 0, h8 * w8), None
        if step >= n8:
            return self._head_slice(x8)
        for i in range(0, n8, step):
            part = self._head_slice(x8[i:i + step])
            if out is None:
                out = self._new(n8, part.shape[1], part.shape[2], part.shape[3], x8.device)
            out[i:i + step].copy_(part)
        return out

    def _head_slice(self, x8):
        """_head for a batch every kernel can address"""
        if self.fuse_stem and self.fuse_tail and self.stop_after != 'stem':
            x0, y = self.stem_fused(self.stem, x8)
        else:
            x = self.conv(self.conv1, x8, relu=True)
            x = self.conv(self.conv2, x, relu=True)
            if self.stop_after == 'stem':
                return x
            x0, y = x, None
        if self.fuse_tail:
            # layer1 as 1 + 4 x 2 launches: conv1 of the first block, then per block the 3x3 and ONE pointwise-tail launch (conv3 + residual
            # / downsample + ReLU + the next block's conv1): the 256-channel tensor is written once and read once per block
            res = None
            if y is None:
                y = self.pointwise64(self.pw0, x0)
            for i, b in enumerate(self.layer1):
                if self.fuse_bneck and (i > 0 or self.fuse_bneck0):
                    x, y = self.bottleneck_fused(self.bnecks[i], y, res, x0 if i == 0 else None)
                else:
                    y2 = self.conv(b['c2'], y, relu=True)
                    x, y = self.bottleneck_tail(self.tails[i], y2, x0 if i == 0 else None, res, self.tail_cfg)
                res = x
        else:
            x = x0
            for b in self.layer1:
                r = x if b['down'] is None else self.conv(b['down'], x)
                y = self.conv(b['c1'], x, relu=True)
                y = self.conv(b['c2'], y, relu=True)
                x = self.conv(b['c3'], y, res=r, relu=True)
        return x

    def _new_branch(self, op, xs):
        """The lazy transition of a stage's new branch: it reads the last output of the previous stage, which stream len(xs) - 1 issued."""
        if self.flags_on and self.multi_stream:
            f = self._flag_new()
            with torch.cuda.stream(self._stream(len(xs) - 1)):
                self._sig(f)                                          # behind that stream's sum
            return ('lazy', op, xs[-1], f)
        self._barrier()
        return ('lazy', op, xs[-1])

    def _body(self, x):
        """stages 2-4 on the branch streams"""
        self._barrier()                                               # fork: branch streams must see layer1's output
        xs = [('lazy', self.t1[0], x), ('lazy', self.t1[1], x)]
        for m in self.stage2:
            xs = self._hr_module(m, xs)
        if self.stop_after == 'stage2':
            return self._end(xs)
        xs = xs + [self._new_branch(self.t2, xs)]                     # the new branch's stream reads the last sum of stage 2
        for m in self.stage3:
            xs = self._hr_module(m, xs)
        if self.stop_after == 'stage3':
            return self._end(xs)
        xs = xs + [self._new_branch(self.t3, xs)]
        for m in self.stage4:
            xs = self._hr_module(m, xs)
        return self._end(xs)


class HipHRNetW32(HipHRNet):
    """HRNet-W32 (branches of 32 / 64 / 128 / 256 channels) on the same executor.  The 32-channel branch has a fused block
    (k_bblock2_32, block2 bit 0); the 64-channel branch runs as two launches per block (its two weight sets, 144 KB, do not fit LDS
    beside a tile).  k_fuse_sum (fused_sums) and the 32-channel slabs of the 192- / 384-channel layers (slab32) have no W32 form, the
    stride-2 k_down48 / k_down_s never see a W32 input (48 / 96 / 192 channels)."""
    CONFIGS = {
        'w32_fused': dict(block2=1, c96_slab=0, fused_sums=False, slab32=False),       # one k_bblock2_32 launch per 32-channel block
        'w32_unfused': dict(block2=0, c96_slab=0, fused_sums=False, slab32=False),     # two k_conv3x3<32> launches per block (bit-identical)
    }
    config_name = 'w32_fused'
    block2 = 1
    c96_slab = 0


class HipPoseResNet(ConvEngine):
    """PoseResNet-{50,101,152} (poseresnet.PoseResNet, BN folded) on the conv stack: ONE dependent chain on the caller's stream.
    k_resnet_stem (7x7 conv + ReLU + max-pool), layer1 on HRNet's fused Bottleneck kernels (k_pw1 + k_bneck; or the un-fused
    ConvEngine.conv launches), layer2-4 on ConvEngine.conv, then the three k_deconv4x4s2.  ``features`` returns the (N, 256, H/4, W/4)
    channels-last bf16 map that HRNetPose's head + decode read.  No branch streams: the device-side flags are never used."""
    CONFIGS = {
        'resnet_fused': dict(fuse_layer1=True),       # layer1: k_pw1, then one k_bneck launch per block (3x3 + pointwise tail)
        'resnet_unfused': dict(fuse_layer1=False),    # layer1 as ConvEngine.conv launches (1x1, 3x3, 1x1 + residual, downsample)
    }
    config_name = 'resnet_fused'
    fuse_layer1 = True
    flag_sync = False           # one chain: HRNetPose captures the stream-event form only
    stop_after = None           # tests / tools: 'stem' | 'layer1' .. 'layer4' | 'deconv0' | 'deconv1' -> the forward ends there
    STAGES = ('stem', 'layer1', 'layer2', 'layer3', 'layer4', 'deconv0', 'deconv1', 'deconv2')

    def __init__(self, folded_model, device):
        self.lib = _lib.load()
        self.device = device
        self._pack(folded_model, device)
        self.count = None

    def _pack(self, m, device):
        P = lambda c: PackedConv(c, device)
        self.stem = PackedResNetStem(m.conv1, device)
        l1 = list(m.layer1)
        assert l1[0].conv1.weight.shape == (64, 64, 1, 1) and l1[0].downsample is not None
        self.layer1 = [dict(c1=P(b.conv1), c2=P(b.conv2), c3=P(b.conv3), down=P(b.downsample[0]) if b.downsample is not None else None) for b in l1]
        self.pw0 = PackedPointwise64(l1[0].conv1, device)
        self.tails = [PackedTail(b.conv3, b.downsample[0] if b.downsample is not None else None, l1[i + 1].conv1 if i + 1 < len(l1) else None, device)
                      for i, b in enumerate(l1)]
        self.bnecks = [PackedBneck(b.conv2, self.tails[i], device) for i, b in enumerate(l1)]
        self.layers = [[dict(c1=P(b.conv1), c2=P(b.conv2), c3=P(b.conv3), down=P(b.downsample[0]) if b.downsample is not None else None)
                        for b in layer] for layer in (m.layer2, m.layer3, m.layer4)]
        dl = m.deconv_layers
        self.deconvs = [PackedDeconv(dl[i], device) for i in (0, 3, 6)]

    # -- launches of csrc/pam_resnet.hip ------------------------------------------------------------------------------------------------
    def resnet_stem(self, op, x8):
        """ReLU(conv7x7 s2 (x8) + b), then max-pool 3x3 s2 p1: (N, 8, H, W) -> (N, 64, Hp, Wp) in one launch (k_resnet_stem)."""
        n, c, h, w = x8.shape
        assert c == 8
        hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
        y = self._new(n, 64, hp, wp, x8.device)
        nbytes = 2 * (x8.numel() + y.numel() + 64 * 7 * 7 * 8) + 4 * 64
        flops = 2 * n * hc * wc * 64 * 3 * 49                           # counted at the 3 real input channels
        if self._tally(x8, nbytes, flops):
            return y
        assert x8.is_contiguous(memory_format=torch.channels_last)
        self._run(x8, 'pam_resnet_stem_nhwc_bf16', lambda: self.lib.pam_resnet_stem_nhwc_bf16(
            self._cur(x8), ptr(x8), ptr(op.frag), ptr(op.bias), ptr(y), n, h, w),
            nbytes, flops, 'k_resnet_stem 7x7 s2 + max-pool', (n, h, w), what=(' for %s', tuple(x8.shape)))
        return y

    def deconv(self, op, x, relu=True):
        """ReLU(ConvTranspose2d 4x4 s2 p1 (x) + b): (N, Cin, H, W) -> (N, Cout, 2H, 2W) in one launch (k_deconv4x4s2, all four parities)."""
        n, cin, h, w = x.shape
        assert cin == op.cin, (x.shape, op.cin)
        y = self._new(n, op.cout, 2 * h, 2 * w, x.device)
        nbytes = 2 * (x.numel() + y.numel() + op.cin * op.cout * 16) + 4 * op.cout
        flops = 2 * y.numel() * op.cin * 4                               # 4 live taps per output pixel
        if self._tally(x, nbytes, flops):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last)
        self._run(x, 'pam_deconv4x4s2_nhwc_bf16', lambda: self.lib.pam_deconv4x4s2_nhwc_bf16(
            self._cur(x), ptr(x), ptr(op.w), ptr(op.bias), ptr(y), n, h, w, op.cin, op.cout, 1 if relu else 0),
            nbytes, flops, 'k_deconv4x4s2 %d->%d' % (op.cin, op.cout), (n, h, w, op.cin, op.cout, bool(relu)), what=(' for %s', tuple(x.shape)))
        return y

    # -- network ------------------------------------------------------------------------------------------------------------------------
    def _layer1(self, x0):
        n, _, h, w = x0.shape
        # the fused bottleneck indexes its 256-channel tensors with 32 bits and refuses 2^31 bytes; a larger batch takes the un-fused
        # convolutions, which conv() issues as slices of N below the generic kernels' own 32-bit frontiers
        small = n * h * w * 512 < 2 ** 31
        if self.fuse_layer1 and small:
            y = self.pointwise64(self.pw0, x0)                          # the stem's epoch: block 0 reads x0 and y from the other half
            res = None
            for i in range(len(self.layer1)):
                self._epoch()
                x, y = self.bottleneck_fused(self.bnecks[i], y, res, x0 if i == 0 else None)
                res = x
            return x
        x = x0
        for b in self.layer1:
            x = self._bottleneck(b, x)
        return x

    def _bottleneck(self, b, x):
        self._epoch()                                                   # a block reads its input (previous epoch) and writes this one's
        r = x if b['down'] is None else self.conv(b['down'], x)
        y = self.conv(b['c1'], x, relu=True)
        y = self.conv(b['c2'], y, relu=True)
        return self.conv(b['c3'], y, res=r, relu=True)

    def _features(self, x8):
        """x8: (N, 8, H, W) channels-last bf16 (RGB + 5 zero channels) -> (N, 256, H/4, W/4) channels-last bf16."""
        if x8.device.type == 'meta' and self.arena is not None and self.arena.buf is None:
            # a measuring arena (HRNetPose._arena_for sizes the activation arena ONCE, before the first capture): the largest epoch of every
            # configuration -- the un-fused layer1 holds 640 channels at H/4 in one epoch, the fused one 320
            saved = self.config_name
            try:
                for name in self.CONFIGS:
                    self.apply_config(name)
                    y = self._chain(x8)
            finally:
                self.apply_config(saved)
            return y
        return self._chain(x8)

    def _chain(self, x8):
        stop = self.stop_after
        self._epoch()
        x = self.resnet_stem(self.stem, x8)
        if stop == 'stem':
            return x
        x = self._layer1(x)
        if stop == 'layer1':
            return x
        for k, layer in enumerate(self.layers):
            for b in layer:
                x = self._bottleneck(b, x)
            if stop == 'layer%d' % (k + 2):
                return x
        for k, op in enumerate(self.deconvs):
            self._epoch()
            x = self.deconv(op, x, relu=True)
            if stop == 'deconv%d' % k:
                return x
        return x


class HipViTPose(ConvEngine):
    """ViTPose-B / -L (vitpose.ViTPose, BN folded) on the token kernels of csrc/pam_vit.hip: ONE dependent chain on the caller's stream.
    A token tensor (N T rows of D channels) is the channels-last tensor (N, D, 16, 12), so every activation comes from the arena like a
    feature map.  Patch embedding (+ position table), then per block LayerNorm, qkv, attention, proj + residual, LayerNorm, fc1 + GELU,
    fc2 + residual -- all four linears through pam_vit_linear_bf16 --, the last LayerNorm and the two k_deconv4x4s2 of the head.
    ``features`` returns the (N, 256, 64, 48) channels-last bf16 map that HRNetPose's head + decode read.  No branch streams."""
    CONFIGS = {'vit': dict()}
    config_name = 'vit'
    flag_sync = False           # one chain: HRNetPose captures the stream-event form only
    stop_after = None           # tests / tools: a name of STAGES -> the forward ends there
    STAGES = ('patch',) + tuple('block%d' % i for i in range(12)) + ('norm', 'deconv0', 'deconv1')     # ViTPose-B's; an object holds its own

    def __init__(self, folded_model, device):
        self.lib = _lib.load()
        self.device = device
        self._pack(folded_model, device)
        self.count = None

    def _pack(self, m, device):
        from . import vitpose
        bb = m.backbone
        self.dim, self.heads, self.depth = m.dim, m.heads, m.depth
        self.STAGES = ('patch',) + tuple('block%d' % i for i in range(m.depth)) + ('norm', 'deconv0', 'deconv1')
        self.patch = PackedLinear(vitpose.patch_matrix(bb.patch_embed.proj), None, device)
        self.pos_bias = vitpose.position_bias(bb).to(device).contiguous()
        L = lambda lin: PackedLinear(lin.weight, lin.bias, device)
        N = lambda ln: (ln.weight.detach().float().to(device).contiguous(), ln.bias.detach().float().to(device).contiguous(), float(ln.eps))
        self.blocks = [dict(n1=N(b.norm1), qkv=L(b.attn.qkv), proj=L(b.attn.proj), n2=N(b.norm2), fc1=L(b.mlp.fc1), fc2=L(b.mlp.fc2))
                       for b in bb.blocks]
        self.last_norm = N(bb.last_norm)
        dl = m.keypoint_head.deconv_layers
        self.deconvs = [PackedDeconv(dl[i], device) for i in (0, 3)]

    deconv = HipPoseResNet.deconv

    # -- launches of csrc/pam_vit.hip ---------------------------------------------------------------------------------------------------
    def patch_embed(self, op, pos_bias, x8):
        """Conv2d(3, D, 16, stride 16, padding 2) + position table: (N, 8, H, W) -> the token tensor (N, D, H / 16, W / 16)."""
        n, c, h, w = x8.shape
        assert c == 8 and h % 16 == 0 and w % 16 == 0, tuple(x8.shape)
        d, t = op.n, (h // 16) * (w // 16)
        y = self._new(n, d, h // 16, w // 16, x8.device)
        nbytes = 2 * (x8.numel() + y.numel() + d * op.k) + 4 * t * d
        flops = 2 * n * t * d * 3 * 256                                 # counted at the 3 real input channels
        if self._tally(x8, nbytes, flops):
            return y
        assert x8.is_contiguous(memory_format=torch.channels_last) and tuple(pos_bias.shape) == (t, d)
        self._run(x8, 'pam_vit_patch_embed_bf16', lambda: self.lib.pam_vit_patch_embed_bf16(
            self._cur(x8), ptr(x8), ptr(op.w), ptr(pos_bias), ptr(y), n, h, w, d),
            nbytes, flops, 'k_vit_gemm patch embedding', (n, h, w, d), what=(' for %s', tuple(x8.shape)))
        return y

    def layernorm(self, p, x):
        """LayerNorm over the channels of every token; p = (gamma, beta, eps)."""
        n, d, h, w = x.shape
        y = self._new(n, d, h, w, x.device)
        nbytes, flops = 2 * 2 * x.numel() + 8 * d, 8 * x.numel()
        if self._tally(x, nbytes, flops):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last)
        self._run(x, 'pam_vit_layernorm_bf16', lambda: self.lib.pam_vit_layernorm_bf16(
            self._cur(x), ptr(x), ptr(p[0]), ptr(p[1]), ptr(y), n * h * w, d, C.c_float(p[2])),
            nbytes, flops, 'k_vit_layernorm D=%d' % d, (n * h * w, d), what=(' for %s', tuple(x.shape)))
        return y

    def linear(self, op, x, res=None, gelu=False):
        """bf16(act(x W^T + b) [+ res]) per token: (N, K, h, w) -> (N, N', h, w)."""
        n, k, h, w = x.shape
        assert k == op.k and not (gelu and res is not None), (x.shape, op.k)
        y = self._new(n, op.n, h, w, x.device)
        nbytes = 2 * (x.numel() + y.numel() + op.n * op.k + (y.numel() if res is not None else 0)) + 4 * op.n
        flops = 2 * y.numel() * op.k
        if self._tally(x, nbytes, flops):
            return y
        assert x.is_contiguous(memory_format=torch.channels_last) and (res is None or (res.shape == y.shape and res.is_contiguous(memory_format=torch.channels_last)))
        self._run(x, 'pam_vit_linear_bf16', lambda: self.lib.pam_vit_linear_bf16(
            self._cur(x), ptr(x), ptr(op.w), ptr(op.bias), ptr(res), ptr(y), n * h * w, op.k, op.n, 1 if gelu else 0),
            nbytes, flops, 'k_vit_gemm %d->%d' % (op.k, op.n), (n * h * w, op.k, op.n, res is not None, bool(gelu)),
            what=(' for %s -> %d', tuple(x.shape), op.n))
        return y

    def attention(self, qkv, heads):
        """softmax(Q K^T / 8) V per crop and head: (N, 3 heads 64, h, w) -> (N, heads 64, h, w)."""
        n, c, h, w = qkv.shape
        assert c == 3 * heads * 64, (qkv.shape, heads)
        t = h * w
        y = self._new(n, heads * 64, h, w, qkv.device)
        nbytes, flops = 2 * (qkv.numel() + y.numel()), 2 * 2 * n * heads * t * t * 64
        if self._tally(qkv, nbytes, flops):
            return y
        assert qkv.is_contiguous(memory_format=torch.channels_last)
        self._run(qkv, 'pam_vit_attention_bf16', lambda: self.lib.pam_vit_attention_bf16(self._cur(qkv), ptr(qkv), ptr(y), n, t, heads),
                  nbytes, flops, 'k_vit_attention T=%d' % t, (n, t, heads), what=(' for %s', tuple(qkv.shape)))
        return y

    # -- network ------------------------------------------------------------------------------------------------------------------------
    def block(self, b, x):
        """One pre-norm block: an arena epoch of its own (it reads the previous block's output from the other half)."""
        self._epoch()
        a = self.attention(self.linear(b['qkv'], self.layernorm(b['n1'], x)), self.heads)
        x = self.linear(b['proj'], a, res=x)
        return self.linear(b['fc2'], self.linear(b['fc1'], self.layernorm(b['n2'], x), gelu=True), res=x)

    def _features(self, x8):
        """x8: (N, 8, 256, 192) channels-last bf16 (RGB + 5 zero channels) -> (N, 256, 64, 48) channels-last bf16."""
        stop = self.stop_after
        self._epoch()
        x = self.patch_embed(self.patch, self.pos_bias, x8)
        if stop == 'patch':
            return x
        for i, b in enumerate(self.blocks):
            x = self.block(b, x)
            if stop == 'block%d' % i:
                return x
        self._epoch()
        x = self.layernorm(self.last_norm, x)
        if stop == 'norm':
            return x
        for k, op in enumerate(self.deconvs):
            self._epoch()
            x = self.deconv(op, x, relu=True)
            if stop == 'deconv%d' % k:
                return x
        return x
