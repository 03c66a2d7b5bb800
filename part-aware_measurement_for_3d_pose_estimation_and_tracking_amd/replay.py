"""The captured-forward cache of a pose network: one hipGraph replay per (crop count, kind, slot), the capture-time race between
device-side flags and stream events, the void protocol of a gate that gave up, activation arenas, graph pools and crop-count buckets."""
import os

import torch

from . import _lib


class ForwardReplay(object):
    """Base class of ``hrnet.HRNetPose``: runs ``_forward(x, kind)`` eagerly or as a cached hipGraph replay.

    The subclass provides ``_forward(x, kind)`` (kind: 'features' or 'heatmaps'), ``hip`` (the executor: hrnet_hip.HipHRNet and its
    kin), ``device``, ``dtype``, ``resolution``, ``in_channels``, ``config_for(n)``, ``forward_crops(n)`` and ``input_buffer(n, slot)``,
    and calls ``_init_replay`` once ``hip`` and ``device`` exist.

    No capture ever loses its last reference while the object lives: destroying a captured multi-stream graph corrupts the runtime's
    heap (_lib.new_graph), so a capture that leaves the cache is parked on ``_dead_graphs``."""
    flag_margin = float(os.environ.get('PAM_FLAG_MARGIN', '0.01'))    # flags must win the capture-time race by this fraction to be kept
    flag_race_rounds = int(os.environ.get('PAM_FLAG_RACE_ROUNDS', '5'))
    _flag_sync_failed = False    # True: this object orders its branch streams by stream events from now on (disable_flag_sync)

    def _init_replay(self, use_graph, graph_bucket, max_crops):
        self.use_graph = use_graph
        self.flag_synced = {}        # (crops, kind, slot) -> the replay orders its branch streams by device-side flags (False: stream events)
        # a gate that times out in ANY replay stores 1 here (pinned host memory, csrc/pam_sync.hip): read before every replay
        self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._flag_host_np = self._flag_host.numpy()
        self.hip.flag_host_err = self._flag_host
        # ... and 1 in this DEVICE word, which the frame kernel reads in front of every frame (pam_set_input_guard): keypoints decoded from a
        # forward whose gate gave up never reach the tracker state, whoever consumes them and however far the host has run ahead.  The
        # consumers recover (DumpResults / ivclabpose: the forward is re-run with stream events; FramePipeline.results raises FrameVoid
        # with the frame to resume from) -- check_void / clear_void below.
        self.void_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.hip.flag_dev_void = self.void_word
        self.hip.flag_limit()                             # (the gates' bound as a device word: made here, never inside a capture)
        self.void_pending = False    # a time-out has been seen and the forwards since have not been re-run yet
        self.flag_timeouts = 0       # time-outs seen by this object after the capture-time checks
        self.flag_timing = {}        # crop count -> the race of its first flagged capture against stream events: dict(ms={mode: (flags, events)}, kept={mode: bool})
        self._alt = {}               # (crops, kind, slot) -> {mode: (graph, static_in, static_out)} when both forms exist
        self.flag_race = 'serial'    # which timing of that race picks a replay's form: 'serial' (one replay at a time: predict()'s use), 'throughput' (back to back: FramePipeline); None = no race, flags stay
        self._dead_graphs = []       # captures that lost that race or failed the flag check (never destroyed: _lib.new_graph)
        self.captures = 0            # hipGraph captures made so far (a capture inside a frame is a stall of hundreds of ms: warm())
        # predict() pads a batch to the next multiple of graph_bucket crops (repeating its last box; the padded rows are not
        # decoded): a sequence whose person count wanders then replays a handful of captured graphs instead of capturing one
        # per count (a capture is a multi-100-ms stall); 1 = exact batch sizes
        self.graph_bucket = max(1, int(graph_bucket)) if use_graph else 1
        self._graphs = {}
        # activations of the captured forwards: one arena per replay slot, sized for max_crops crops per forward (a larger forward gets a
        # new, larger arena; the captures made before keep theirs) -- hrnet_hip.ActivationArena
        self.max_crops = int(max_crops)
        self._arenas = {}
        self._arena_bytes_per_crop = None
        self._pools = {}             # graph memory pool per replay slot: graphs of ONE slot replay one after the other and may share
                                     # intermediates; the two slots of FramePipeline(pose_streams=2) replay concurrently and must not

    def _run(self, x, kind, slot=0):
        assert self.flag_race in (None, 'serial', 'throughput'), self.flag_race
        if not self.use_graph:
            with torch.no_grad():
                return self._forward(x, kind)
        key = (x.shape[0], kind, slot)
        self.check_void()                                  # a time-out of an EARLIER replay: stream events from here on (before any capture)
        if key not in self._graphs:
            self._build(x, kind, slot)
        if self.check_void() and key not in self._graphs:  # (a replay of the capture-time race gave up: the switch to stream events has
            return self._run(x, kind, slot)                #  replaced or dropped this forward's flagged capture)
        graph, static_in, static_out = self._pick(key)
        if static_in.data_ptr() != x.data_ptr():
            static_in.copy_(x)
        graph.replay()
        return static_out

    def _pick(self, key):
        """The cached capture a replay of `key` uses.  Where both forms of the forward exist: the one that is faster the way this
        object is used now (flag_race)."""
        alt = self._alt.get(key)
        if alt is None:
            return self._graphs[key]
        return alt['flags' if self.flag_timing[key[0]]['kept'][self.flag_race or 'throughput'] else 'events']

    def _build(self, x, kind, slot):
        """Capture the forward of x's crop count into the cache: two eager forwards on a side stream, the capture, and -- when it orders
        its branch streams by device-side flags -- one checked replay, the same forward ordered by stream events beside it, and the
        race between the two."""
        n = x.shape[0]
        key = (n, kind, slot)
        self.hip.apply_config(self.config_for(n))
        self.hip.arena = self._arena_for(n, slot)
        other = self._graphs.get((n, 'features' if kind == 'heatmaps' else 'heatmaps', slot))
        static_in = other[1] if other is not None else torch.empty_like(x)     # one input buffer per batch size and slot
        static_in.copy_(x)
        with torch.no_grad():
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._forward(static_in, kind)
            torch.cuda.current_stream(self.device).wait_stream(s)
            raced = self.flag_timing.get(n)
            want_flags = self._flag_sync_ok() and (raced is None or raced['kept']['serial'] or raced['kept']['throughput'])
            graph, static_out, flags = self._capture(static_in, kind, slot, want_flags)
            alt = None
            if flags is not None and not self._flags_held(graph, flags):
                # a gate timed out (two branch chains on one in-order hardware queue, a profiler that serialises kernels) -> this object
                # goes back to stream events, for this and every later capture (the flagged capture stays alive, never destroyed)
                self._flag_sync_failed = True
                self._dead_graphs.append((graph, static_out, flags))
                graph, static_out, flags = self._capture(static_in, kind, slot, False)
            elif flags is not None and self.flag_race:
                # every flagged capture has the same forward ordered by stream events beside it, and both are timed both ways: 'throughput'
                # = replays back to back (FramePipeline: the host runs a frame ahead; flags win by 1-6 %), 'serial' = one replay at a
                # time (the synchronous drop-in surface: the runtime enqueues a flagged graph chain by chain, so a new branch's first
                # kernel is enqueued ~200 us after the caller stream's, which only back-to-back replays hide -- small forwards lose
                # more to that than the joins cost).  A replay uses the form that is faster in the object's CURRENT mode (_pick).
                # Under rocprofv3's kernel tracing the gates wait ~1 ms each without ever timing out: flags lose every race.
                ev_graph, ev_out, _ = self._capture(static_in, kind, slot, False)
                if raced is None:
                    # interleaved rounds, the median of each form; flags are kept only where they win by more than flag_margin
                    # (round 5 decided from 4 replays with a 1.7 % margin: not reproducible from box to box)
                    t = {m: self._race(graph, ev_graph, m) for m in ('serial', 'throughput')}
                    raced = self.flag_timing[n] = dict(ms=t, kept={m: t[m][0] <= (1.0 - self.flag_margin) * t[m][1] for m in t})
                alt = {'flags': (graph, static_in, static_out), 'events': (ev_graph, static_in, ev_out)}
            self.captures += 1
        self.hip.arena = None
        self._graphs[key] = (graph, static_in, static_out)
        self._alt[key] = alt
        self.flag_synced[key] = flags is not None if alt is None else bool(raced['kept'][self.flag_race])

    def _flags_held(self, graph, flags):
        """The flagged replay once, then its error word: did every gate see its flag?  Resets the host and device words: a time-out of
        THIS replay is dealt with by the caller (its output is discarded)."""
        graph.replay()
        torch.cuda.synchronize(self.device)
        ok = int(flags[0].item()) == 0
        self._flag_host_np[0] = 0
        if not self.void_pending:
            self.void_word.zero_()
        return ok

    def _race(self, graph, ev_graph, mode):
        """(ms flags, ms events) of one forward captured both ways: flag_race_rounds interleaved rounds of 4 replays each (20 replays per
        form), the median round of each."""
        a, b = [], []
        for _ in range(max(1, self.flag_race_rounds)):
            a.append(self._replay_ms(graph, mode)); b.append(self._replay_ms(ev_graph, mode))
        a.sort(); b.sort()
        return a[len(a) // 2], b[len(b) // 2]

    def _replay_ms(self, graph, mode='serial', reps=4):
        """ms per replay of a captured forward (events on the caller's stream): 'serial' = the shortest of `reps` replays issued one at a
        time, 'throughput' = `reps` replays issued back to back."""
        if mode == 'throughput':
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps
        best = float('inf')
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); graph.replay(); e1.record(); e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    def disable_flag_sync(self):
        """From now on every replay orders its branch streams by stream events; flagged captures leave the cache (kept alive, never
        destroyed) and are re-captured at their next use.  For callers that keep two forwards in flight at the same time: the gates
        of two flagged replays can block each other's hardware queues (FramePipeline(pose_streams=2) calls this)."""
        self._flag_sync_failed = True
        for key in list(self.flag_synced):
            alt = self._alt.pop(key, None)
            if alt is not None:                            # the stream-event form of this forward exists already
                self._dead_graphs.append(alt['flags']); self._graphs[key] = alt['events']; self.flag_synced[key] = False
            elif self.flag_synced[key]:
                self._dead_graphs.append(self._graphs.pop(key))
                self.flag_synced.pop(key)

    def drop_captures(self):
        """Empty the cache: every forward is captured again at its next use (a test that changes the executor configuration under a
        live object).  The captures themselves stay alive on ``_dead_graphs``."""
        self._dead_graphs.extend(self._graphs.values())
        self._dead_graphs.extend(v for v in self._alt.values() if v is not None)
        self._graphs.clear(); self._alt.clear(); self.flag_synced.clear(); self.flag_timing.clear()

    def check_void(self):
        """Has a gate of a replay given up since the last clear_void()?  (One read of a pinned host word: free.)  The first sighting
        switches the object to stream events for every later forward; the forwards replayed between the time-out and the switch are
        void -- their consumers on the device skipped them (void_word), and whoever holds their inputs re-runs them after clear_void()."""
        if self._flag_host_np[0] != 0:
            self._flag_host_np[0] = 0
            if not self.void_pending:
                self.flag_timeouts += 1
                import warnings
                warnings.warn('a device-side gate of a captured HRNet forward timed out (flag_max_us = %d us; a second process on this GPU?): '
                              'the affected forwards are re-run and this object orders its branch streams by stream events from now on'
                              % self.hip.flag_max_us, RuntimeWarning)
            self.void_pending = True
            self.disable_flag_sync()
        return self.void_pending

    def clear_void(self):
        """Call with the device's work drained or about to be re-issued: lowers the device word (the frame kernel applies frames again) and
        the pending mark.  Synchronises the device."""
        torch.cuda.synchronize(self.device)
        self._flag_host_np[0] = 0
        self.void_word.zero_()
        torch.cuda.synchronize(self.device)
        self.void_pending = False

    def _flag_sync_ok(self):
        return bool(self.hip.flag_sync) and not self._flag_sync_failed and os.environ.get('PAM_FLAG_SYNC', '1') != '0'

    def _capture(self, static_in, kind, slot, flags_on):
        """Capture one forward on static_in; flags_on: the branch streams are ordered by device-side flags (hrnet_hip.HipHRNet)."""
        self.hip.flags_on = bool(flags_on)
        try:
            graph = _lib.new_graph()
            with torch.cuda.graph(graph, pool=self._pool_of(slot)):
                static_out = self._forward(static_in, kind)
            flags = self.hip._flags if flags_on else None
        finally:
            self.hip.flags_on = False
            self.hip._flags = None
        return graph, static_out, flags

    def _arena_for(self, n, slot):
        """The activation arena the n-crop capture of `slot` allocates from (created / replaced by a larger one on demand)."""
        from .hrnet_hip import ActivationArena
        if self._arena_bytes_per_crop is None:            # largest epoch of a one-crop forward, from a shape-only walk of this executor
            hip, probe = self.hip, ActivationArena()
            saved = (hip.multi_stream, hip.arena, hip.count, hip.prof)
            hip.multi_stream, hip.arena, hip.count, hip.prof = False, probe, None, None
            try:
                H, W = self.resolution
                hip._features(torch.empty((1, self.in_channels, H, W), dtype=self.dtype, device='meta').contiguous(memory_format=torch.channels_last))
            finally:
                hip.multi_stream, hip.arena, hip.count, hip.prof = saved
            self._arena_bytes_per_crop = probe.peak       # per tensor rounded up to 256 B: n crops need <= n times this
        ar = self._arenas.get(slot)
        need = n * self._arena_bytes_per_crop
        if ar is None or ar.half_bytes < need:
            # first arena: twice the first forward's need, at most max_crops crops (a rig of 31 views x 16 detections would otherwise
            # reserve 18 GB per replay slot for frames of 40 crops); warm() captures its largest bucket first and so sizes the arena once.
            # A forward beyond the arena gets a new one of TWICE its need (the captures made so far keep the old one: their kernels hold
            # its addresses, and a captured graph is never destroyed, _lib.new_graph): a crop count that creeps upwards costs at most
            # 4 x the largest forward's need in total
            cap = self.forward_crops(self.max_crops) * self._arena_bytes_per_crop
            ar = ActivationArena(self.device, max(need, min(2 * need, cap)) if ar is None else 2 * need)
            self._arenas[slot] = ar
        return ar

    def bucket(self, n, cap=None):
        """Crop count of the replay that serves a call of n crops: the next multiple of graph_bucket (at most cap)."""
        b = self.graph_bucket
        m = (n + b - 1) // b * b
        return min(m, cap) if cap is not None and cap >= n else m

    def warm(self, max_crops, slots=(0,), kind='features'):
        """Capture the replay of every crop-count bucket up to max_crops NOW (largest first: one activation arena, sized once), so that
        no frame pays a capture later -- the first sight of a bucket inside a frame is a stall of hundreds of milliseconds.
        -> dict(buckets, captures, seconds, arena_bytes): what the prewarmed cache holds."""
        import time
        t0, c0 = time.perf_counter(), self.captures
        buckets = sorted({self.bucket(k) for k in range(1, int(max_crops) + 1)}, reverse=True)
        self.max_crops = max(self.max_crops, buckets[0] if buckets else 0)
        for slot in slots:
            for n in buckets:
                if (self.forward_crops(n), kind, slot) not in self._graphs:
                    self._run(self.input_buffer(n, slot), kind, slot)
        torch.cuda.synchronize(self.device)
        return dict(buckets=sorted(buckets), captures=self.captures - c0, seconds=time.perf_counter() - t0, arena_bytes=self.arena_bytes())

    def arena_bytes(self):
        """Device memory of the activation arenas of all replay slots."""
        return int(sum(2 * a.half_bytes for a in self._arenas.values()))

    def _pool_of(self, slot):
        if slot not in self._pools:
            self._pools[slot] = torch.cuda.graph_pool_handle()
        return self._pools[slot]
