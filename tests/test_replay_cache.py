"""CPU: host logic of the captured-forward cache (pam.replay.ForwardReplay, the base class of HRNetPose) on objects built with __new__,
and the names the benchmark and the harness entry read from pam.hrnet."""
import pytest

from pam import hrnet, selfcheck
from pam.replay import ForwardReplay

K1, K2, K3 = (20, 'features', 0), (8, 'features', 0), (4, 'features', 0)


def _filled():
    """One forward with both forms, one flagged-only capture, one stream-event capture (as test_abi's disable_flag_sync case)."""
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    net._graphs = {K1: ('F1',), K2: ('F2',), K3: ('E3',)}
    net._alt = {K1: {'flags': ('F1',), 'events': ('E1',)}, K2: None, K3: None}
    net.flag_synced = {K1: True, K2: True, K3: False}
    net.flag_timing = {20: dict(kept={'serial': True, 'throughput': True})}
    net._dead_graphs = []
    return net


def test_drop_captures_empties_the_cache_and_keeps_every_capture_alive():
    net = _filled()
    graphs, alts = list(net._graphs.values()), [v for v in net._alt.values() if v is not None]
    held = graphs + [form for alt in alts for form in alt.values()]
    net._dead_graphs.append(('D0',))                           # (a capture parked earlier stays)
    net.drop_captures()
    assert net._graphs == {} and net._alt == {} and net.flag_synced == {} and net.flag_timing == {}
    assert net._dead_graphs == [('D0',)] + graphs + alts and len(net._dead_graphs) == 1 + 3 + 1
    assert all(any(d is alt for d in net._dead_graphs) for alt in alts)                      # the very objects, not copies
    reachable = [d for d in net._dead_graphs if isinstance(d, tuple)] + [f for d in net._dead_graphs if isinstance(d, dict) for f in d.values()]
    assert all(any(r is h for r in reachable) for h in held)                                 # nothing was dropped
    net.drop_captures()                                        # an empty cache: nothing moves
    assert len(net._dead_graphs) == 5 and net._graphs == {}


@pytest.mark.parametrize('flag_race', [None, 'serial', 'throughput'])
@pytest.mark.parametrize('kept', [dict(serial=True, throughput=True), dict(serial=True, throughput=False),
                                  dict(serial=False, throughput=True), dict(serial=False, throughput=False)])
def test_pick_follows_the_race_of_the_current_mode(flag_race, kept):
    net = _filled()
    net.flag_race = flag_race
    net.flag_timing = {20: dict(kept=dict(kept))}
    flags_win = kept[flag_race or 'throughput']
    assert net._pick(K1) is net._alt[K1]['flags' if flags_win else 'events']
    assert net._pick(K1) == (('F1',) if flags_win else ('E1',))
    assert net._pick(K2) is net._graphs[K2] and net._pick(K3) is net._graphs[K3]             # one form only: the cache's entry
    del net._alt[K3]                                           # (no _alt entry at all reads the same)
    assert net._pick(K3) is net._graphs[K3]


def test_the_names_the_benchmark_and_the_harness_entry_read():
    """bench.py reads the model and drift helpers and the replay cache's state through pam.hrnet / HRNetPose; the harness entry calls
    hrnet.smoke_check().  Neither file may change with the package's layout."""
    for name in ('HRNetPose', 'PoseHighResolutionNet', 'init_random', 'fold_batchnorm', 'algorithmic_work', 'measure_bf16_drift',
                 'smoke_check', 'DumpResults'):
        assert hasattr(hrnet, name), name
    for name in ('reference_preprocess', 'reference_decode', 'drift_statistics'):            # callers written against the old home
        assert getattr(hrnet, name) is getattr(selfcheck, name), name
    for name in ('_replay_ms', 'config_for', 'check_void', 'clear_void', 'disable_flag_sync', 'warm', 'bucket'):
        assert callable(getattr(hrnet.HRNetPose, name)), name
    assert issubclass(hrnet.HRNetPose, ForwardReplay)
    # class-level defaults that objects built with __new__ rely on
    net = hrnet.HRNetPose.__new__(hrnet.HRNetPose)
    assert net._flag_sync_failed is False and net._hd_scratch is None
