"""CPU: pam_fuse_sum_plan (csrc/pam_fuse_plan.hpp, the host-side choice behind pam_fuse_sum_nhwc_bf16: accepted or refused, which of the
two kernels, anchor level and unit rectangle or tile, grid, dynamic LDS bytes) against tests/golden/fuse_plan.json -- what the commit
before the plan existed chose, query by query: its unchanged entry point run up to the launch with dummy pointers and a note of what it
was about to launch (tools/record_fuse_plans.py).  The rows with n_cu = 0 were recorded at 256 compute units,
which is what the query assumes on a machine without a device and finds on an MI355X.  Needs the built library, no GPU.

The recording and pam.h agree on every row: the combinations outside the table that reach the persistent kernel's host side in that
commit (OUTSIDE_LDS below) were refused there too, because their weights do not fit its LDS, so no row's expectation is set by
decision instead of by recording."""
import ctypes
import itertools
import json
import os

from pam import _lib

COLUMNS = ('N', 'H', 'W', 'C', 'n_plain', 'shifts', 'chan_off', 'tile_a', 'tile_b', 'max_workgroups', 'n_cu',
           'rc', 'kernel', 'L', 'rows', 'cols', 'per_image_y', 'per_image_x', 'grid', 'lds_bytes')
NQ = 11
UNTOUCHED = -99
TABLE = {(48, 1), (48, 12), (48, 123), (96, 1), (96, 12), (96, 2), (192, 1)}          # FUSE_COMBOS of csrc/pam_fuse_plan.hpp
OUTSIDE = {(192, 12), (192, 2), (96, 13), (96, 23), (48, 2), (64, 1)}
OUTSIDE_LDS = {(192, 12), (192, 2), (96, 13), (96, 23)}         # sizes exist at which the recorded commit handed these to the persistent kernel
K_STEPS = {(48, 1): 3, (48, 12): 9, (48, 123): 21, (96, 1): 6, (96, 12): 18, (96, 2): 12, (192, 1): 12}


def _rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fuse_plan.json')) as f:
        t = json.load(f)
    assert tuple(t['columns']) == COLUMNS
    return [tuple(r) for r in t['rows']]


def _lib_cdll():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pam_fuse_sum_plan.restype, lib.pam_fuse_sum_plan.argtypes = _lib._SIGS['pam_fuse_sum_plan']
    return lib


def _ask(lib, q):
    n, h, w, c, n_plain, shifts, chan_off, tile_a, tile_b, max_wg, n_cu = q
    sh = [int(d) for d in str(shifts)]
    ch = [c << s for s in sh]
    ch[-1] += chan_off
    out = (ctypes.c_int32 * 8)(*[UNTOUCHED] * 8)
    rc = lib.pam_fuse_sum_plan(n, h, w, c, n_plain, len(sh), (ctypes.c_int32 * len(sh))(*sh), (ctypes.c_int32 * len(sh))(*ch),
                               tile_a, tile_b, max_wg, n_cu, out)
    return rc, tuple(out)


def _units(h, w, level):
    """Units per image at an anchor level: 16 anchor pixels as 4 x 4, 2 x 8, 8 x 2, 1 x 16 or 16 x 1, whichever takes the fewest."""
    ha, wa = h >> level, w >> level
    return min(-(-ha // (1 << a)) * -(-wa // (1 << b)) for a, b in ((2, 2), (1, 3), (3, 1), (0, 4), (4, 0)))


def test_every_recorded_query():
    """Return code and the eight outputs of every row; a refused query leaves its outputs alone."""
    lib, bad = _lib_cdll(), []
    for k, row in enumerate(_rows()):
        rc, out = _ask(lib, row[:NQ])
        want = row[NQ + 1:] if row[NQ] == 0 else (UNTOUCHED,) * 8
        if rc != row[NQ] or out != want:
            bad.append((k, row, rc, out))
    assert not bad, (len(bad), bad[:10])


def test_null_output_and_null_arrays_are_refused():
    lib = _lib_cdll()
    sh, ch = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(96)
    out = (ctypes.c_int32 * 8)(*[UNTOUCHED] * 8)
    assert lib.pam_fuse_sum_plan(2, 10, 6, 48, 0, 1, sh, ch, 0, 0, 0, 0, out) == 0 and out[0] == 1
    assert lib.pam_fuse_sum_plan(2, 10, 6, 48, 0, 1, sh, ch, 0, 0, 0, 0, None) == -1
    out = (ctypes.c_int32 * 8)(*[UNTOUCHED] * 8)
    assert lib.pam_fuse_sum_plan(2, 10, 6, 48, 0, 1, None, ch, 0, 0, 0, 0, out) == -1
    assert lib.pam_fuse_sum_plan(2, 10, 6, 48, 0, 1, sh, None, 0, 0, 0, 0, out) == -1 and tuple(out) == (UNTOUCHED,) * 8


def test_table_holds_every_combination_both_kernels_and_both_sides_of_every_threshold():
    rows = _rows()
    ok = [r for r in rows if r[NQ] == 0]
    no = [r for r in rows if r[NQ] != 0]
    assert all(len(r) == NQ + 9 for r in ok) and all(len(r) == NQ + 1 and r[NQ] == -1 for r in no)
    combo = lambda r: (r[3], r[5])
    # every combination of the table is accepted somewhere, by both kernels where it can reach the persistent one; nothing else ever is
    assert {combo(r) for r in ok} == TABLE and OUTSIDE <= {combo(r) for r in no}
    assert {combo(r) for r in ok if r[12] == 2} == {(96, 12), (192, 1)} and {combo(r) for r in ok if r[12] == 1} == TABLE
    # the combinations the recorded commit chose a kernel for before it looked at its instantiations: refused in the recording as well
    for c in OUTSIDE_LDS:
        mine = [r for r in rows if combo(r) == c]
        assert len(mine) >= 96 and all(r[NQ] == -1 for r in mine), c
    # refusals of every kind: three plain terms, an H that is no multiple of 2^shift, other channels than C << shift, four sources, N = 0
    in_table = [r for r in no if combo(r) in TABLE]
    assert {r[4] for r in in_table} >= {0, 3} and any(r[6] for r in in_table) and any(r[0] == 0 for r in no) and any(r[5] == 1234 for r in no)
    assert any(r[1] % (1 << int(str(r[5])[-1])) for r in in_table)
    assert {r[4] for r in ok} == {0, 2}
    # the grid: maps, crop counts, named levels, caps and CU counts
    lib_choice = [r for r in ok if r[7] == 0 and r[9] == 0 and r[10] == 0]
    smax = lambda r: int(str(r[5])[-1])
    assert {(r[1] >> smax(r), r[2] >> smax(r)) for r in lib_choice} == {(12, 9), (8, 6), (5, 3), (1, 1), (1, 7), (7, 1)}
    assert {r[0] for r in lib_choice} >= {1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 29, 32, 40, 64, 217}
    assert {r[7] for r in ok} == {0, 1, 2, 3, 7} and all(r[12] == 1 and r[13] == min(r[7], 2, smax(r)) for r in ok if r[7] > 0)
    assert all(r[9] == 0 and r[10] == 0 for r in rows if r[7] > 0)
    assert {(r[9], r[10]) for r in ok} == {(0, 0), (5, 0), (100, 0), (0, 64), (0, 304), (5, 64), (100, 304)}
    assert any(r[18] == 5 for r in ok if r[12] == 2 and r[9] == 5) and all(r[18] <= (r[10] or 256) for r in ok if r[12] == 2)
    # threshold 1 and 2, C = 192: the persistent kernel up to 64 units at level 1 and above one unit per CU
    u1 = lambda r: r[0] * _units(r[1], r[2], 1)
    c192 = [r for r in lib_choice if r[3] == 192] + [r for r in ok if r[3] == 192 and r[7] == 0 and r[9] == 0 and r[10] == 304]
    for n_cu, cus in ((0, 256), (304, 304)):
        kern = {}
        for r in c192:
            if r[10] == n_cu:
                kern.setdefault(u1(r), set()).add(r[12])
        assert kern[64] == {2} and kern[65] == {1} and kern[cus] == {1} and kern[cus + 1] == {2}, (n_cu, kern)
        assert all(k == {2 if (u <= 64 or u > cus) else 1} for u, k in kern.items()), (n_cu, kern)
    assert {18, 180, 360} <= {u1(r) for r in c192}
    # threshold 3, C = 96 under two sources: the persistent kernel above 768 units at level 1 (28 | 29 crops at 48 x 36 are 756 | 783)
    kern = {u1(r): r[12] for r in lib_choice if combo(r) == (96, 12)}
    assert kern[756] == 1 and kern[783] == 2 and all(k == (2 if u > 768 else 1) for u, k in kern.items()), kern
    assert all(r[12] == 1 for r in lib_choice if r[3] == 48 or combo(r) in ((96, 1), (96, 2)))
    # threshold 4, the level: 2 from 18 k-steps and 128 units at level 2 on, else 1
    u2 = lambda r: r[0] * _units(r[1], r[2], 2)
    for c in ((48, 123), (96, 12)):
        lev = {}
        for r in lib_choice:
            if combo(r) == c and r[12] == 1:
                lev.setdefault(u2(r), set()).add(r[13])
        assert lev[127] == {1} and lev[128] == {2} and all(v == {2 if u >= 128 else 1} for u, v in lev.items()), (c, lev)
    for c in ((48, 12), (96, 2)):                              # a coarsest shift of 2 with fewer k-steps: level 1 at any size
        mine = [r for r in lib_choice if combo(r) == c]
        assert K_STEPS[c] < 18 and any(u2(r) >= 128 for r in mine) and all(r[13] == 1 for r in mine), c
    # what a plan says about itself: one workgroup per unit and no dynamic LDS (kernel 1); whole tiles, LDS within a workgroup's 160 KB (2)
    for r in ok:
        if r[12] == 1:
            assert r[14] + r[15] == 4 and r[18] == r[0] * r[16] * r[17] == r[0] * _units(r[1], r[2], r[13]) and r[19] == 0, r
        else:
            assert r[13] == 0 and r[16] == -(-r[1] // (r[14] << smax(r))) and r[17] == -(-r[2] // (r[15] << smax(r))), r
            assert 1 <= r[18] <= r[0] * r[16] * r[17] and 0 < r[19] <= 160 * 1024, r


def test_the_accepted_combinations_are_the_table_at_every_size():
    """Every C the entry point knows (and one it does not) with every ascending choice of one to three shifts, at sizes on both sides of
    every threshold and at every level a caller can name: accepted exactly when (C, shifts) is a row of the table."""
    lib = _lib_cdll()
    accepted, refused = set(), set()
    for c in (48, 64, 96, 192):
        for k in (1, 2, 3):
            for sh in itertools.combinations((1, 2, 3, 4, 5), k):
                shifts = int(''.join(str(s) for s in sh))
                for m in ((1, 1), (12, 9)):
                    for n in (1, 2, 20, 40, 217, 1000):
                        for ta in (0, 1, 2):
                            rc, out = _ask(lib, (n, m[0] << sh[-1], m[1] << sh[-1], c, 0, shifts, 0, ta, 0, 0, 0))
                            (accepted if rc == 0 else refused).add((c, shifts))
                            assert rc in (0, -1) and (rc == 0) == (out[0] in (1, 2))
    assert accepted == TABLE and not (accepted & refused)
