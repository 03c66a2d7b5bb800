"""Records tests/golden/fuse_plan.json (no GPU): what pam_fuse_sum_plan answers -- return code and, where the call is accepted, kernel,
level, unit or tile shape, units or tiles per image, grid and dynamic LDS bytes of the launch pam_fuse_sum_nhwc_bf16 would make -- over
a grid of the fuse-layer sums' integer arguments.  tests/test_fuse_plan.py replays the table and asserts what it covers.

A row is the query's integers, then rc, then (accepted rows only) the eight outputs; a refused query must leave its outputs alone.
`shifts` holds the sources' shifts as decimal digits (123 = shifts 1, 2, 3); source s has (C << shift_s) channels, the last one
`chan_off` more.

Uses only the query, so it runs on any build that has it (PAM_LIB selects the build): record from the build whose choice is the
reference, then change the plan.

    python tools/record_fuse_plans.py [--out tests/golden/fuse_plan.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pam  # noqa: E402,F401  (the package alias)
from pam import _lib  # noqa: E402

COLUMNS = ('N', 'H', 'W', 'C', 'n_plain', 'shifts', 'chan_off', 'tile_a', 'tile_b', 'max_workgroups', 'n_cu',
           'rc', 'kernel', 'L', 'rows', 'cols', 'per_image_y', 'per_image_x', 'grid', 'lds_bytes')
NQ = 11                                                          # integers of the query
UNTOUCHED = -99
TABLE = ((48, 1), (48, 12), (48, 123), (96, 1), (96, 12), (96, 2), (192, 1))          # csrc/pam_fuse_plan.hpp, FUSE_COMBOS
OUTSIDE = ((192, 12), (192, 2), (96, 13), (96, 23), (48, 2), (64, 1))
MAPS = ((12, 9), (8, 6), (5, 3), (1, 1), (1, 7), (7, 1))        # coarsest source's map; the output is (rows, columns) << coarsest shift
CROPS = (1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 28, 29, 32, 40, 64, 217)
CU_SENSITIVE = tuple(k for k in TABLE + OUTSIDE if k[0] == 192 or (k[0] == 96 and k[1] > 9))     # where max_workgroups / n_cu can matter


def digits(shifts):
    return [int(d) for d in str(shifts)]


def query(n, m, c, shifts, n_plain=0, chan_off=0, tile_a=0, tile_b=0, max_wg=0, n_cu=0, dh=0):
    smax = digits(shifts)[-1]
    return (n, (m[0] << smax) + dh, m[1] << smax, c, n_plain, shifts, chan_off, tile_a, tile_b, max_wg, n_cu)


def queries():
    # every combination x coarsest map x crop count at the library's choice
    for c, sh in TABLE + OUTSIDE:
        for m in MAPS:
            for n in CROPS:
                yield query(n, m, c, sh)
    # a named level (and values past the clamp) where the library's own choice is either kernel
    for c, sh in TABLE + OUTSIDE:
        for m in ((12, 9), (1, 7)):
            for n in (2, 40, 217):
                for ta in (1, 2, 3, 7):
                    yield query(n, m, c, sh, tile_a=ta, tile_b=ta + 2)
    # a cap on the workgroups and other CU counts, library's choice only
    for c, sh in CU_SENSITIVE:
        for m in ((12, 9), (5, 3)):
            for n in (2, 20, 40, 64):
                for max_wg, n_cu in ((5, 0), (100, 0), (0, 64), (0, 304), (5, 64), (100, 304)):
                    yield query(n, m, c, sh, max_wg=max_wg, n_cu=n_cu)
    # plain terms: 2, and 3 (refused)
    for c, sh in TABLE + OUTSIDE:
        for n in (2, 40):
            for npl in (2, 3):
                yield query(n, (5, 3), c, sh, n_plain=npl)
    # C = 192: 64 | 65 units and one unit per CU | one more, at the default CU count and at 304 (a 1 x 1 map is one unit, 8 x 6 are four)
    for n_cu in (0, 304):
        for n in (63, 64, 65, 66, 255, 256, 257, 303, 304, 305):
            yield query(n, (1, 1), 192, 1, n_cu=n_cu)
        for n in (16, 17, 64, 65, 76, 77):
            yield query(n, (8, 6), 192, 1, n_cu=n_cu)
    # the level-2 switch: 127 | 128 units at level 2 for the two combinations with at least 18 k-steps (a 1 x 1 map is one unit), and the
    # same sizes where the k-steps are fewer
    for c, sh in ((48, 123), (96, 12), (48, 12), (96, 2)):
        for n in (127, 128):
            yield query(n, (1, 1), c, sh)
    # an H that is no multiple of 2^shift; a last source with other channels than C << shift; no source, four sources, N = 0
    for c, sh in TABLE:
        yield query(2, (5, 3), c, sh, dh=1)
        yield query(2, (5, 3), c, sh, chan_off=32)
    yield query(2, (5, 3), 48, 1234)
    yield query(0, (5, 3), 48, 1)
    yield query(2, (5, 3), 48, 21)


def ask(lib, q):
    """One query -> [rc] or [0, eight outputs]."""
    n, h, w, c, n_plain, shifts, chan_off, tile_a, tile_b, max_wg, n_cu = q
    sh = digits(shifts)
    ch = [c << s for s in sh]
    ch[-1] += chan_off
    out = (ctypes.c_int32 * 8)(*[UNTOUCHED] * 8)
    rc = lib.pam_fuse_sum_plan(n, h, w, c, n_plain, len(sh), (ctypes.c_int32 * len(sh))(*sh), (ctypes.c_int32 * len(sh))(*ch),
                               tile_a, tile_b, max_wg, n_cu, out)
    if rc != 0:
        assert list(out) == [UNTOUCHED] * 8, (q, list(out))
        return [rc]
    return [rc] + list(out)


def cdll():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pam_fuse_sum_plan.restype, lib.pam_fuse_sum_plan.argtypes = _lib._SIGS['pam_fuse_sum_plan']
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'fuse_plan.json'))
    args = ap.parse_args()
    lib = cdll()
    rows = [list(q) + ask(lib, q) for q in queries()]
    with open(args.out, 'w') as f:
        f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(list(COLUMNS)), ',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows)))
    print('wrote %d rows from %s to %s' % (len(rows), _lib.LIB_PATH, args.out))


if __name__ == '__main__':
    main()
