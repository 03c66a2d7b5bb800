"""Records tests/golden/block_tiles.json (no GPU): what the host-side tile searches of the resident-weights kernels answer, query by
query IN ORDER -- pam_basic_block2_tile(C, N, H, W) for the fused BasicBlocks and pam_conv3x3s2_c48_tile(N, H, W, Cout) for k_down48.
tests/test_block_tiles.py replays the table in the same order and compares every row.

The order is part of the record: the searches keep their last answers, so for every (N, H, W) the channel counts are asked 48, 32, 96,
48, 32, 96 (then 192, a refusal), and the whole walk is repeated with N and the shapes reversed -- a memo that forgets one of the things
its answer depends on then returns another query's tile.  A refused query must leave its outputs alone (-99 here).

Uses only the two queries, so it runs on any commit that has them: record at the commit whose choice is the reference (PAM_LIB selects
another build of the library), then change the searches.

    python tools/record_block_tiles.py [--out tests/golden/block_tiles.json]"""
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

COLUMNS = ('entry', 'C', 'N', 'H', 'W', 'rc', 'rows', 'cols', 'groups')      # entry 0: the block (C, no groups: -99), 1: k_down48 (C = Cout)
BATCHES = (1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 20, 24, 28, 32, 40, 64)
SHAPES = ((96, 72), (64, 48), (48, 36), (32, 24), (24, 18), (12, 9), (7, 5), (33, 41), (50, 72), (96, 70), (1, 1))
BLOCK_C = (48, 32, 96, 48, 32, 96, 192)
DOWN_SHAPES = SHAPES + ((2, 2),)
DOWN_COUT = (48, 96, 144, 192, 384, 100)
UNTOUCHED = -99


def queries():
    for batches, shapes, down_shapes in ((BATCHES, SHAPES, DOWN_SHAPES), (BATCHES[::-1], SHAPES[::-1], DOWN_SHAPES[::-1])):
        for n in batches:
            for h, w in shapes:
                for c in BLOCK_C:
                    yield 0, c, n, h, w
        for n in batches:
            for h, w in down_shapes:
                for c in DOWN_COUT:
                    yield 1, c, n, h, w


def ask(lib, entry, c, n, h, w):
    """One query -> (rc, rows, cols, groups)."""
    out = (ctypes.c_int32 * 3)(UNTOUCHED, UNTOUCHED, UNTOUCHED)
    rc = lib.pam_basic_block2_tile(c, n, h, w, out) if entry == 0 else lib.pam_conv3x3s2_c48_tile(n, h, w, c, out)
    return (rc,) + tuple(out)


def cdll():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pam_basic_block2_tile', 'pam_conv3x3s2_c48_tile'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGS[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'block_tiles.json'))
    args = ap.parse_args()
    lib = cdll()
    rows = [list(q + ask(lib, *q)) for q in queries()]
    with open(args.out, 'w') as f:
        f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(list(COLUMNS)), ',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows)))
    print('wrote %d rows from %s to %s' % (len(rows), _lib.LIB_PATH, args.out))


if __name__ == '__main__':
    main()
