"""CPU: the tile searches of the resident-weights kernels (csrc/pam_resident.hpp for the C = 32 / 48 BasicBlocks, pick_tile96 and
d48_pick beside their kernels) against tests/golden/block_tiles.json -- what pam_basic_block2_tile and pam_conv3x3s2_c48_tile answered,
query by query, at the commit before the C = 32 and C = 48 searches became one (tools/record_block_tiles.py).  The table is replayed IN
ITS ORDER: the searches keep their last answers, and the order (48, 32, 96, 48, 32, 96 per shape, then everything backwards) makes a
memo that forgets one of its keys hand out another query's tile.  Needs the built library, no GPU."""
import ctypes
import json
import os

from pam import _lib

COLUMNS = ('entry', 'C', 'N', 'H', 'W', 'rc', 'rows', 'cols', 'groups')
UNTOUCHED = -99


def _rows():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'block_tiles.json')) as f:
        t = json.load(f)
    assert tuple(t['columns']) == COLUMNS
    return [tuple(r) for r in t['rows']]


def _lib_cdll():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pam_basic_block2_tile', 'pam_conv3x3s2_c48_tile'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGS[name]
    return lib


def test_every_recorded_query_in_its_order():
    """Return code and outputs of every row; a refused query leaves its outputs alone."""
    lib, bad = _lib_cdll(), []
    for k, row in enumerate(_rows()):
        entry, c, n, h, w = row[:5]
        out = (ctypes.c_int32 * 3)(UNTOUCHED, UNTOUCHED, UNTOUCHED)
        rc = lib.pam_basic_block2_tile(c, n, h, w, out) if entry == 0 else lib.pam_conv3x3s2_c48_tile(n, h, w, c, out)
        got = (rc,) + tuple(out)
        if got != row[5:]:
            bad.append((k, row, got))
    assert not bad, (len(bad), bad[:10])


def test_table_holds_the_grid_and_the_order_that_catches_a_short_memo_key():
    rows = _rows()
    block, down = [r for r in rows if r[0] == 0], [r for r in rows if r[0] == 1]
    batches = {1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 16, 20, 24, 28, 32, 40, 64}
    shapes = {(96, 72), (64, 48), (48, 36), (32, 24), (24, 18), (12, 9), (7, 5), (33, 41), (50, 72), (96, 70), (1, 1)}
    assert {r[1] for r in block} == {32, 48, 96, 192} and {r[2] for r in block} == batches and {r[3:5] for r in block} == shapes
    assert {r[1] for r in down} == {48, 96, 144, 192, 384, 100} and {r[2] for r in down} == batches and {r[3:5] for r in down} == shapes | {(2, 2)}
    assert len(block) == 2 * 7 * len(batches) * len(shapes) and len(down) == 2 * 6 * len(batches) * (len(shapes) + 1)
    # every (N, H, W) asks the three searches in turn, twice, so each answers between two queries of the same shape to the others
    for k in range(0, len(block), 7):
        assert [r[1] for r in block[k:k + 7]] == [48, 32, 96, 48, 32, 96, 192] and len({r[2:5] for r in block[k:k + 7]}) == 1
    # the second half is the first one backwards in N and shape
    half = len(block) // 7 // 2
    firsts = [block[7 * k][2:5] for k in range(2 * half)]
    assert firsts[half:] == firsts[:half][::-1]
    # accepted and refused queries of both entries; the channel counts answer differently somewhere, or the order would prove nothing
    assert all(r[5] == 0 for r in block if r[1] != 192) and all(r[5:] == (-1, UNTOUCHED, UNTOUCHED, UNTOUCHED) for r in block if r[1] == 192)
    assert all((r[5] == 0) == (r[1] % 48 == 0 and r[3] >= 2) for r in down)
    assert all(r[6:] == (UNTOUCHED,) * 3 for r in down if r[5] != 0) and all(r[8] >= 1 for r in down if r[5] == 0)
    by_shape = {}
    for r in block:
        if r[5] == 0:
            by_shape.setdefault(r[2:5], {})[r[1]] = r[6:8]
    assert any(len({v[32], v[48]}) == 2 for v in by_shape.values()) and any(len({v[48], v[96]}) == 2 for v in by_shape.values())
