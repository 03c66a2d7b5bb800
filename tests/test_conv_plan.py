"""CPU: pam_conv_plan (csrc/pam_conv_plan.hpp, the host-side choice of kernel and instantiation behind pam_conv2d_nhwc_bf16_ex) against
tests/golden/conv_plan.json -- what the library reported, launch by launch on an MI355X, for the six networks' forwards and the
convolution cases of tests/exact_ref.py over every tile code (tools/record_conv_plans.py), recorded at the commit before the choice
became a function of its own.  Needs the built library, no GPU."""
import ctypes
import json
import os

from pam import _lib

import conv_plan_cases as P

K_IGEMM, K_3X3, K_3X3S, K_GS, K_STEM = range(5)


def _table():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plan.json')) as f:
        t = json.load(f)
    assert tuple(t['columns']) == P.COLUMNS
    return [dict(zip(P.COLUMNS, r)) for r in t['rows']]


def _lib_cdll():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('pam_conv_plan', 'pam_conv3x3_slab', 'pam_conv3x3_layout', 'pam_conv3x3_layout_ex', 'pam_conv3x3_layout_gen', 'pam_conv3x3_layout_small'):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib._SIGS[name]
    return lib


def plan(lib, row):
    k, f = ctypes.c_int32(-99), ctypes.c_int32(-99)
    rc = lib.pam_conv_plan(*[row[c] for c in P.INTS + P.FLAGS], ctypes.byref(k), ctypes.byref(f))
    return rc, k.value, f.value


def test_plan_reproduces_every_recorded_launch():
    """Return code of every row; (kernel, form) of every accepted one; a refused plan leaves its outputs alone."""
    lib, bad = _lib_cdll(), []
    for row in _table():
        got = plan(lib, row)
        want = (row['rc'], row['kernel'], row['form']) if row['rc'] == 0 else (row['rc'], -99, -99)
        if got != want:
            bad.append((row, got))
    assert not bad, (len(bad), bad[:10])


def test_slab_in_the_form_is_the_layout_the_caller_packed_for():
    """3x3 / stride 1 / pad 1: the form's slab width equals the layout query the caller packs the weight image by."""
    lib, bad, seen = _lib_cdll(), [], set()
    for row in _table():
        if row['rc'] != 0 or (row['KH'], row['KW'], row['stride'], row['pad']) != (3, 3, 1, 1):
            continue
        shape = (row['H'], row['W'], row['Cin'], row['Cout'])
        if row['kernel'] == K_3X3:
            want = lib.pam_conv3x3_slab(*shape)
            got = 16 * (row['form'] % 10)
        elif row['kernel'] == K_3X3S:
            t = row['tile_cfg']
            assert t in (-1, -3, -5, -7, -8), row
            want = {-1: lambda: lib.pam_conv3x3_layout(*shape), -3: lambda: lib.pam_conv3x3_layout(*shape),
                    -5: lambda: lib.pam_conv3x3_layout_ex(*(shape + (48,))), -7: lambda: lib.pam_conv3x3_layout_gen(*shape),
                    -8: lambda: lib.pam_conv3x3_layout_small(*shape)}[t]()
            got = 16 * (row['form'] // 10 % 10)
        else:
            continue
        seen.add((row['kernel'], row['tile_cfg']))
        if got != want or got == 0:
            bad.append((row, got, want))
    assert not bad, bad[:10]
    # the executors state the layout of every streamed image (-3, not -1), so the table holds no streamed launch under -1
    assert {t for k, t in seen if k == K_3X3S} >= {-3, -5, -7, -8} and any(k == K_3X3 for k, _ in seen)


def test_table_reaches_every_family_and_tile_code():
    rows = _table()
    assert {r['kernel'] for r in rows if r['rc'] == 0} == {K_IGEMM, K_3X3, K_3X3S, K_GS, K_STEM}
    codes = {r['tile_cfg'] for r in rows}
    assert set(range(-8, 0)) | set(range(0, 13)) <= codes, sorted(set(range(-8, 13)) - codes)
    assert any(r['rc'] != 0 for r in rows)
    # the code no executor states: -6 has no branch of its own and lands on the classic rows-in-LDS kernel
    assert [(r['kernel'], r['form']) for r in rows if r['tile_cfg'] == -6] == [(K_3X3, 963)]
