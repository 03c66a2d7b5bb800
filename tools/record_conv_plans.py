"""Records tests/golden/conv_plan.json (needs a GPU): for every distinct pam_conv2d_nhwc_bf16_ex call of the forwards and cases below, the
integer arguments, the pointer-presence flags, the return code and -- when it is 0 -- what pam_conv_last_kernel() / pam_conv_last_form()
report for the launch.  tests/test_conv_plan.py holds pam_conv_plan() to this table without a GPU.

Uses only the launch entry and the two last_* queries, so it runs on any commit that has them: record at the commit whose choice is the
reference, then change the chooser.

Covered (tests/conv_plan_cases.py): one forward of HRNet-W48, HRNet-W32 and PoseResNet-50 under each named configuration of its
executor at 1, 2, 6 and 20 crops; Darknet-53, YOLOv3-tiny and YOLOv3-SPP at 1, 3 and 5 views; every CONV_CASES case of
tests/exact_ref.py with its own variants and over all of ALL_TILES, refused pairs included.

    python tools/record_conv_plans.py [--out tests/golden/conv_plan.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import pam  # noqa: E402,F401  (the package alias)
import conv_plan_cases as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'conv_plan.json'))
    args = ap.parse_args()
    from pam import _lib
    lib = _lib.load()
    rows = set()

    def on_conv(query, rc):
        rows.add(query + ((rc, lib.pam_conv_last_kernel(), lib.pam_conv_last_form()) if rc == 0 else (rc, None, None)))

    wrap = lambda l: P.ConvSpy(l, on_conv)
    dev = torch.device('cuda:0')
    log = lambda s: print('%-50s %d rows' % (s, len(rows)), flush=True)
    P.drive_networks(wrap, dev, crops=(1, 2, 6, 20), views=(1, 3, 5), all_configs=True, log=log)
    P.drive_cases(wrap, dev)
    log('cases')
    key = lambda r: tuple(-1 if v is None else v for v in r)
    with open(args.out, 'w') as f:
        f.write('{"columns": %s,\n "rows": [\n%s\n]}\n' % (json.dumps(list(P.COLUMNS)), ',\n'.join(json.dumps(list(r)) for r in sorted(rows, key=key))))
    print('wrote %d rows to %s' % (len(rows), args.out))


if __name__ == '__main__':
    main()
