#!/usr/bin/env python3
"""CMU Panoptic ``calibration_<sequence>.json`` -> the calibration pickle the drivers load: {'P', 'K', 'RT', 'distCoef'}.

    python tools/panoptic_calibration.py calibration_160906_pizza1.json --cameras 00_03 00_06 00_12 00_13 00_23 \\
        --out ../CatchImage/Panoptic/160906_pizza1/camera_parameter_lens.pickle

Each camera of the file has a name ("00_03": panel 0, node 3), K (3 x 3), distCoef (5: k1, k2, p1, p2, k3 -- OpenCV's order), R (3 x 3) and
t (3 x 1, centimetres).  The pickle holds the cameras named by --cameras, in that order (DATASET.FOLDERS_ORDER of the config): P = K [R | t]
(C, 3, 4), K (C, 3, 3), RT (C, 3, 4), distCoef (C, 5), float64.  --unit-scale multiplies t (0.01: metres instead of centimetres; the
matcher's thresholds are in pixels, the 3D output comes out in the unit of t).  The file serves as DATASET.CALIBRATION_FILE and as
DATASET.DISTORTION_FILE (configs/Panoptic/model_configs_lens.yaml)."""
import argparse
import json
import pickle

import numpy as np


def convert(calibration, cameras=None, unit_scale=1.0):
    """calibration: the parsed JSON; cameras: names in output order (None: every 'hd' camera in file order)."""
    by_name = {c['name']: c for c in calibration['cameras']}
    if cameras is None:
        cameras = [c['name'] for c in calibration['cameras'] if c.get('type') == 'hd']
    missing = [n for n in cameras if n not in by_name]
    if missing:
        raise KeyError('not in the calibration file: %s' % ', '.join(missing))
    K = np.array([by_name[n]['K'] for n in cameras], dtype=np.float64).reshape(-1, 3, 3)
    R = np.array([by_name[n]['R'] for n in cameras], dtype=np.float64).reshape(-1, 3, 3)
    t = np.array([by_name[n]['t'] for n in cameras], dtype=np.float64).reshape(-1, 3, 1) * float(unit_scale)
    dist = np.array([by_name[n]['distCoef'] for n in cameras], dtype=np.float64).reshape(len(cameras), -1)
    if dist.shape[1] != 5:
        raise ValueError('distCoef has %d coefficients per camera, the model takes 5 (k1, k2, p1, p2, k3)' % dist.shape[1])
    RT = np.concatenate([R, t], axis=2)
    return {'P': K @ RT, 'K': K, 'RT': RT, 'distCoef': dist}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('calibration', help="Panoptic's calibration_<sequence>.json")
    ap.add_argument('--cameras', nargs='+', default=None, help='camera names in the order of DATASET.FOLDERS_ORDER (default: every hd camera)')
    ap.add_argument('--unit-scale', type=float, default=1.0, help='factor on t (0.01: metres)')
    ap.add_argument('--out', required=True, help='pickle to write')
    a = ap.parse_args()
    with open(a.calibration) as f:
        out = convert(json.load(f), a.cameras, a.unit_scale)
    with open(a.out, 'wb') as f:
        pickle.dump(out, f)
    print('%s: %d cameras, largest |k1| %.3f' % (a.out, len(out['K']), np.abs(out['distCoef'][:, 0]).max()))


if __name__ == '__main__':
    main()
