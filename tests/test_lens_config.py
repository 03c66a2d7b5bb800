"""The configuration side of the lens model, on the CPU: tools/panoptic_calibration.py (Panoptic's calibration JSON -> the drivers' pickle),
configs/Panoptic/model_configs_lens.yaml (the Panoptic config plus one DATASET key) and testmodel.load_calibration, which hands
'distCoef' to GetCameraParameters next to P / K / RT."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest
import yaml

import lens_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'part-aware_measurement_for_3d_pose_estimation_and_tracking_amd')


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _panoptic_json(names):
    rng = np.random.default_rng(5)
    cams = []
    for i, n in enumerate(names):
        s = L.SETS['hd' if i % 2 == 0 else 'vga']
        fx, fy, cx, cy, skew = s['k']
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        cams.append(dict(name=n, type='hd' if n.startswith('00_') else 'vga', resolution=list(s['wh']), panel=int(n[:2]), node=int(n[3:]),
                         K=[[fx, skew, cx], [0, fy, cy], [0, 0, 1]], distCoef=list(s['dist']), R=q.tolist(),
                         t=(rng.uniform(-300, 300, (3, 1))).tolist()))
    return dict(calibDataSource='synthetic', cameras=cams)


def test_panoptic_calibration_tool(tmp_path):
    tool = _load(os.path.join(ROOT, 'tools', 'panoptic_calibration.py'), 'panoptic_calibration_tool')
    names = ['00_03', '01_02', '00_06', '00_12']
    cal = _panoptic_json(names)
    out = tool.convert(cal, ['00_12', '00_03'], unit_scale=0.01)
    assert set(out) == {'P', 'K', 'RT', 'distCoef'}
    assert out['P'].shape == (2, 3, 4) and out['K'].shape == (2, 3, 3) and out['RT'].shape == (2, 3, 4) and out['distCoef'].shape == (2, 5)
    src = {c['name']: c for c in cal['cameras']}
    for i, n in enumerate(['00_12', '00_03']):
        assert np.array_equal(out['K'][i], np.array(src[n]['K'])) and np.array_equal(out['distCoef'][i], np.array(src[n]['distCoef']))
        assert np.array_equal(out['RT'][i, :, :3], np.array(src[n]['R']))
        assert np.allclose(out['RT'][i, :, 3], 0.01 * np.array(src[n]['t']).reshape(3), rtol=0, atol=1e-15)
        assert np.allclose(out['P'][i], out['K'][i] @ out['RT'][i], rtol=0, atol=1e-9)
    assert len(tool.convert(cal)['K']) == 3                        # default: every hd camera, in file order
    with pytest.raises(KeyError):
        tool.convert(cal, ['00_99'])
    # the command line writes the pickle the drivers load
    jp, pp = tmp_path / 'calibration_x.json', tmp_path / 'camera_parameter_lens.pickle'
    jp.write_text(json.dumps(cal))
    import sys
    argv = sys.argv
    sys.argv = ['panoptic_calibration.py', str(jp), '--cameras', '00_03', '00_06', '--out', str(pp)]
    try:
        tool.main()
    finally:
        sys.argv = argv
    with open(pp, 'rb') as f:
        got = pickle.load(f)
    assert got['distCoef'].shape == (2, 5) and np.array_equal(got['P'], tool.convert(cal, ['00_03', '00_06'])['P'])


def test_lens_config_is_the_panoptic_config_plus_one_dataset_key():
    with open(os.path.join(PKG, 'configs', 'Panoptic', 'model_configs.yaml')) as f:
        base = yaml.safe_load(f)
    with open(os.path.join(PKG, 'configs', 'Panoptic', 'model_configs_lens.yaml')) as f:
        lens = yaml.safe_load(f)
    extra = {k: lens['DATASET'].pop(k) for k in list(lens['DATASET']) if k not in base['DATASET']}
    assert lens == base and list(extra) == ['DISTORTION_FILE'] and isinstance(extra['DISTORTION_FILE'], str)


def test_load_calibration_hands_distcoef_on(tmp_path):
    from pam.dataset import GetConfig
    from pam import testmodel
    tool = _load(os.path.join(ROOT, 'tools', 'panoptic_calibration.py'), 'panoptic_calibration_tool2')
    names = ['00_03', '00_06', '00_12', '00_13', '00_23']
    cal = tool.convert(_panoptic_json(names), names)
    with open(tmp_path / 'camera_parameter.pickle', 'wb') as f:
        pickle.dump({k: cal[k] for k in ('P', 'K', 'RT')}, f)
    with open(tmp_path / 'camera_parameter_lens.pickle', 'wb') as f:
        pickle.dump(cal, f)
    cfg = GetConfig(os.path.join(PKG, 'configs', 'Panoptic', 'model_configs_lens.yaml'))
    cfg.DATASET['ROOT'] = str(tmp_path)
    got = testmodel.load_calibration(cfg.DATASET)
    assert np.array_equal(got['distCoef'], cal['distCoef']) and np.array_equal(got['P'], cal['P'])
    plain = GetConfig(os.path.join(PKG, 'configs', 'Panoptic', 'model_configs.yaml'))
    plain.DATASET['ROOT'] = str(tmp_path)
    assert 'distCoef' not in testmodel.load_calibration(plain.DATASET)
    with open(tmp_path / 'camera_parameter_lens.pickle', 'wb') as f:
        pickle.dump(dict(cal, distCoef=cal['distCoef'][:3]), f)
    with pytest.raises(ValueError):
        testmodel.load_calibration(cfg.DATASET)
