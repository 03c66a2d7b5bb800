"""The demo loop with DATASET.DEVICE_OVERLAY on a real MI355X: testmodel's loop on a short synthetic sequence (boxes and 2D poses
precomputed, images from disk) draws with pam_overlay_draw and saves through pam.egress.FrameWriter.  The files are those of the host
path by count and name, and every one is byte for byte what the restatements give for that frame: tests/overlay_ref.py's drawing of the
loop's result into the decoded input frame, encoded by tests/jpeg_enc_ref.py (which is held to Pillow).  With the key off none of the
new entry points is called and the files are the host path's."""
import os
import pickle

import numpy as np
import pytest

import pam
from pam import synth
from pam.dataset import GetConfig, LoadFilenames, LoadImages
import jpeg_enc_ref as E
import overlay_ref as R
from recorded_calls import recorded_calls

pytestmark = pytest.mark.gpu
N_FRAMES, W, H = 5, 360, 288
NEW_CALLS = ('pam_overlay_draw', 'pam_jpeg_forward', 'pam_jpeg_encode', 'pam_jpeg_encode_bound', 'pam_jpeg_quality_tables')


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    """Three cameras of 360 x 288 smooth frames as PNG files (their decode is exact), the calibration and the precomputed detections."""
    from PIL import Image
    import jpeg_ref as J
    root = tmp_path_factory.mktemp('overlay_seq') / 'CampusSeq1'
    seq = synth.make_sequence('S1', n_frames=N_FRAMES, seed=2)
    for c in range(3):
        os.makedirs(root / ('Camera%d' % c))
        for t in range(N_FRAMES):
            Image.fromarray(J.content('smooth', W, H, 10 * c + t)).save(root / ('Camera%d' % c) / ('%04d.png' % t))
    with open(root / 'camera_parameter.pickle', 'wb') as f:
        pickle.dump(seq['calib'], f)
    pre = {}
    for t, views in enumerate(seq['frames']):
        _, dr = synth.to_dump_results(views)
        pre[t] = [[dict(bbox=d['bbox'], keypoints=d['keypoints'], keypoints_score=d['keypoints_score']) for d in v] for v in dr]
    with open(root / 'detections.pickle', 'wb') as f:
        pickle.dump(pre, f)
    return root


def run_loop(dataset, out, **keys):
    from pam import testmodel
    cfg = GetConfig(os.path.join(pam.PKG_DIR, 'configs', 'CampusSeq1', 'model_configs.yaml'))
    cfg.DATASET.ROOT = str(dataset); cfg.DATASET.DATA_FORMAT = '*.png'; cfg.DATASET.TEST_RANGE = [0, N_FRAMES]
    cfg.OUTPUT = str(out); cfg.SAVE_IMAGE = True
    cfg.PIPELINE_COMBINATION.POSE_MODEL = 'Precomputed'
    for k, v in keys.items():
        cfg.DATASET[k] = v
    files = LoadFilenames(cfg.DATASET)
    seen = []
    with recorded_calls() as calls:
        testmodel.test_ivclabpose_PersonTrack_Project3DPose(cfg, files, on_frame=lambda fid, ts, res: seen.append((fid, res)))
    store = os.path.join(str(out), 'CampusSeq1', 'Images')
    return files, seen, calls, {n: open(os.path.join(store, n), 'rb').read() for n in sorted(os.listdir(store))}


def people_of(result, n_views):
    people = [[] for _ in range(n_views)]
    for cids, poses, pids in zip(result[0], result[1], result[2]):
        for cid, pose, pid in zip(cids, poses, pids):
            people[cid].append((pose, pid))
    return people


def test_device_overlay_loop_writes_the_restatements_files(dataset, tmp_path):
    import torch
    files, seen, calls, saved = run_loop(dataset, tmp_path / 'dev', DEVICE_OVERLAY=True, WRITER_DEPTH=2)
    torch.cuda.synchronize()
    drawn = [(fid, res) for fid, res in seen if res is not None]
    assert [f for f, _ in seen] == list(range(N_FRAMES)) and len(drawn) > 2          # a run longer than the writer's ring of two
    assert sorted(saved) == sorted('%s_%d.jpg' % (fid, c) for fid, _ in drawn for c in range(3))
    n_people = 0
    for fid, res in drawn:
        frames, _ = LoadImages('CampusSeq1', files[fid])
        people = people_of(res, 3)
        n_people += sum(len(p) for p in people)
        for c in range(3):
            want = E.encode_bgr(R.draw(frames[c], people[c]))
            assert saved['%s_%d.jpg' % (fid, c)] == want, (fid, c)
    assert n_people > 6                                                  # skeletons were drawn, not only frames copied
    assert calls.count('pam_jpeg_forward') == len(drawn) and calls.count('pam_jpeg_encode') == 3 * len(drawn)
    assert 1 <= calls.count('pam_overlay_draw') <= len(drawn)


def test_with_the_key_off_none_of_the_new_entry_points_is_called_and_the_files_are_the_host_paths(dataset, tmp_path):
    import io
    from PIL import Image
    from pam.visualization import joints_dict, draw_points_and_skeleton
    for k, keys in enumerate((dict(), dict(DEVICE_OVERLAY=False))):
        files, seen, calls, saved = run_loop(dataset, tmp_path / ('host%d' % k), **keys)
        assert not [c for c in calls if c in NEW_CALLS]
        drawn = [(fid, res) for fid, res in seen if res is not None]
        assert sorted(saved) == sorted('%s_%d.jpg' % (fid, c) for fid, _ in drawn for c in range(3)) and len(drawn) > 2
        for fid, res in drawn[:2] if k else drawn:
            frames, _ = LoadImages('CampusSeq1', files[fid])
            for c, ppl in enumerate(people_of(res, 3)):
                im = frames[c]
                for pose, pid in ppl:
                    im = draw_points_and_skeleton(im, pose, joints_dict()['coco']['skeleton'], person_index=pid, points_color_palette='gist_rainbow',
                                                  skeleton_color_palette='tab20', points_palette_samples=17, confidence_threshold=0.0)
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(buf, format='JPEG')
                assert saved['%s_%d.jpg' % (fid, c)] == buf.getvalue(), (fid, c)
