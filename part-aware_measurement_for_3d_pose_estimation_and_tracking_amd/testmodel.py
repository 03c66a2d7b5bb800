#!/usr/bin/env python3
"""Demo driver with the reference's CLI (/root/reference/src/testmodel.py): ``python testmodel.py --dataset Shelf``.

Per frame: load C images -> person boxes -> HRNet 2D poses -> PersonTrack_Project3DPose, with the reference's timing
print-out.  Boxes come from PersonDetect when ``DETECT_MODEL: YOLOv3`` (testmodel.py:56-58), else -- ``DETECT_MODEL: None``,
the shipped default -- boxes (and optionally 2D poses) come from ``DATASET.PRECOMPUTED``, a pickle
{frame_id: [per view list of {'bbox': [x,y,w,h], optional 'keypoints', 'keypoints_score'}]} -- see INTEGRATION.md."""
import argparse
import os
import pickle
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import pam  # noqa: E402
from pam.dataset import GetConfig, LoadFilenames  # noqa: E402
from pam.ingest import FrameLoader  # noqa: E402


def build_model(cfg):
    from pam.ivclabpose import ivclabpose
    pipe = cfg.PIPELINE_COMBINATION
    det = cfg.DETECT_MODELS[str(pipe['DETECT_MODEL']).upper()]
    pose_key = str(pipe['POSE_MODEL']).upper()
    pose = cfg.POSE_MODELS[pose_key] if pose_key in cfg.POSE_MODELS else None
    matcher = cfg.PERSON_MATCHERS[str(pipe['PERSON_MATCHER']).upper()]
    return ivclabpose(person_detector=det, pose_detector=pose, person_matcher=matcher,
                      conf_threshold=pipe['CONF_THRESHOLD']), pipe['BUILD_3D']


def load_calibration(dataset):
    """DATASET.CALIBRATION_FILE, the reference's {'P', 'K', 'RT'} pickle (/root/reference/src/testmodel.py:29-30; a 'distCoef' it
    holds is kept).  DATASET.DISTORTION_FILE (optional, not in the reference): a pickle whose 'distCoef' (C, 5) -- (k1, k2, p1, p2, k3)
    per camera, in FOLDERS_ORDER -- is handed to GetCameraParameters next to them (tools/panoptic_calibration.py writes one)."""
    with open(os.path.join(dataset.ROOT, dataset.CALIBRATION_FILE), 'rb') as f:
        camera_parameter = dict(pickle.load(f))
    lens_file = dataset.get('DISTORTION_FILE')
    if lens_file:
        with open(os.path.join(dataset.ROOT, lens_file), 'rb') as f:
            dist = np.asarray(pickle.load(f)['distCoef'], dtype=np.float64)
        if dist.shape != (len(camera_parameter['K']), 5):
            raise ValueError('%s: distCoef is %s, the calibration has %d cameras' % (lens_file, dist.shape, len(camera_parameter['K'])))
        camera_parameter['distCoef'] = dist
    return camera_parameter


def frame_inputs(model, precomputed, frame_id, imagelist, ahead=None, next_frame=None):
    """person_bbox_list + dump_result_list for one frame -> (pbl, dump, detect seconds, pose seconds, the next frame's detection ticket).
    ahead: this frame's detection, issued one frame ago (PersonDetectAhead); next_frame = (frame_id, imagelist) of the frame after this
    one when the loader has it already: its detection is issued BEFORE this frame's pose network and runs under it."""
    dt_det = 0.0
    nxt = None
    if model.person_detector is not None:                    # testmodel.py:56-58
        t0 = time.time()
        # DETECT_EVERY (optional key): the detector on every K-th frame, boxes round the tracks' predictions in between
        if model.schedule_frame() == 'detector':
            pbl = model.PersonDetectResult(ahead) if ahead is not None else model.PersonDetect(imagelist, frame_id)
        else:
            pbl = model.PersonBoxesFromTracks(imagelist, frame_id)
        if next_frame is not None and model.box_source() == 'detector':      # (the next frame's source: schedule_frame has counted this one)
            nxt = model.PersonDetectAhead(next_frame[1], next_frame[0])
        dt_det = time.time() - t0
    else:
        views = precomputed.get(frame_id, [[] for _ in imagelist])
        pbl = [[dict(image_id=frame_id, category_id=1, score=float(p.get('score', 1.0)), bbox=list(p['bbox']),
                     data=imagelist[v], feature=[]) for p in persons] for v, persons in enumerate(views)]
        if all('keypoints' in p for persons in views for p in persons):
            dump = [[dict(bbox=list(p['bbox']), keypoints=list(p['keypoints']), keypoints_score=list(p['keypoints_score']),
                          feature=[]) for p in persons] for persons in views]
            return pbl, dump, 0.0, 0.0, None
    t0 = time.time()
    dump = model.PersonPoseDetect(imagelist=None, person_bbox_list=pbl, batch_size=20)
    return pbl, dump, dt_det, time.time() - t0, nxt


def _device_available():
    import torch
    return torch.cuda.is_available()


def view3d_setup(model, block):
    """DATASET.VIEW3D {SIZE: [width, height], AZIMUTH, ELEVATION, UP, MARGIN} (every key optional) -> what overlay_on_device needs for the
    free-viewpoint 3D view: the look-at matrix on the device and the background canvas, both made once."""
    import torch
    from pam.visualization import view3d_setup as setup
    device = torch.device('cuda', model.device) if isinstance(model.device, int) else torch.device(model.device)
    v3 = setup(model.cameras, block, device, what='DATASET.VIEW3D')
    return dict(P=v3['P_dev'], background=v3['background'])


def overlay_on_device(model, imagelist, result, tracks=False, view3d=None):
    """The overlay of one frame drawn on the device: the 2D poses of PersonTrack_Project3DPose's result per view, in the order the host
    path draws them, then (ONE_EURO) the re-projected filtered tracks.  Frames that are still NumPy arrays are uploaded first.
    tracks (DATASET.OVERLAY_TRACKS): the tracks' 3D poses instead, projected and drawn straight from the tracker's device-resident
    state -- the filtered ones under ONE_EURO -- without a host table (pam.visualization.draw_tracks_device); view3d (view3d_setup): a
    3D canvas more, appended to the list.  -> the list of CUDA frames, drawn in place."""
    import torch
    from pam.visualization import draw_overlay_device, draw_tracks, draw_tracks_device
    device = torch.device('cuda', model.device) if isinstance(model.device, int) else torch.device(model.device)
    frames = [im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im)).to(device) for im in imagelist]
    if tracks or view3d is not None:
        trk = model.tracker
        pose = trk._oe.dev[0] if getattr(trk, '_oe', None) is not None else None
        canvas = [view3d['background'].clone()] if view3d is not None else []          # a new one per frame: the writer reads the last
        if tracks:
            draw_tracks_device(trk.handle, frames + canvas, extra=view3d['P'] if canvas else None, pose=pose)
            return frames + canvas
        draw_tracks_device(trk.handle, canvas, views=[-1], extra=view3d['P'], pose=pose)
    people = [[] for _ in frames]
    for cids, poses_2d, pids in zip(result[0], result[1], result[2]):
        for cid, pose_2d, pid in zip(cids, poses_2d, pids):
            people[cid].append((pose_2d, pid))
    draw_overlay_device(frames, people)
    if getattr(model, 'pts3d_filtered', None) is not None:
        draw_tracks(frames, model.cameras, model.tracker.tracks, device=True)
    return frames + (canvas if view3d is not None else [])


def test_ivclabpose_PersonTrack_Project3DPose(cfg, inputs, on_frame=None):
    dataset = cfg.DATASET
    os.makedirs(cfg.OUTPUT, exist_ok=True)
    camera_parameter = load_calibration(dataset)
    model, build3D = build_model(cfg)
    precomputed = {}
    if model.person_detector is None:
        with open(os.path.join(dataset.ROOT, dataset.PRECOMPUTED), 'rb') as f:
            precomputed = pickle.load(f)
    t_det = t_pose = t_track = 0.0
    start, end = dataset.TEST_RANGE
    n_views = len(dataset.FOLDERS_ORDER)
    # images are decoded a few frames ahead on worker threads; with a GPU pipeline behind them (detector or pose network) they are
    # uploaded from pinned memory on a copy stream and arrive as CUDA tensors (LOADER_DEVICE: false keeps them NumPy arrays, which
    # the host overlay needs anyway).  DETECT_AHEAD (default on): frame t + 1's person detection is issued before frame t's pose network.
    # DEVICE_JPEG (optional key, default off): the workers run only the Huffman pass of a baseline JPEG and the device rebuilds the
    # frame (pam.ingest.FrameLoader(device_decode=True)); a file that path does not take goes through Pillow as before.
    # DEVICE_OVERLAY (optional key, default off; needs a device): VISUALIZATION / SAVE_IMAGE no longer switch the device loader off --
    # the overlay is drawn into the CUDA frames by pam_overlay_draw (pam.visualization.draw_overlay_device) and SAVE_IMAGE encodes them
    # behind the device (pam.egress.FrameWriter: pam_jpeg_forward, then the Huffman pass and the file on worker threads).
    # OVERLAY_TRACKS / VIEW3D (optional keys, default off, only with DEVICE_OVERLAY): the tracks' 3D poses are drawn from the tracker's
    # device-resident state instead of the 9-tuple's 2D poses (pam_overlay_tracks: no host table), and a free-viewpoint 3D view of them
    # is written as <frame_id>_3d.jpg beside the per-camera files (VIEW3D: {SIZE: [w, h], AZIMUTH:, ELEVATION:, UP:}).
    draw = bool(cfg.get('VISUALIZATION') or cfg.get('SAVE_IMAGE'))
    device_overlay = draw and bool(dataset.get('DEVICE_OVERLAY', False)) and _device_available()
    overlay_tracks, view3d_block = bool(dataset.get('OVERLAY_TRACKS', False)), dataset.get('VIEW3D')
    if (overlay_tracks or view3d_block) and not dataset.get('DEVICE_OVERLAY', False):
        raise ValueError('DATASET.OVERLAY_TRACKS / DATASET.VIEW3D need DATASET.DEVICE_OVERLAY: true')
    view3d = None
    on_gpu = ((model.person_detector is not None or model.pose_model is not None) and (not draw or device_overlay)
              and bool(dataset.get('LOADER_DEVICE', True)))
    look_ahead = model.person_detector is not None and bool(dataset.get('DETECT_AHEAD', True))
    loader = FrameLoader(dataset.TEST_DATASET, inputs, indices=range(start, end), workers=int(dataset.get('LOADER_THREADS', 8)),
                         device=(model.device if on_gpu else None), device_decode=bool(dataset.get('DEVICE_JPEG', False)))
    it = iter(loader)
    cur = next(it, None)
    ahead = None
    writer = store = None
    i = -1
    while cur is not None:
        i += 1
        frame_id, imagelist, timestamp = cur
        nxt_frame = next(it, None)
        if i == 0:
            model.GetCameraParameters(camera_parameter, imagelist[0].shape[0], imagelist[0].shape[1])
        pbl, dump, dt_det, dt_pose, ahead = frame_inputs(model, precomputed, frame_id, imagelist, ahead,
                                                         (nxt_frame[0], nxt_frame[1]) if (look_ahead and nxt_frame is not None) else None)
        cur = nxt_frame
        result = None
        dt_track = 0.0
        if any(len(v) for v in dump):                       # testmodel.py:66 guard: no pose in any view -> frame skipped
            t0 = time.time()
            result = model.PersonTrack_Project3DPose(frame_id=frame_id, person_bbox_list=pbl, dump_results=dump, build3D=build3D)
            dt_track = time.time() - t0
        if result is not None and device_overlay:
            if writer is None and cfg.get('SAVE_IMAGE'):
                from pam.egress import FrameWriter
                store = os.path.join(cfg.OUTPUT, dataset.TEST_DATASET, 'Images')
                os.makedirs(store, exist_ok=True)
                writer = FrameWriter(model.device, workers=int(dataset.get('WRITER_THREADS', 4)), depth=int(dataset.get('WRITER_DEPTH', 4)))
            if view3d_block and view3d is None:
                view3d = view3d_setup(model, view3d_block)
            imagelist = overlay_on_device(model, imagelist, result, tracks=overlay_tracks, view3d=view3d)
            if cfg.get('SAVE_IMAGE'):
                names = ['%s_%d.jpg' % (frame_id, cid) for cid in range(n_views)] + (['%s_3d.jpg' % frame_id] if view3d is not None else [])
                writer.submit(frame_id, imagelist, [os.path.join(store, n) for n in names])
        elif result is not None and (cfg.get('VISUALIZATION') or cfg.get('SAVE_IMAGE')):      # testmodel.py:70-75 overlay
            from pam.visualization import joints_dict, draw_points_and_skeleton
            camera_ids, pts, person_ids = result[0], result[1], result[2]
            for cids, poses_2d, pids in zip(camera_ids, pts, person_ids):
                for cid, pose_2d, pid in zip(cids, poses_2d, pids):
                    imagelist[cid] = draw_points_and_skeleton(imagelist[cid], pose_2d, joints_dict()['coco']['skeleton'],
                                                              person_index=pid, points_color_palette='gist_rainbow',
                                                              skeleton_color_palette='tab20', points_palette_samples=17,
                                                              confidence_threshold=0.0)
            if getattr(model, 'pts3d_filtered', None) is not None:                              # ONE_EURO: the filtered 3D poses, re-projected
                from pam.visualization import draw_tracks
                imagelist = draw_tracks(imagelist, model.cameras, model.tracker.tracks)
            if cfg.get('SAVE_IMAGE'):
                from PIL import Image
                store = os.path.join(cfg.OUTPUT, dataset.TEST_DATASET, 'Images')
                os.makedirs(store, exist_ok=True)
                for cid, im in enumerate(imagelist):
                    Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(os.path.join(store, '%s_%d.jpg' % (frame_id, cid)))
        if on_frame is not None:
            on_frame(frame_id, timestamp, result)
        if frame_id > start + 10:
            t_det += dt_det
            t_pose += dt_pose
            t_track += dt_track
    loader.close()
    if writer is not None:
        writer.close()
    n = max(1, end - start - 10)
    print("Person Detect Processing time (s/f): %f" % (t_det / n))
    print("Pose Detect Processing time (s/f): %f" % (t_pose / n))
    print("Track Processing time (s/f): %f" % (t_track / n))
    print("fps: %f" % (1 / max(1e-12, (t_det / n + t_pose / n) / n_views + t_track / n)))
    print("tracking fps: %f" % (1 / max(1e-12, t_track / n)))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset', help='Three options: CampusSeq1, Shelf, Panoptic', type=str, default='CampusSeq1')
    parser.add_argument('--config', help='model configuration file (default: configs/<dataset>/model_configs.yaml)', type=str, default=None)
    opt = parser.parse_args()
    cfg = GetConfig(opt.config or os.path.join(_HERE, 'configs', opt.dataset, 'model_configs.yaml'))
    datas = LoadFilenames(cfg.DATASET)
    {'PersonTrack_Project3DPose': test_ivclabpose_PersonTrack_Project3DPose}[cfg.TEST_FUNCTION](cfg, datas)
