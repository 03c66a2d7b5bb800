"""2D overlay of the tracked poses: the ``joints_dict`` / ``draw_points_and_skeleton`` pair that the
reference's demo driver imports from the absent ``HRPose.misc.visualization`` (/root/reference/src/testmodel.py:34,72-75).
Pure host code (NumPy + PIL; OpenCV is not a dependency here).  Points are rows (y, x, confidence) like the 2D poses
``PersonTrack_Project3DPose`` returns; images are H x W x 3 uint8 BGR arrays and a new array is returned.
``draw_tracks`` overlays the tracks' 3D poses instead, re-projected into every view: the One-Euro filtered pose of a track that has one
(IterativeTracker(one_euro=...), ``TrackView.pose3d_filtered``), else its raw one.

``overlay_table`` / ``draw_overlay_device`` are the device form (csrc/pam_overlay.hip): the same primitives in the same order -- per
person the limbs, then the joints, the same colours, radius and width -- as one table of integer capsules that ONE launch paints into
the CUDA frames of all views in place.  The rasteriser is the project's own, defined in include/pam.h; it is not pixel-identical to
ImageDraw's lines and ellipses.  ``draw_tracks(..., device=True)`` feeds it the re-projected tracks.

``draw_tracks_device`` needs no host table: pam_overlay_tracks builds it on the device from the tracker state of a handle (csrc/
pam_overlay_tracks.hip) and pam_overlay_draw_counted paints it, two launches and nothing fetched or uploaded.  ``view3d_camera`` /
``view3d_background`` give the free-viewpoint 3D view next to the 2D overlays (the ``plot3DPose`` the reference's demo calls and does
not ship, src/testmodel.py:77-81 of the reference): one more 3 x 4 matrix in the same launch, drawn over a ground grid."""
import colorsys
import math

import numpy as np
from PIL import Image, ImageDraw

_TAB20 = [(31, 119, 180), (174, 199, 232), (255, 127, 14), (255, 187, 120), (44, 160, 44), (152, 223, 138), (214, 39, 40),
          (255, 152, 150), (148, 103, 189), (197, 176, 213), (140, 86, 75), (196, 156, 148), (227, 119, 194), (247, 182, 210),
          (127, 127, 127), (199, 199, 199), (188, 189, 34), (219, 219, 141), (23, 190, 207), (158, 218, 229)]


def joints_dict():
    """COCO 17-keypoint names and limb list (pairs of joint indices)."""
    return {'coco': {
        'keypoints': {0: 'nose', 1: 'left_eye', 2: 'right_eye', 3: 'left_ear', 4: 'right_ear', 5: 'left_shoulder',
                      6: 'right_shoulder', 7: 'left_elbow', 8: 'right_elbow', 9: 'left_wrist', 10: 'right_wrist',
                      11: 'left_hip', 12: 'right_hip', 13: 'left_knee', 14: 'right_knee', 15: 'left_ankle', 16: 'right_ankle'},
        'skeleton': [[15, 13], [13, 11], [16, 14], [14, 12], [11, 12], [5, 11], [6, 12], [5, 6], [5, 7], [6, 8], [7, 9],
                     [8, 10], [1, 2], [0, 1], [0, 2], [1, 3], [2, 4], [0, 5], [0, 6]]}}


def _palette(name, samples):
    if name == 'tab20':
        return [_TAB20[i % 20] for i in range(samples)]
    # rainbow-like palettes ('gist_rainbow', 'jet', ...): evenly spaced hues
    return [tuple(int(255 * c) for c in colorsys.hsv_to_rgb(0.83 * i / max(1, samples - 1), 1.0, 1.0)) for i in range(samples)]


def draw_points_and_skeleton(image, points, skeleton, points_color_palette='tab20', points_palette_samples=16,
                             skeleton_color_palette='Set2', skeleton_palette_samples=8, person_index=0, confidence_threshold=0.5):
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    im = Image.fromarray(np.ascontiguousarray(np.asarray(image)[..., ::-1]))           # BGR -> RGB for PIL
    draw = ImageDraw.Draw(im)
    radius = max(2, int(round(min(im.size) / 150.0)))
    limb_colors = _palette(skeleton_color_palette, skeleton_palette_samples)
    color = limb_colors[int(person_index) % len(limb_colors)]
    for a, b in skeleton:                                                              # limbs: one colour per person
        if pts[a, 2] > confidence_threshold and pts[b, 2] > confidence_threshold:
            draw.line([(pts[a, 1], pts[a, 0]), (pts[b, 1], pts[b, 0])], fill=color, width=max(1, radius // 2 + 1))
    pt_colors = _palette(points_color_palette, points_palette_samples)
    for j, (y, x, c) in enumerate(pts):                                                # joints: one colour per joint
        if c > confidence_threshold:
            draw.ellipse([x - radius, y - radius, x + radius, y + radius], fill=pt_colors[j % len(pt_colors)])
    return np.asarray(im)[..., ::-1].copy()


def track_pose3d(track):
    """The 3D pose (17, 3) an overlay shows for a TrackView: the filtered one when the track has one, else ``pose3d``."""
    f = getattr(track, 'pose3d_filtered', None)
    return np.asarray(track.pose3d if f is None else f, dtype=np.float64)


OVERLAY_COORD_MAX = 1 << 18          # 1/8 pixel: what pam_overlay_draw takes (include/pam.h)


def overlay_style(width, height):
    """(joint radius, limb width) in pixels for a frame of this size, as draw_points_and_skeleton picks them."""
    radius = max(2, int(round(min(width, height) / 150.0)))
    return radius, max(1, radius // 2 + 1)


def _overlay_q(v):
    v = float(v)
    if not math.isfinite(v):
        return None
    q = int(math.floor(8.0 * v + 0.5))
    return q if abs(q) <= OVERLAY_COORD_MAX else None


def overlay_table(per_view_people, sizes, skeleton=None, points_color_palette='gist_rainbow', points_palette_samples=17,
                  skeleton_color_palette='tab20', skeleton_palette_samples=8, confidence_threshold=0.0):
    """The primitive table of one pam_overlay_draw call.  per_view_people: per view a list of (pose rows (y, x, confidence),
    person_index), the pairs draw_points_and_skeleton is called with, in drawing order; sizes: per view (width, height).
    -> (int32 (n, 8) rows of PamOverlayPrim, [(first, count)] per view).  A joint is drawable when its confidence is above the threshold,
    both coordinates are finite and within 2^18 eighths of a pixel; a limb needs both of its joints."""
    skeleton = joints_dict()['coco']['skeleton'] if skeleton is None else skeleton
    limb_colors = _palette(skeleton_color_palette, skeleton_palette_samples)
    pt_colors = _palette(points_color_palette, points_palette_samples)
    bgr = lambda c: int(c[2]) | (int(c[1]) << 8) | (int(c[0]) << 16)          # palettes are RGB, the word is B | G << 8 | R << 16
    rows, ranges = [], []
    for people, (width, height) in zip(per_view_people, sizes):
        first = len(rows)
        radius, limb_width = overlay_style(width, height)
        for points, person_index in people:
            pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
            q = [(_overlay_q(x), _overlay_q(y)) if c > confidence_threshold else (None, None) for y, x, c in pts]
            ok = [a is not None and b is not None for a, b in q]
            color = bgr(limb_colors[int(person_index) % len(limb_colors)])
            for a, b in skeleton:
                if ok[a] and ok[b]:
                    rows.append((q[a][0], q[a][1], q[b][0], q[b][1], 4 * limb_width, color, 0, 0))
            for j, (x, y) in enumerate(q):
                if ok[j]:
                    rows.append((x, y, x, y, 8 * radius, bgr(pt_colors[j % len(pt_colors)]), 0, 0))
        ranges.append((first, len(rows) - first))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 8).astype(np.int32), ranges


def draw_overlay_device(frames, per_view_people, stream=None, **style):
    """Draws every view's people into its CUDA frame IN PLACE with one pam_overlay_draw launch on ``stream`` (default: the current
    one).  frames: per view a contiguous uint8 (H, W, 3) BGR CUDA tensor; per_view_people and style as ``overlay_table`` takes them.
    -> frames.  More than 32 views take one launch per 32."""
    import torch
    from . import _lib
    lib = _lib.load()
    for f in frames:
        if not (f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
            raise ValueError('draw_overlay_device takes contiguous uint8 (H, W, 3) CUDA tensors')
    if not frames:
        return frames
    device = frames[0].device
    stream = torch.cuda.current_stream(device) if stream is None else stream
    for lo in range(0, len(frames), _lib.OVERLAY_MAX_VIEWS):
        part = frames[lo:lo + _lib.OVERLAY_MAX_VIEWS]
        table, ranges = overlay_table(per_view_people[lo:lo + len(part)], [(f.shape[1], f.shape[0]) for f in part], **style)
        if not len(table):
            continue                                     # nothing to draw: no upload, no launch
        with torch.cuda.stream(stream):
            prims = torch.from_numpy(table).pin_memory().to(device, non_blocking=True)
        views = (_lib.PamOverlayView * len(part))()
        for v, f, (first, count) in zip(views, part, ranges):
            v.dev_bgr, v.width, v.height, v.prim_first, v.prim_count = f.data_ptr(), f.shape[1], f.shape[0], first, count
        rc = lib.pam_overlay_draw(stream.cuda_stream, len(part), views, prims.data_ptr(), len(table))
        if rc != 0:
            raise _lib.PamError('pam_overlay_draw failed (%d)' % rc)
    return frames


def track_rows(cameras, tracks, emitted_only=True):
    """Per view the (rows, track id) pairs ``draw_tracks`` draws: every (emitted) track's 3D pose re-projected with
    ``Camera.projectPoints``, joints behind the camera with confidence 0."""
    out = [[] for _ in cameras]
    for tr in tracks:
        if emitted_only and not getattr(tr, 'emitted', True):
            continue
        X = track_pose3d(tr)
        for v, cam in enumerate(cameras):
            depth = np.asarray(cam.P, dtype=np.float64)[2] @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T
            yx = np.asarray(cam.projectPoints(X), dtype=np.float64)
            out[v].append((np.concatenate([np.where(depth[:, None] > 0, yx, 0.0), (depth[:, None] > 0).astype(np.float64)], axis=1), tr.track_id))
    return out


def draw_tracks(imagelist, cameras, tracks, skeleton=None, emitted_only=True, device=False, **style):
    """Every (emitted) track's 3D pose (``track_pose3d``) re-projected into every view with ``Camera.projectPoints`` and drawn with
    ``draw_points_and_skeleton`` (colour by track id) -> a new list of images.  Joints behind a camera are not drawn.
    device=True: imagelist holds CUDA frames, which ``draw_overlay_device`` draws into in place (the same list comes back)."""
    skeleton = joints_dict()['coco']['skeleton'] if skeleton is None else skeleton
    kw = dict(points_color_palette='gist_rainbow', skeleton_color_palette='tab20', points_palette_samples=17, confidence_threshold=0.0)
    kw.update(style)
    if device:
        return draw_overlay_device(imagelist, track_rows(cameras, tracks, emitted_only), skeleton=skeleton, **kw)
    out = list(imagelist)
    for tr in tracks:
        if emitted_only and not getattr(tr, 'emitted', True):
            continue
        X = track_pose3d(tr)
        for v, cam in enumerate(cameras):
            depth = np.asarray(cam.P, dtype=np.float64)[2] @ np.concatenate([X, np.ones((len(X), 1))], axis=1).T
            yx = np.asarray(cam.projectPoints(X), dtype=np.float64)
            rows = np.concatenate([np.where(depth[:, None] > 0, yx, 0.0), (depth[:, None] > 0).astype(np.float64)], axis=1)
            out[v] = draw_points_and_skeleton(out[v], rows, skeleton, person_index=tr.track_id, **kw)
    return out


# ---- the tracks drawn from the device-resident state -------------------------------------------------------------------------------
def track_palette():
    """The 25 colour words (B | G << 8 | R << 16) pam_overlay_tracks takes: the 8 limb colours and the 17 joint colours draw_tracks uses."""
    word = lambda c: int(c[2]) | (int(c[1]) << 8) | (int(c[0]) << 16)
    return [word(c) for c in _palette('tab20', 8)] + [word(c) for c in _palette('gist_rainbow', 17)]


def draw_tracks_device(handle, frames, views=None, extra=None, pose=None, emitted_only=True, stream=None):
    """Draws the tracks of ``handle`` (a _lib.Handle, scene 0) into CUDA frames IN PLACE from the device-resident tracker state, behind
    whatever is queued on ``stream`` (default: the current one): pam_overlay_tracks builds the primitive table, pam_overlay_draw_counted
    paints it -- two launches per 32 views, no fetch, no upload and no synchronisation once the table's buffers exist (they are kept on
    the handle).  frames: contiguous uint8 (H, W, 3) BGR CUDA tensors; views: per frame the camera it shows, c >= 0 a camera of the
    handle, -1 - k row k of ``extra`` (None: frame i is camera i, frames beyond the handle's cameras are the extra views in order);
    extra: (n, 3, 4) float32 CUDA tensor of further projection matrices (view3d_camera); pose: the device pose buffer of
    Handle.one_euro, to draw the filtered poses instead of the newest raw ones; emitted_only as in draw_tracks.  -> frames."""
    import torch
    from . import _lib
    frames = list(frames)
    for f in frames:
        if not (f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous()):
            raise ValueError('draw_tracks_device takes contiguous uint8 (H, W, 3) CUDA tensors')
    if not frames:
        return frames
    n_cam = handle.C
    views = [i if i < n_cam else n_cam - 1 - i for i in range(len(frames))] if views is None else [int(v) for v in views]
    if len(views) != len(frames):
        raise ValueError('%d frames, %d views' % (len(frames), len(views)))
    device = frames[0].device
    if extra is not None and not torch.is_tensor(extra):
        extra = torch.from_numpy(np.ascontiguousarray(extra, dtype=np.float32)).to(device)
    stream = torch.cuda.current_stream(device) if stream is None else stream
    cap, palette = _lib.OVERLAY_TRACK_ROWS * handle.max_tracks, track_palette()
    keep = handle.__dict__.setdefault('_overlay_tables', {})
    for lo in range(0, len(frames), _lib.OVERLAY_MAX_VIEWS):
        part = frames[lo:lo + _lib.OVERLAY_MAX_VIEWS]
        key = (lo, len(part), str(device))
        if key not in keep:
            keep[key] = (torch.zeros((len(part), cap, 8), dtype=torch.int32, device=device),
                         torch.zeros(len(part), dtype=torch.int32, device=device))
        prims, count = keep[key]
        tv, dv = (_lib.PamOverlayTrackView * len(part))(), (_lib.PamOverlayView * len(part))()
        for k, (f, v) in enumerate(zip(part, views[lo:lo + len(part)])):
            tv[k].camera, tv[k].extra, tv[k].width, tv[k].height = (v, 0, f.shape[1], f.shape[0]) if v >= 0 else (-1, -1 - v, f.shape[1], f.shape[0])
            dv[k].dev_bgr, dv[k].width, dv[k].height, dv[k].prim_first, dv[k].prim_count = f.data_ptr(), f.shape[1], f.shape[0], k * cap, cap
        handle.overlay_tracks(stream.cuda_stream, tv, palette, prims, count, extra_P=extra, pose=pose, emitted_only=emitted_only)
        rc = handle.lib.pam_overlay_draw_counted(stream.cuda_stream, len(part), dv, prims.data_ptr(), len(part) * cap, count.data_ptr())
        if rc != 0:
            raise _lib.PamError('pam_overlay_draw_counted failed (%d)' % rc)
    return frames


def _positions(cameras):
    return np.stack([np.asarray(getattr(c, 'position', c), dtype=np.float64).reshape(3) for c in cameras])


def _ground_basis(up):
    up = np.asarray(up, dtype=np.float64)
    up = up / np.linalg.norm(up)
    e1 = np.eye(3)[int(np.argmin(np.abs(up)))]
    e1 = e1 - up * (e1 @ up)
    e1 /= np.linalg.norm(e1)
    return up, e1, np.cross(up, e1)


def view3d_camera(cameras, size, azimuth=35.0, elevation=25.0, up=(0, 0, 1), margin=0.08):
    """A look-at projection matrix for the free-viewpoint 3D view -> float32 (3, 4), to be handed to draw_tracks_device as an extra
    view.  cameras: the rig (objects with ``position``, or (3,) centres); size = (width, height) of the canvas; the ground is the
    plane through the origin whose normal is ``up``.  The eye looks at the point half-way between the ground and the centroid of the
    camera centres, from ``azimuth`` degrees round ``up`` and ``elevation`` degrees (clamped to 1 .. 89) above the ground, three rig
    radii away; the focal length is the largest that keeps every camera centre AND its foot on the ground -- the hull the people of
    the rig stand in -- at least ``margin`` x the canvas size away from every border, with positive depth."""
    pos = _positions(cameras)
    up, e1, e2 = _ground_basis(up)
    centre = pos.mean(axis=0)
    target = centre - up * (centre @ up) / 2.0
    fit = np.concatenate([pos, pos - np.outer(pos @ up, up)])
    radius = max(float(np.linalg.norm(fit - target, axis=1).max()), 1e-6)
    az, el = math.radians(float(azimuth)), math.radians(min(max(float(elevation), 1.0), 89.0))
    toward = math.cos(el) * (math.cos(az) * e1 + math.sin(az) * e2) + math.sin(el) * up
    eye = target + 3.0 * radius * toward
    fwd = -toward
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    cam = (fit - eye) @ R.T                                  # depth >= 3 radius - radius > 0
    w, h = float(size[0]), float(size[1])
    half = 0.5 - min(max(float(margin), 0.0), 0.45)
    f = min(half * w / max(float(np.abs(cam[:, 0] / cam[:, 2]).max()), 1e-9), half * h / max(float(np.abs(cam[:, 1] / cam[:, 2]).max()), 1e-9))
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    return (K @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)).astype(np.float32)


def view3d_background(cameras, P, size, up=(0, 0, 1), spacing=1.0, device=None, colour=(32, 32, 32), grid_colour=(96, 96, 96),
                      camera_colour=(200, 160, 60)):
    """The canvas of the 3D view, drawn ONCE at set-up with pam_overlay_draw -> uint8 (height, width, 3) BGR CUDA tensor: ``colour``
    everywhere, a ground grid of ``spacing`` (world units) over the square the rig stands on, and a disc per camera centre (colours
    are BGR).  P: view3d_camera's matrix.  Per frame the caller does ``canvas.copy_(background)`` and draws the tracks on top."""
    import torch
    from . import _lib
    w, h = int(size[0]), int(size[1])
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    canvas = torch.empty((h, w, 3), dtype=torch.uint8, device=device)
    canvas[:] = torch.tensor([int(c) for c in colour], dtype=torch.uint8, device=device)
    pos = _positions(cameras)
    up, e1, e2 = _ground_basis(up)
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    word = lambda c: int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)
    radius, limb_width = overlay_style(w, h)

    def at(X):
        x = P @ np.append(X, 1.0)
        if not x[2] > 0:
            return None
        q = (_overlay_q(x[0] / x[2]), _overlay_q(x[1] / x[2]))
        return None if q[0] is None or q[1] is None else q
    ground = pos - np.outer(pos @ up, up)
    mid = ground.mean(axis=0)
    n = max(1, int(math.ceil(float(np.linalg.norm(ground - mid, axis=1).max()) / float(spacing))))
    rows = []
    for k in range(-n, n + 1):
        for a, b in ((mid + spacing * (k * e1 - n * e2), mid + spacing * (k * e1 + n * e2)),
                     (mid + spacing * (-n * e1 + k * e2), mid + spacing * (n * e1 + k * e2))):
            qa, qb = at(a), at(b)
            if qa is not None and qb is not None:
                rows.append((qa[0], qa[1], qb[0], qb[1], 4, word(grid_colour), 0, 0))
    for c in pos:
        q = at(c)
        if q is not None:
            rows.append((q[0], q[1], q[0], q[1], 8 * (radius + limb_width), word(camera_colour), 0, 0))
    if rows:
        table = torch.from_numpy(np.asarray(rows, dtype=np.int64).astype(np.int32)).to(device)
        view = (_lib.PamOverlayView * 1)()
        view[0].dev_bgr, view[0].width, view[0].height, view[0].prim_first, view[0].prim_count = canvas.data_ptr(), w, h, 0, len(rows)
        rc = _lib.load().pam_overlay_draw(torch.cuda.current_stream(device).cuda_stream, 1, view, table.data_ptr(), len(rows))
        if rc != 0:
            raise _lib.PamError('pam_overlay_draw failed (%d)' % rc)
        torch.cuda.current_stream(device).synchronize()          # set-up: the table may go once the launch has read it
    return canvas


def view3d_setup(cameras, block, device, what='view3d'):
    """The free-viewpoint 3D view, made once.  block: dict(size=(width, height), azimuth, elevation, up, margin), keys in either letter
    case, every one optional (view3d_camera's defaults; size (640, 480)); anything without keys is the empty block -> dict(size,
    P = view3d_camera's float32 (3, 4), P_dev = the same as a (1, 3, 4) tensor on ``device``, background = view3d_background's canvas).
    what: how an error names the block."""
    import torch
    kw = {str(k).lower(): v for k, v in (dict(block) if hasattr(block, 'keys') else {}).items()}
    unknown = set(kw) - {'size', 'azimuth', 'elevation', 'up', 'margin'}
    if unknown:
        raise ValueError('%s: unknown key(s) %s (size, azimuth, elevation, up, margin)' % (what, sorted(unknown)))
    size = tuple(int(x) for x in kw.pop('size', (640, 480)))
    up = tuple(float(x) for x in kw.pop('up', (0, 0, 1)))
    P = view3d_camera(cameras, size, up=up, **{k: float(v) for k, v in kw.items()})
    return dict(size=size, P=P, P_dev=torch.from_numpy(P.reshape(1, 3, 4)).to(device),
                background=view3d_background(cameras, P, size, up=up, device=device))
