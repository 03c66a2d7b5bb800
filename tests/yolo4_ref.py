"""References for the YOLOv4 additions (test infrastructure: nothing under the package imports this).

``mish32``   the mish epilogue of csrc/pam_conv.hpp (epi_mish) restated in NumPy float32, operation for operation.
``layer``    one plan step of a convolution layer restated in torch float32: conv + bias, activation, THEN the shortcut, one bf16 rounding
             left to the caller.  The GPU walk of test_gpu_yolo4.py uses it with torch's own mish; the CPU tests use it with planted
             mistakes to show that the restatement tells them apart.
``decode``   oracle/yolo_ref.py's decode with YOLOv4's scale_x_y; its greedy NMS is imported from there."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import yolo_ref as Y

f32 = np.float32


def mish32(x):
    """e = expf(x); n = e * e + 2 * e; x <= -0.6f ? x * (n / (n + 2)) : x - 2 * (x / (n + 2)), every operation rounded to float32."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(x).astype(f32)
        n = (e * e).astype(f32) + (f32(2) * e).astype(f32)
        n = n.astype(f32)
        d = (n + f32(2)).astype(f32)
        lo = (x * (n / d).astype(f32)).astype(f32)
        hi = (x - (f32(2) * (x / d).astype(f32)).astype(f32)).astype(f32)
    return np.where(x <= f32(-0.6), lo, hi).astype(f32)


def mish64(x):
    """x * tanh(softplus(x)) in float64 (softplus by logaddexp: no overflow)."""
    x = np.asarray(x, dtype=np.float64)
    return x * np.tanh(np.logaddexp(0.0, x))


def mish_torch(t):
    """mish32 on a torch tensor (any device): the same operations in float32."""
    e = torch.exp(t)
    n = e * e + 2.0 * e
    return torch.where(t <= -0.6, t * (n / (n + 2.0)), t - 2.0 * (t / (n + 2.0)))


ACTS = {'linear': lambda t: t, 'leaky': lambda t: F.leaky_relu(t, 0.1), 'mish': F.mish}


def layer(x, conv, act, skip=None, acts=ACTS, order='act_then_skip', bias_first=True):
    """fp32 reference of one conv step: act(conv(x) + bias) [+ skip].  x, skip: float32 (N, C, H, W); conv: a folded nn.Conv2d.
    order / bias_first exist for the planted mistakes of test_yolo4_cpu.py ('skip_then_act': the activation after the shortcut;
    bias_first False: the bias added after the activation)."""
    y = F.conv2d(x, conv.weight, conv.bias if bias_first else None, conv.stride, conv.padding)
    if order == 'skip_then_act' and skip is not None:
        y = y + skip
    y = acts[act](y)
    if not bias_first and conv.bias is not None:
        y = y + conv.bias.reshape(1, -1, 1, 1)
    if order == 'act_then_skip' and skip is not None:
        y = y + skip
    return y


def candidates(heads, anchors, scales, net_w, net_h, num_classes, class_id, score_thresh, frame_w, frame_h):
    """oracle.yolo_ref.yolo_candidates with the centre (sigmoid(t) * s - 0.5 * (s - 1) + cell) / grid, s = scales[head], in float32 and
    in that order of operations.  heads: any number, in the order given (candidate order: head, cell row-major, anchor)."""
    boxes, scores = [], []
    st = 5 + num_classes
    for h, t in enumerate(heads):
        gh, gw = t.shape[:2]
        v = t[:, :, :3 * st].reshape(gh, gw, 3, st).astype(f32)
        gy, gx = np.meshgrid(np.arange(gh, dtype=f32), np.arange(gw, dtype=f32), indexing='ij')
        s = f32(scales[h])
        off = (f32(0.5) * (s - f32(1))).astype(f32)
        sc = (Y.sigmoid(v[..., 4]) * Y.sigmoid(v[..., 5 + class_id])).astype(f32)
        bx = ((((Y.sigmoid(v[..., 0]) * s).astype(f32) - off).astype(f32) + gx[..., None]).astype(f32) / f32(gw)).astype(f32)
        by = ((((Y.sigmoid(v[..., 1]) * s).astype(f32) - off).astype(f32) + gy[..., None]).astype(f32) / f32(gh)).astype(f32)
        aw = np.asarray(anchors, dtype=f32)[h, :, 0][None, None, :]; ah = np.asarray(anchors, dtype=f32)[h, :, 1][None, None, :]
        with np.errstate(over='ignore'):
            bw = (np.exp(v[..., 2]) * aw / f32(net_w)).astype(f32)
            bh = (np.exp(v[..., 3]) * ah / f32(net_h)).astype(f32)
        x1 = (bx - f32(0.5) * bw) * f32(frame_w); x2 = (bx + f32(0.5) * bw) * f32(frame_w)
        y1 = (by - f32(0.5) * bh) * f32(frame_h); y2 = (by + f32(0.5) * bh) * f32(frame_h)
        keep = sc > f32(score_thresh)
        boxes.append(np.stack([x1, y1, x2, y2], -1)[keep]); scores.append(sc[keep])
    return np.concatenate(boxes).astype(f32), np.concatenate(scores).astype(f32)


def decode(heads, anchors, scales, net_w, net_h, num_classes, class_id, score_thresh, nms_thresh, frame_w, frame_h, max_det):
    """-> (rows (k, 5) x1 y1 x2 y2 score, candidates above the threshold): oracle.yolo_ref.detect with scale_x_y."""
    boxes, scores = candidates(heads, anchors, scales, net_w, net_h, num_classes, class_id, score_thresh, frame_w, frame_h)
    kept = Y.greedy_nms(boxes, scores, nms_thresh, max_det)
    return np.concatenate([boxes[kept], scores[kept, None]], axis=1).reshape(-1, 5), len(scores)
