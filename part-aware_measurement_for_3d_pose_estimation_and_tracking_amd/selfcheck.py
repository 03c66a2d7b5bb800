"""Helpers that check the pose product rather than being it: the bf16 drift measurement of the benchmark, the tiny end-to-end check of
the harness entry, and the plain-torch restatements of the crop and decode kernels that both (and the tests) compare against."""
import os

import torch

from .hrnet_model import PoseHighResolutionNet, fold_batchnorm, init_random


def measure_bf16_drift(net, n_crops=2, seed=2, checker_device='cpu'):
    """Self-consistency number of the bf16 conv stack (parity with the authors' backend is unpinned: no weights offline): the same
    folded weights run as a plain fp32 PyTorch module (the checker; on the CPU by default, so that no PyTorch-ROCm / MIOpen kernel
    appears in a profile of the run) vs ``net``'s product path, on seeded random crops.  -> relative L2 error of the heat-maps,
    fraction of (crop, joint) arg-max cells that moved, and the largest move in heat-map cells.  With random weights the heat-maps are
    nearly flat noise, so the arg-max fraction is a pessimistic figure."""
    dev = net.device
    cdev = torch.device(checker_device)
    seed_w = int(net.weights.split('=')[1].rstrip(')')) if net.weights.startswith('random') else 0
    if not net.weights.startswith('random'):
        raise RuntimeError('measure_bf16_drift rebuilds the fp32 module from the seed; load the checkpoint into both to use it with real weights')
    ref = fold_batchnorm(init_random(PoseHighResolutionNet(), seed=seed_w)).to(cdev).eval()
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn((n_crops, 3, net.resolution[0], net.resolution[1]), generator=g).to(dev)
    xb = x32.to(torch.bfloat16)
    x8 = torch.cat([xb, torch.zeros((n_crops, net.in_channels - 3, net.resolution[0], net.resolution[1]), dtype=torch.bfloat16, device=dev)], dim=1) \
        if net.in_channels > 3 else xb
    x8 = x8.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        if cdev.type == 'cpu':
            nthr = torch.get_num_threads()
            torch.set_num_threads(min(16, os.cpu_count() or 16))       # many-core hosts: a full team is slower by orders of magnitude
            h32 = ref(xb.float().to(cdev)).to(dev)
            torch.set_num_threads(nthr)
        else:
            h32 = ref(xb.float())
        hb = net.heatmaps(x8).float()
    return drift_statistics(h32, hb, dict(crops=n_crops, weights=net.weights,
                                          checker='same folded weights as a plain fp32 PyTorch module on the %s' % cdev.type))


def drift_statistics(h32, hb, extra=None, planted_seed=5):
    """What the bf16 stack's error does to the DECODE, in terms that bound something (random weights give nearly flat heat-maps whose
    arg-max moves at the slightest error -- that rate alone says nothing about the kernels):
      * ``rms_err``: RMS of (bf16 heat-map - fp32 heat-map) over all cells;
      * decided joints: maps whose fp32 peak stands above every cell OUTSIDE its 3 x 3 neighbourhood by a margin > k x rms_err; on those the
        bf16 arg-max should stay within one cell.  ``decided[k]`` = {frac, joints, max_cells} for k = 4, 8 (k = 8 is asserted in
        tests/test_gpu_image.py: moving such a peak takes two cells whose errors differ by 8 sigma);
      * planted peaks: one cell per map (seeded position) raised k x rms_err above the map's maximum in BOTH heat-maps, i.e. a joint the
        network is sure about by k error sigmas: ``planted_peak_max_cells[k]`` = largest distance in cells between the two decodes, k = 4,
        8, 16 (0 expected from k = 8; k = 16 asserted);
      * the unconditioned rate (``argmax_moved_frac``) stays for the record."""
    n, j, h, w = h32.shape
    f32, fb = h32.flatten(2), hb.flatten(2)
    a32, ab = f32.argmax(2), fb.argmax(2)
    moved = a32 != ab
    cells = torch.maximum((a32 // w - ab // w).abs(), (a32 % w - ab % w).abs())
    rms = float((hb - h32).pow(2).mean().sqrt())
    # margin of the fp32 peak over the rest of the map (3 x 3 neighbourhood of the peak excluded)
    yy = torch.arange(h, device=h32.device).view(1, 1, h, 1); xx = torch.arange(w, device=h32.device).view(1, 1, 1, w)
    py, px = (a32 // w).view(n, j, 1, 1), (a32 % w).view(n, j, 1, 1)
    near = ((yy - py).abs() <= 1) & ((xx - px).abs() <= 1)
    rest = h32.masked_fill(near, float('-inf')).flatten(2).max(2)[0]
    margin = f32.max(2)[0] - rest
    decided = {}
    for k in (4, 8):
        d = margin > k * rms
        decided[str(k)] = dict(frac=float(d.float().mean()), joints=int(d.sum()), max_cells=int(cells[d].max()) if bool(d.any()) else 0)
    planted = {}
    g = torch.Generator().manual_seed(planted_seed)
    pos = (torch.randint(0, h, (n, j), generator=g) * w + torch.randint(0, w, (n, j), generator=g)).to(h32.device).view(n, j, 1)
    top = f32.max(2, keepdim=True)[0]
    for k in (4, 8, 16):
        amp = (top - torch.gather(f32, 2, pos)) + k * rms              # the planted cell ends k x rms above the map's own maximum
        p32, pb = f32.scatter_add(2, pos, amp).argmax(2), fb.scatter_add(2, pos, amp).argmax(2)
        planted[str(k)] = int(torch.maximum((p32 // w - pb // w).abs(), (p32 % w - pb % w).abs()).max())
    out = dict(rel_l2_err=float((hb - h32).norm() / h32.norm()), rms_err=rms, decided=decided, planted_peak_max_cells=planted,
               argmax_moved_frac=float(moved.float().mean()), argmax_max_cells=int(cells.max()),
               argmax_mean_cells_when_moved=float(cells[moved].float().mean()) if bool(moved.any()) else 0.0,
               score_max_abs_err=float((fb.max(2)[0] - f32.max(2)[0]).abs().max()),
               headline='decided joints (fp32 peak margin > k x rms error) move by decided[k].max_cells; planted peaks of k x rms by planted_peak_max_cells[k]')
    out.update(extra or {})
    return out


def smoke_check():
    """Tiny self-check used by __graft_entry__.smoke(): 2 crops, decode vs torch arg-max, preprocess vs torch."""
    from .hrnet import HRNetPose
    dev = torch.device('cuda:0')
    net = HRNetPose(48, 17, None, resolution=(384, 288), use_graph=False)
    g = torch.Generator().manual_seed(0)
    frame = torch.randint(0, 256, (2, 480, 640, 3), dtype=torch.uint8, generator=g).to(dev)
    ptrs = torch.tensor([frame[0].data_ptr(), frame[1].data_ptr()], dtype=torch.int64, device=dev)
    view_of = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    slot_of = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    boxes = torch.tensor([[100.0, 50.0, 200.0, 300.0], [300.5, 100.25, 150.0, 280.0]], dtype=torch.float32, device=dev)
    x = net.input_buffer(2)
    net.preprocess(ptrs, 480, 640, view_of, boxes, x)
    ref = reference_preprocess(frame, view_of, boxes, (384, 288))
    err = (x[:, :3].float() - ref).abs().max().item()
    assert err < 0.03, err                               # bf16 rounding of values in [-2.2, 2.7]
    assert x.shape[1] == 3 or float(x[:, 3:].float().abs().max()) == 0.0
    hm = net.heatmaps(x)
    det = torch.zeros((2, 4, 17, 3), dtype=torch.float64, device=dev)
    net.decode(hm, view_of, slot_of, boxes, det)
    exp = reference_decode(hm, boxes)
    assert torch.equal(det[:, 0], exp), (det[:, 0] - exp).abs().max()


def reference_preprocess(frames, view_of, boxes, resolution):
    """Plain torch float32 restatement of the preprocessing kernel (tests): half-pixel bilinear sample of the box."""
    H, W = resolution
    n = view_of.numel()
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=frames.device)
    fh, fw = frames.shape[1], frames.shape[2]
    mean = torch.tensor([0.485, 0.456, 0.406], device=frames.device).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=frames.device).view(3, 1, 1)
    for i in range(n):
        img = frames[int(view_of[i])].float()
        bx, by, bw, bh = [boxes[i, k] for k in range(4)]
        sx = (bx + (torch.arange(W, device=frames.device, dtype=torch.float32) + 0.5) * (bw / W) - 0.5).clamp(0, fw - 1)
        sy = (by + (torch.arange(H, device=frames.device, dtype=torch.float32) + 0.5) * (bh / H) - 0.5).clamp(0, fh - 1)
        x0 = sx.floor().long(); y0 = sy.floor().long()
        x1 = (x0 + 1).clamp(max=fw - 1); y1 = (y0 + 1).clamp(max=fh - 1)
        fx = (sx - x0.float()).view(1, W, 1); fy = (sy - y0.float()).view(H, 1, 1)
        a = img[y0][:, x0]; b = img[y0][:, x1]; c = img[y1][:, x0]; d = img[y1][:, x1]
        top = a + (b - a) * fx; bot = c + (d - c) * fx
        v = (top + (bot - top) * fy) / 255.0                    # (H,W,3) BGR
        out[i] = (v.flip(2).permute(2, 0, 1) - mean) / std
    return out


def reference_decode(hm, boxes):
    """torch restatement of the decode kernel: hard arg-max (first maximum), upstream SimpleHRNet box mapping."""
    n, j, h, w = hm.shape
    flat = hm.float().reshape(n, j, h * w)
    val, idx = flat.max(dim=2)
    # torch.max may return any maximal index on ties; recompute the first one
    first = (flat == val.unsqueeze(2)).float().argmax(dim=2)
    py = (first // w).double(); px = (first % w).double()
    b = boxes.double()
    # divisors as tensors: on the GPU torch divides by a Python scalar as a multiplication with its reciprocal, which is one float32 ulp
    # off the kernel's (and NumPy's) true division now and then (seen at h = 96)
    hh = torch.tensor(float(h), dtype=torch.float64, device=hm.device); ww = torch.tensor(float(w), dtype=torch.float64, device=hm.device)
    y = (py / hh * b[:, 3:4] + b[:, 1:2]).float().double()
    x = (px / ww * b[:, 2:3] + b[:, 0:1]).float().double()
    return torch.stack([y, x, val.double()], dim=2)
