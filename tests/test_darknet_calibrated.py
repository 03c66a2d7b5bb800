"""CPU: the calibrated test detector of darknet_calibrated.py must stay a network whose folded biases and per-channel scales are
non-trivial, whose activations stay bounded and whose heads give a few tens of boxes -- the per-launch GPU parity tests
(test_gpu_darknet_layers.py) see a wiring fault only through them."""
import os

import torch

import darknet_calibrated as DC
from pam import yolov3


def test_calibrated_detector_is_deterministic():
    a = DC._build(DC.SEED).state_dict()
    b = DC.calibrated().state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_every_folded_conv_has_its_own_bias_and_channel_scales():
    model = DC.calibrated()
    convs = DC.folded_convs(model, bf16=False)
    assert len(convs) == 75
    for i, c in convs.items():
        assert float(c.bias.std()) > 0.1 and float(c.bias.abs().max()) > 0.3, i
    for i, m in enumerate(model.mods):
        if hasattr(m, 'bn'):
            s = m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)
            assert float(s.max() / s.min()) > 1.5, i
    # the product's random network folds to the same kind of biases but barely spread scales: the reason this network exists
    plain = yolov3.Darknet().init_random(0)
    with torch.no_grad():
        scales = [m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps) for m in plain.conv_modules() if hasattr(m, 'bn')]
    assert max(float(s.std() / s.mean()) for s in scales) < 0.2


def test_activations_stay_bounded_through_all_75_convs():
    model = DC.calibrated()
    x = DC.images((1, 3, 416, 416), 123)
    F = torch.nn.functional
    convs = DC.folded_convs(model, bf16=False)
    rms, outs = [], []
    with torch.no_grad():
        for i, b in enumerate(model.layers):
            t = b['type']
            if t == 'convolutional':
                x = convs[i](x)
                x = F.leaky_relu(x, 0.1) if b['activation'] == 'leaky' else x
                rms.append(float(x.pow(2).mean().sqrt()))
            elif t == 'shortcut':
                x = outs[i - 1] + outs[i + b['from']]
            elif t == 'route':
                xs = [outs[l if l >= 0 else i + l] for l in b['layers']]
                x = xs[0] if len(xs) == 1 else torch.cat(xs, 1)
            elif t == 'upsample':
                x = F.interpolate(x, scale_factor=2, mode='nearest')
            outs.append(x)
    assert len(rms) == 75
    assert all(0.1 <= r <= 30.0 for r in rms), [round(r, 3) for r in rms]


def test_heads_give_a_few_tens_of_boxes_at_score_one_half():
    """Fresh 416 x 416 images: 5-60 boxes each after NMS, far fewer than the 1024 candidates the NMS holds (a test that compares boxes
    compares a real list; none is cut by the capacity)."""
    model = DC.calibrated()
    heads = DC.storage_forward(model, DC.images((3, 3, 416, 416), 7), bf16_weights=False, bf16_store=False)
    for kept, cand in DC.boxes_per_image(model, heads):
        assert 5 <= kept <= 60 and cand < 1024, (kept, cand)


def test_darknet_weights_file_round_trips_bit_exact(tmp_path):
    """save_darknet_weights -> Darknet.load_darknet_weights gives back every tensor bit-exact (the GPU tests then load the same file
    through the product constructor YOLOv3(cfg, weights))."""
    model = DC.calibrated()
    path = os.path.join(str(tmp_path), 'calibrated.weights')
    model.save_darknet_weights(path)
    back = yolov3.Darknet(yolov3.default_cfg())
    back.load_darknet_weights(path)
    ref, got = model.state_dict(), back.state_dict()
    for k in ref:
        if k.endswith('num_batches_tracked'):
            continue                                  # not part of the Darknet format
        assert torch.equal(got[k], ref[k]), k
