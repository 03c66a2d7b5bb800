"""CPU: the weight packers and the shape-only walks of the conv-stack executors give what tests/golden/pack_digests.json records
(tools/make_pack_digests.py wrote it from the code as it was before packing.py and engine.py were split off hrnet_hip.py): every packed
image bit for bit, and per executor configuration the counted bytes / flops / launches and the measuring arena's peak.  Images that
several kernels share are built by one function each; the equalities at the end keep it that way."""
import importlib.util
import json
import os

import pytest
import torch

from pam import hrnet_hip, packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('make_pack_digests', os.path.join(ROOT, 'tools', 'make_pack_digests.py'))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with open(os.path.join(ROOT, 'tests', 'golden', 'pack_digests.json')) as _f:
    GOLDEN = json.load(_f)


def test_packed_images_are_bit_identical_to_the_recorded_ones():
    got = tool.pack_digests()
    assert sorted(got) == sorted(GOLDEN['digests'])
    bad = [k for k in sorted(got) if got[k] != GOLDEN['digests'][k]]
    assert not bad, bad


@pytest.mark.parametrize('net', sorted(tool.WALKS))
def test_shape_only_walk_counts_what_was_recorded(net):
    got = tool.WALKS[net]()
    assert got and all(got[k] == GOLDEN['walks'][k] for k in got), (got, {k: GOLDEN['walks'].get(k) for k in got})


def test_every_configuration_has_a_recorded_walk():
    names = {'%s/%s' % (cls.__name__, name) for cls in (hrnet_hip.HipHRNet, hrnet_hip.HipHRNetW32, hrnet_hip.HipPoseResNet) for name in cls.CONFIGS}
    assert names | {'HipDarknet/darknet53', 'HipDarknet/tiny'} == set(GOLDEN['walks'])


def test_streamed_image_has_one_builder():
    op = hrnet_hip.PackedConv(tool.conv(192, 192, seed=30), 'cpu')
    saved = hrnet_hip.PackedConv.layout_lib
    hrnet_hip.PackedConv.layout_lib = tool.StubLayout(64, 64)
    try:
        img = op.image(24, 18)
    finally:
        hrnet_hip.PackedConv.layout_lib = saved
    assert op.last_streamed and torch.equal(img, hrnet_hip.streamed_image(op._w_ohwi, 64, 'cpu'))


def test_pointwise64_image_has_one_builder():
    conv = tool.conv(64, 64, 1, seed=31)
    op = hrnet_hip.PackedConv(conv, 'cpu')
    shared = packing.pointwise64_image(op.w[:, :64].float()).to(torch.bfloat16)
    assert torch.equal(hrnet_hip.PackedPointwise64(conv, 'cpu').w, shared)
    assert torch.equal(tool.pw64_image_as_conv_builds_it(op), shared)


def test_48_channel_kstep_image_has_one_builder():
    conv = tool.conv(48, 48, 3, 2, seed=32)
    op = hrnet_hip.PackedConv(conv, 'cpu')
    shared = packing.kstep48_image(op.w[:, :432].float()).to(torch.bfloat16)
    assert torch.equal(hrnet_hip.down48_image(op), shared)
    block = hrnet_hip.PackedBlock(tool.conv(48, 48, seed=33), tool.conv(48, 48, seed=34), 'cpu')
    for i, seed in enumerate((33, 34)):
        w = tool.conv(48, 48, seed=seed).weight.detach().permute(0, 2, 3, 1).reshape(48, 432)
        part = block.wpack[1024 + i * 43008:1024 + (i + 1) * 43008].view(torch.bfloat16)
        assert torch.equal(part, packing.kstep48_image(w).to(torch.bfloat16).reshape(-1))
