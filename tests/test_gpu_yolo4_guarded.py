"""GPU: one forward of YOLOv4 and of YOLOv4-tiny with every launch's output carved from sentinel-filled, banded memory and the input
between poison bands -- the method of test_gpu_guarded_forward.py (its ``guarded_forward``, imported) on the executors of pam.yolov4:
the outputs are bitwise those of the unguarded forward whatever the arena held before, no band is damaged, no payload element is left
unwritten.  This is where k_route, the mish forms of k_conv_stem / k_conv_gs and the general-activation kernels with code 3 run at the
networks' real shapes next to guard bands."""
import pytest
import torch

import test_gpu_guarded_forward as GF

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


class Nets4(GF.Nets):
    def __init__(self):
        from pam import yolov4
        self.made, self.arena = {}, None
        self.make = {name: (lambda cfg=cfg: yolov4.HipDarknet4(yolov4.Darknet4(cfg()).init_random(0).eval(), DEV), 416, 416, False)
                     for name, cfg in (('yolov4', yolov4.yolov4_cfg), ('yolov4_tiny', yolov4.yolov4_tiny_cfg))}


@pytest.fixture(scope='module')
def nets():
    n = Nets4()
    yield n
    n.made.clear(); n.arena = None
    torch.cuda.empty_cache()


@pytest.mark.parametrize('views', [1, 3])
@pytest.mark.parametrize('name', ['yolov4_tiny', 'yolov4'])
def test_v4_forward_in_guarded_memory(nets, name, views):
    GF.guarded_forward(nets, name, None, views, False)
