"""GPU: pam_conv_plan (the host-side choice, csrc/pam_conv_plan.hpp) against what every conv launch reports.  A ConvSpy
(tests/conv_plan_cases.py) asserts after every pam_conv2d_nhwc_bf16_ex call that the plan for the same arguments is the call's return
code and -- when it launched -- (pam_conv_last_kernel(), pam_conv_last_form()), which each launcher records from the template
parameters of the kernel it launched.  No numbers are compared here: tests/test_gpu_exact.py owns the bits."""
import ctypes

import pytest
import torch

import pam  # noqa: F401
import conv_plan_cases as P

pytestmark = pytest.mark.gpu


class Agreement(object):
    def __init__(self):
        from pam import _lib
        self.lib, self.calls, self.launched, self.bad = _lib.load(), 0, 0, []

    def wrap(self, lib):
        return P.ConvSpy(lib, self.on_conv)

    def on_conv(self, query, rc):
        k, f = ctypes.c_int32(-99), ctypes.c_int32(-99)
        prc = self.lib.pam_conv_plan(*query, ctypes.byref(k), ctypes.byref(f))
        got = (prc, k.value, f.value)
        want = (0, self.lib.pam_conv_last_kernel(), self.lib.pam_conv_last_form()) if rc == 0 else (rc, -99, -99)
        self.calls += 1
        self.launched += rc == 0
        if got != want:
            self.bad.append((dict(zip(P.INTS + P.FLAGS, query)), 'plan', got, 'launch', want))

    def done(self, at_least):
        assert not self.bad, (len(self.bad), self.bad[:10])
        assert self.launched >= at_least, (self.launched, at_least)


def test_plan_equals_every_launch_of_the_networks():
    """One forward each of HRNet-W48, HRNet-W32 and PoseResNet-50 at 2 crops and of Darknet-53, YOLOv3-tiny and YOLOv3-SPP at 1 view,
    random weights."""
    a = Agreement()
    P.drive_networks(a.wrap, torch.device('cuda:0'), crops=(2,), views=(1,))
    a.done(6 * 10)


def test_plan_equals_every_launch_of_the_conv_cases():
    """exact_ref's CONV_CASES with their own variants and over all of ALL_TILES at their own small shapes: the accepted pairs launch what
    the plan says, the refused pairs are refused by both."""
    a = Agreement()
    P.drive_cases(a.wrap, torch.device('cuda:0'))
    a.done(200)
    assert a.calls > a.launched                        # the pairs exact_ref.tile_refused names came through here too
