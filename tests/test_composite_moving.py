"""The composite network with boxes that move — sizes on the host, positions on the device — on the CPU lane emulator (tests/emu): the
cases of composite_moving_cases.py.  A frame with ``bbox_size`` + ``bbox_xy`` must equal the frame with ``bbox`` BIT FOR BIT at
every position, without a new shape; what a GPU run cannot show — that a refusal enqueues nothing — is checked here.
test_composite_moving_gpu.py runs the cases on an MI355X, and the graph replay."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_moving_cases as MC


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


@pytest.mark.parametrize("cached", [False, True], ids=["forward", "forward_cached"])
@pytest.mark.parametrize("name", ["b", "a"])
def test_device_positions_give_the_host_paths_bits_in_one_shape(name, cached):
    MC.same_bits_case(*_emu(), name, cached)


@pytest.mark.parametrize("name", ["b", "a"])
def test_positions_are_clamped_into_the_image_and_flagged(name):
    MC.clamp_case(*_emu(), name)


@pytest.mark.parametrize("Cc", [16, 32])
def test_windowed_volume_with_a_corner_on_the_device(Cc):
    MC.volume_at_case(*_emu(), Cc)


@pytest.mark.parametrize("D", [8, 32])
def test_windowed_regression_with_a_corner_on_the_device(D):
    MC.regression_at_case(*_emu(), D)


@pytest.mark.parametrize("L", [1, 2, 4])
def test_layer_merge_with_corners_on_the_device(L):
    MC.layers_at_case(*_emu(), L)


@pytest.mark.parametrize("which", list(MC.BOX_CASES))
def test_layer_boxes_against_the_float64_restatement(which):
    MC.layer_boxes_case(*_emu(), which)


def test_network_refusals():
    MC.network_refusals_case(*_emu())


def test_c_entry_refusals_name_the_field_and_enqueue_nothing():
    MC.c_refusals_case(*_emu(), traced=True)
