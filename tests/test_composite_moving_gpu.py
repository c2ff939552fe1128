"""The composite network with boxes that move on an MI355X: the cases of composite_moving_cases.py (test_composite_moving.py runs
them on the emulator), and what only a GPU shows — a captured ``layer_boxes -> forward_cached`` loop replayed for cameras whose boxes
land at different positions, and a frame with device positions under torch's synchronisation check."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_moving_cases as MC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@pytest.mark.parametrize("cached", [False, True], ids=["forward", "forward_cached"])
@pytest.mark.parametrize("name", ["b", "a"])
def test_device_positions_give_the_host_paths_bits_in_one_shape_on_gpu(name, cached):
    MC.same_bits_case(*_gpu(), name, cached)


@pytest.mark.parametrize("name", ["b", "a"])
def test_positions_are_clamped_into_the_image_and_flagged_on_gpu(name):
    MC.clamp_case(*_gpu(), name)
    MC.clamp_case(*_gpu(), name, cached=True)


@pytest.mark.parametrize("Cc", [16, 32])
def test_windowed_volume_with_a_corner_on_the_device_on_gpu(Cc):
    MC.volume_at_case(*_gpu(), Cc)


@pytest.mark.parametrize("D", [8, 32])
def test_windowed_regression_with_a_corner_on_the_device_on_gpu(D):
    MC.regression_at_case(*_gpu(), D)


@pytest.mark.parametrize("L", [1, 2, 4])
def test_layer_merge_with_corners_on_the_device_on_gpu(L):
    MC.layers_at_case(*_gpu(), L)


@pytest.mark.parametrize("which", list(MC.BOX_CASES))
def test_layer_boxes_against_the_float64_restatement_on_gpu(which):
    MC.layer_boxes_case(*_gpu(), which)


def test_graphed_layer_boxes_and_cached_frame_replay_with_moved_boxes():
    MC.graph_case(*_gpu())


def test_frame_with_device_positions_does_not_synchronise():
    MC.no_sync_case(*_gpu())


def test_network_refusals_on_gpu():
    MC.network_refusals_case(*_gpu())


def test_c_entry_refusals_on_gpu():
    MC.c_refusals_case(*_gpu(), traced=False)
