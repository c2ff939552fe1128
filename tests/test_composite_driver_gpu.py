"""The composite network's one-call driver and its preparation kernel on an MI355X: the cases of composite_driver_cases.py
(test_composite_driver.py runs them, and the trace properties, on the emulator).  Here the forked chains really overlap: three
frames in a row with the lane on must all equal the staged frame, which is what a scratch region shared across the fork would break."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_driver_cases as DC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@pytest.mark.parametrize("depth_inv", [True, False])
def test_prep_kernel_holds_the_separate_entries_bits_on_gpu(depth_inv):
    DC.prep_case(*_gpu(), depth_inv)


def test_prep_kernel_jobs_past_their_block_range_on_gpu():
    DC.prep_case(*_gpu(), True, big=True)


def test_prep_refusals_on_gpu():
    DC.prep_refusals(*_gpu())


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_one_call_equals_the_staged_path_three_frames_in_a_row_on_gpu(name):
    DC.driver_case(*_gpu(), name, frames=3)


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_other_boxes_and_back_on_gpu(name):
    DC.boxes_case(*_gpu(), name)


@pytest.mark.parametrize("name", ["b", "a"])
def test_graphed_frame_replays_equal_the_eager_frame(name):
    DC.graph_case(*_gpu(), name)
