"""The composite network's one-call driver and its preparation kernel on the CPU lane emulator (tests/emu): the cases of
composite_driver_cases.py.  The emulator runs launches in enqueue order, so here the forked frame must equal the staged one bit
for bit, and the fork / join discipline — which a GPU run can satisfy by luck — is checked on the launch trace.
test_composite_driver_gpu.py runs the value cases on an MI355X, where the chains really overlap.

The plan repeats every refusal of the stage entries that depends on the arguments alone — the raw render's sample count and size
limits among them — so the refusal tests find an empty trace for each; behind the fork only a launch error or a layer shape no
convolution kernel takes could still fail (frame.hip CompositeRun::bail joins the lane then), and no argument of these tests
reaches either, so there is no error-after-the-fork test here."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_driver_cases as DC


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


@pytest.mark.parametrize("depth_inv", [True, False])
def test_prep_kernel_holds_the_separate_entries_bits(depth_inv):
    DC.prep_case(*_emu(), depth_inv)


def test_prep_kernel_jobs_past_their_block_range():
    DC.prep_case(*_emu(), True, big=True)


def test_prep_refusals():
    DC.prep_refusals(*_emu())


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_one_call_equals_the_staged_path(name):
    DC.driver_case(*_emu(), name)


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_other_boxes_and_back(name):
    DC.boxes_case(*_emu(), name)


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_trace_same_kernels_forked_layers_joined_merges(name):
    DC.trace_case(*_emu(), name)


@pytest.mark.parametrize("which", list(DC.REFUSALS))
def test_refusals_name_the_field_and_enqueue_nothing(which):
    DC.refusal_case(*_emu(), which)


def test_unaligned_box_that_leaves_the_image_is_refused_by_both_drivers():
    DC.unaligned_box_outside_case(*_emu())


def test_null_args_are_refused():
    DC.refusal_null_args(*_emu())


def test_network_raises_the_plans_refusal_and_enqueues_nothing():
    DC.refusal_through_the_network(*_emu())


def test_driver_argument_is_checked():
    from enerf_amd.network_composite import Network
    with pytest.raises(ValueError, match="driver"):
        Network(DC.config("b"), 1, lib=_emu()[0], driver="fused")
