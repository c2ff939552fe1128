"""The composite network's backward kernels and its training step on an MI355X through the C ABI: the cases of
composite_train_cases.py (test_composite_train.py runs them on the emulator; the measured worst ratios of both are in its docstring).
Reads only tests/golden/."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC
import composite_train_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
WORST = {}


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@pytest.mark.parametrize("win", TC.WINDOWS)
@pytest.mark.parametrize("C", [32, 16])
def test_window_warp_backward_on_gpu(C, win):
    TC.window_warp_bwd_case(*_gpu(), C, win, WORST)
    print(f"[composite train] worst hip / bound so far: {WORST}")


@pytest.mark.parametrize("depth_inv", [False, True])
@pytest.mark.parametrize("D", [8, 32])
def test_window_regression_backward_is_the_padded_backward_on_gpu(D, depth_inv):
    TC.window_regression_bwd_case(*_gpu(), D, depth_inv)


@pytest.mark.parametrize("L,name,ns", CC.COMPOSITE_CASES)
def test_layer_composite_backward_matches_float64_on_gpu(L, name, ns):
    TC.layers_bwd_case(*_gpu(), L, name, ns, WORST)
    print(f"[composite train] worst hip / bound so far: {WORST}")


def test_backward_entry_refusals_on_gpu():
    TC.bwd_refusals(*_gpu())


@pytest.mark.parametrize("name", list(TC.TRAIN_CASES))
def test_training_step_matches_reference_on_gpu(name):
    TC.train_step_case(*_gpu(), name, WORST)
    print(f"[composite train] worst so far: {WORST}")


def test_training_is_opt_in_on_gpu():
    TC.surface_optin_case(*_gpu())


def test_optimizer_step_rebuilds_packed_weights_and_refuses_stale_cache_on_gpu():
    TC.surface_step_case(*_gpu())
