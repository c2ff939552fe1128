"""The composite network's backward kernels and its training step on the CPU lane emulator (tests/emu): the cases of
composite_train_cases.py.  test_composite_train_gpu.py runs the same cases on an MI355X.

Measured worst ratios (the assertion is ratio <= 1), emulator | MI355X:
    windowed warp backward, hip / (4 d32 + 16 * 2^-24)          0.23 | 0.23
    layer merge backward, hip / (4 d32 + 16 * 2^-24)            0.13 | 0.15
    windowed regression backward, warp's g_dv inside the window  bit for bit on both
    step "t": outputs, error / max(1e-4, 3 x one-ulp spread)    0.13 | 0.15      running statistics 0.004 | 0.004
    step "t": gradients, ours / (3 x max(ref draw, one-ulp draw, median ref))   0.58 | 0.45   (159 of 196 parameters element-wise)
    step "a": outputs                                            0.13 | 0.17      running statistics 0.005 | 0.005
    step "a": gradients                                          0.41 | 0.42   (159 of 264 parameters element-wise)
Distance to float64 of the gradients, median / 75th percentile, ours on the emulator | ours on the MI355X | the reference's fp32 draw:
    "t"  6.7e-6 / 4.9e-5 | 6.5e-6 / 4.8e-5 | 6.8e-6 / 5.6e-5        "a"  2.1e-5 / 2.2e-4 | 8.5e-6 / 9.0e-5 | 2.6e-5 / 4.4e-4
Every case prints its own figures under ``pytest -s``."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC
import composite_train_cases as TC

WORST = {}


def _emu():
    from emu_lib import emu_lib
    torch.set_num_threads(4)
    return emu_lib(), torch.device("cpu")


@pytest.mark.parametrize("win", TC.WINDOWS)
@pytest.mark.parametrize("C", [32, 16])
def test_window_warp_backward(C, win):
    TC.window_warp_bwd_case(*_emu(), C, win, WORST)
    print(f"[composite train] worst hip / bound so far: {WORST}")


@pytest.mark.parametrize("depth_inv", [False, True])
@pytest.mark.parametrize("D", [8, 32])
def test_window_regression_backward_is_the_padded_backward(D, depth_inv):
    from emu_lib import emu_trace
    lib, dev = _emu()
    with emu_trace(lib) as tr:
        TC.window_regression_bwd_case(lib, dev, D, depth_inv)
    names = [e[1].strip("()") for e in tr if e[0] == "launch"]
    # the launcher branch of this D: the windowed value of the very kernel enerf_depth_regression_bwd (the padded reference of the
    # case) launches for it
    windowed = TC.regression_kernel(D)
    assert windowed in names and windowed.replace(", true", "") in names, (D, names)


@pytest.mark.parametrize("L,name,ns", CC.COMPOSITE_CASES)
def test_layer_composite_backward_matches_float64(L, name, ns):
    TC.layers_bwd_case(*_emu(), L, name, ns, WORST)
    print(f"[composite train] worst hip / bound so far: {WORST}")


def test_backward_entry_refusals():
    TC.bwd_refusals(*_emu())


def test_training_step_matches_reference_case_t():
    """One step of case "t" (one layer, both levels rendered) against the unmodified reference's fp32 / float64 / one-ulp fixtures:
    loss within 1e-5, outputs and running statistics within max(1e-4, 3 x one-ulp spread), every parameter gradient as close to
    float64 as the reference's own fp32 draws (slack 3), the stable parameters element-wise at 3e-4."""
    TC.train_step_case(*_emu(), "t", WORST)
    print(f"[composite train] worst so far: {WORST}")


def test_training_step_matches_reference_case_a():
    """Case "a": two overlapping layers, both levels rendered — the sort decides the composited order."""
    TC.train_step_case(*_emu(), "a", WORST)
    print(f"[composite train] worst so far: {WORST}")


def test_training_is_opt_in():
    TC.surface_optin_case(*_emu())


def test_optimizer_step_rebuilds_packed_weights_and_refuses_stale_cache():
    TC.surface_step_case(*_emu())
