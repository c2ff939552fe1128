"""The composite network's kernels on the CPU lane emulator (tests/emu): the cases of composite_cases.py, and the persistent raw
render walking more than one tile per wave under a small emulated CU count.  test_composite_gpu.py runs the same cases on an MI355X.

Worst errors measured on the emulator (max|x - ref| / max|ref|): raw render 8.7e-7 (raw), 7.6e-7 (z) against the bound
max(5e-6, 3 e_ref) of test_render_regimes.py; layer composite 1.0e-7 (rgb), 6.9e-8 (depth), 6.2e-8 (weights) against 1e-5; the whole
network against the reference's fixtures 1.4e-5 (net_output), 8.2e-6 (rgb) against 1e-4."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC

WORST = {}


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


@pytest.mark.parametrize("C", [32, 16])
def test_window_volume_is_the_crop(C):
    CC.window_volume_case(*_emu(), C)


@pytest.mark.parametrize("depth_inv", [False, True])
@pytest.mark.parametrize("D", [8, 32])
def test_window_regression_is_the_padded_regression(D, depth_inv):
    CC.window_regression_case(*_emu(), D, depth_inv)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_matches_float64(level, S, ns):
    CC.raw_render_case(*_emu(), False, level, S, ns, WORST)
    print(f"[composite] worst so far: {WORST}")


@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_window_selection(level):
    CC.raw_selection_case(*_emu(), False, level)


@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_walks_several_tiles_per_wave(level):
    """Emulator only: sized for 1 and 2 CUs the launch is one or two blocks (F = 35), two or four (F = 11), and 21 tiles make
    every wave walk up to three."""
    CC.raw_tile_walk_case(*_emu(), False, level, cus_list=(1, 2))


@pytest.mark.parametrize("L,name,ns", CC.COMPOSITE_CASES)
def test_layer_composite_matches_float64(L, name, ns):
    CC.composite_case(*_emu(), L, name, ns, WORST)
    print(f"[composite] worst so far: {WORST}")


def test_composite_refusals():
    CC.composite_refusals(*_emu())


def test_window_entry_refusals():
    CC.window_refusals(*_emu())


@pytest.mark.parametrize("name", list(CC.NETWORK_CASES))
def test_network_matches_reference(name):
    """Every output and every regressed depth / std map of both fixtures within 1e-4; strict state-dict load; training mode raises;
    weight rows sum to less than 1; outside every box the image is the background's own composite."""
    CC.network_case(*_emu(), name, WORST)
    print(f"[composite] worst so far: {WORST}")
